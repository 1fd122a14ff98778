// column_cache.hpp -- the record of what a plan's column-spectrum buffer A holds between calls.
// Host-only and HIP-free (the stream is an opaque pointer): tests/column_cache_host drives it with the plain host compiler.
#pragma once

// n packed kernels of one size at dk whose column spectra are (or are to be) in A, and the stream that orders A's contents
struct KernelSet {
    const float* dk = nullptr;
    int n = 0, kh = 0, kw = 0;
    void* stream = nullptr;
    bool operator==(const KernelSet& o) const { return dk == o.dk && n == o.n && kh == o.kh && kw == o.kw && stream == o.stream; }
};

// Always in ONE of three states:
//   Empty    nothing is known about A
//   Pending  fftconv_plan_prepare_kernels_packed DEFERRED: a recorded request whose column pass is launched by whichever comes
//            first, the next set_image on the same stream (then in ONE launch with the image's column pass:
//            launch_fast_cols_fwd_pair) or the next convolve / any call that must see it done (flush_pending_prepare)
//   Ready    the column spectra of the set's first chunk are in A, ordered on the set's stream
// Every invalidation of the plan is one call here: forget (A's contents, or what they depend on, are about to change),
// consume (A is about to be read or overwritten) or source_overwritten (the kernels behind the record are).
class ColumnCache {
public:
    struct Request : KernelSet { int na = 0; };   // (na: kernels of the first chunk)

    bool pending() const { return state_ == Pending; }
    bool pending_off_stream(const void* stream) const { return state_ == Pending && rec_.stream != stream; }
    void request(const KernelSet& ks, int na) {
        static_cast<KernelSet&>(rec_) = ks;
        rec_.na = na;
        state_ = Pending;
    }
    // Pending -> Empty: the caller launches `out` and, if that succeeded, says ready(out)
    bool take_pending(Request& out) {
        if (state_ != Pending) return false;
        out = rec_;
        state_ = Empty;
        return true;
    }
    void ready(const KernelSet& ks) {
        static_cast<KernelSet&>(rec_) = ks;
        state_ = Ready;
    }
    // at the start of a chunk of the per-kernel loop: whether A holds the first chunk of `want`; whatever it held is consumed
    bool consume(const KernelSet& want) {
        if (state_ != Ready) return false;
        state_ = Empty;
        return rec_ == want;
    }
    // the caller knows that A holds ks (block-wise plans: the block before left it there); a recorded request stands
    void adopt(const KernelSet& ks) {
        if (state_ != Pending) ready(ks);
    }
    void forget() { state_ = Empty; }
    void source_overwritten(const float* dk) {
        if (state_ != Empty && rec_.dk == dk) state_ = Empty;
    }

private:
    enum State { Empty, Pending, Ready } state_ = Empty;
    Request rec_;
};
