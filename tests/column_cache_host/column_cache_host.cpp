// column_cache_host.cpp -- TEST-ONLY stand-alone host program for csrc/column_cache.hpp (ColumnCache: the record of what a plan's
// column-spectrum buffer A holds).
//
// Built by tests/test_column_cache_host.py with the host compiler from the product's header alone.  A miniature plan -- the cache, the
// current stream and nothing else -- goes through the calls that touch the record in the library, each written as its call site is
// (fftconv_api.cpp: prepare_kernels, flush_pending_prepare, run_group_impl, fftconv_plan_convolve, fftconv_plan_set_stream,
// kLongOptions; plan_image.cpp: the flush and the pair launch of set_images_impl, as image_route.hpp decides them; blockwise.cpp:
// tiled_convolve_save), next to a ground-truth model of A: which set's first
// chunk it holds, of which contents of the set's memory, written on which stream -- or garbage.  Modes:
//   walk     EVERY sequence of those calls up to a fixed length: a hit (the kernels' column pass skipped) only where the model's A
//            holds exactly the wanted set's first chunk, written on the wanted stream; a recorded request and a ready record never
//            together; a consumed record never hits twice
//   hits     the sequences the library documents as hits do hit, with the launches they are documented to take
// Having its own main, it is also the place for a host sanitizer build (-fsanitize=address,undefined) of this code.
#include <chrono>
#include <cstdio>
#include <cstring>

#include "column_cache.hpp"

namespace {

int g_failures = 0;
long g_ok = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (g_failures++ < 20) {                      \
                printf("FAIL ");                          \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        } else g_ok++;                                    \
    } while (0)

// where a failing check stands: the directed sequence's name, or the walk's operations so far
const char* g_label = "";
int g_ops[8], g_nops = 0;
const char* where() {
    static char buf[96];
    if (!g_nops) return g_label;
    buf[0] = 0;
    for (int i = 0; i < g_nops; i++) snprintf(buf + strlen(buf), sizeof(buf) - strlen(buf), "%s%d", i ? "," : "ops ", g_ops[i]);
    return buf;
}

float g_mem[2];      // the kernels of set X and of set Y live here (addresses only)
int g_streams[2];
constexpr int N = 4, CHUNK = 2;      // kernels of a set; kernels of a chunk in the two-chunk convolve

// what A really holds
struct TruthA {
    bool valid = false;      // false: garbage, or a chunk other than a set's first
    KernelSet set;
    int version = 0;         // of the contents of the set's memory when its columns were transformed
};

struct MiniPlan {
    ColumnCache a_holds;
    int cur = 0;             // index of the plan's stream
    TruthA A;
    int version[2] = {0, 0};      // contents of g_mem[i]: bumped when the library overwrites them
    int kernel_col_launches = 0, pair_launches = 0, hits = 0;

    void* stream() const { return &g_streams[cur]; }
    KernelSet set(int which) const { return KernelSet{&g_mem[which], N, 5, 5, stream()}; }
    static int mem_of(const KernelSet& ks) { return (int)(ks.dk - g_mem); }
    bool truth_holds(const KernelSet& want) const {      // (field by field: not through the operator under test)
        return A.valid && A.set.dk == want.dk && A.set.n == want.n && A.set.kh == want.kh && A.set.kw == want.kw && A.set.stream == want.stream &&
               A.version == version[mem_of(want)];
    }

    // launch_kernel_cols: chunk [a0, ...) of ks into A, on `on`
    void launch_kernel_cols(const KernelSet& ks, int a0, void* on) {
        kernel_col_launches++;
        A.valid = a0 == 0;
        A.set = ks;
        A.set.stream = on;
        A.version = version[mem_of(ks)];
    }
    void flush_pending_prepare() {
        ColumnCache::Request pd;
        if (!a_holds.take_pending(pd)) return;
        launch_kernel_cols(pd, 0, pd.stream);
        a_holds.ready(pd);
    }
    void prepare(int which, bool defer) {
        flush_pending_prepare();
        a_holds.forget();
        const KernelSet ks = set(which);
        if (defer) { a_holds.request(ks, CHUNK); return; }
        launch_kernel_cols(ks, 0, stream());
        a_holds.ready(ks);
    }
    void set_image() {
        if (a_holds.pending_off_stream(stream())) flush_pending_prepare();
        ColumnCache::Request pd;
        if (a_holds.take_pending(pd)) {      // the pair launch
            pair_launches++;
            A.valid = true;
            A.set = pd;
            A.set.stream = stream();
            A.version = version[mem_of(pd)];
            a_holds.ready(pd);
        }
    }
    // run_group_impl over `chunks` chunks; returns whether the first chunk's column pass was skipped
    bool convolve(int which, int chunks, const char* label = "") {
        g_label = label;
        flush_pending_prepare();
        const KernelSet want = set(which);
        bool first_hit = false;
        for (int c = 0; c < chunks; c++) {
            const int a0 = c * CHUNK;
            const bool have_cols = a_holds.consume(want) && a0 == 0;
            if (have_cols) {
                hits++;
                CHECK(truth_holds(want), "safety: %s: a hit for set %d on stream %d, but A %s", where(), which, cur,
                      !A.valid ? "holds garbage" : A.set.dk != want.dk ? "holds the other set" : A.set.stream != want.stream ? "was written on the other stream"
                                                                                                                           : "holds the columns of overwritten kernels");
                first_hit = true;
            } else
                launch_kernel_cols(want, a0, stream());
            ColumnCache again = a_holds;
            CHECK(!again.consume(want), "%s: a consumed record hits again (chunk %d)", where(), c);
        }
        return first_hit;
    }
    // the next block of a block-wise plan: the caller knows that the block before left `which` in A
    void adopt(int which) {
        if (!truth_holds(set(which))) return;
        const bool was_pending = a_holds.pending();
        a_holds.adopt(set(which));
        CHECK(a_holds.pending() == was_pending, "%s: adopt %s a request", where(), was_pending ? "dropped" : "made");
    }
    // an option with OPT_FORGETS changes: what A holds is no longer what a column pass would write now
    void option_changed() {
        A.valid = false;
        a_holds.forget();
    }
    void kernels_overwritten(int which) {      // the pin_k gather of fftconv_plan_convolve
        version[which]++;
        a_holds.source_overwritten(&g_mem[which]);
    }
    void set_stream(int to) {
        if (a_holds.pending()) flush_pending_prepare();
        cur = to;
    }
    // a recorded request excludes a ready record: nothing can hit while one is pending
    void check_exclusion() {
        if (!a_holds.pending()) return;
        for (int which = 0; which < 2; which++)
            for (int s = 0; s < 2; s++) {
                ColumnCache probe = a_holds;
                KernelSet want = set(which);
                want.stream = &g_streams[s];
                CHECK(!probe.consume(want), "exclusion: %s: a request is pending and set %d on stream %d hits", where(), which, s);
                CHECK(probe.pending(), "exclusion: %s: consume dropped a pending request", where());
            }
    }
};

const char* const kOps[] = {"request X", "request Y", "prepare X", "flush", "set_image", "convolve X", "convolve Y", "convolve X in two chunks",
                            "adopt X", "forget (an option changed)", "kernels of X overwritten", "switch stream"};
constexpr int NOPS = sizeof(kOps) / sizeof(kOps[0]);

void apply(MiniPlan& p, int op) {
    switch (op) {
        case 0: p.prepare(0, true); break;
        case 1: p.prepare(1, true); break;
        case 2: p.prepare(0, false); break;
        case 3: p.flush_pending_prepare(); break;
        case 4: p.set_image(); break;
        case 5: p.convolve(0, 1); break;
        case 6: p.convolve(1, 1); break;
        case 7: p.convolve(0, 2); break;
        case 8: p.adopt(0); break;
        case 9: p.option_changed(); break;
        case 10: p.kernels_overwritten(0); break;
        case 11: p.set_stream(1 - p.cur); break;
    }
    p.check_exclusion();
}

long g_sequences = 0, g_hits = 0;

void walk(const MiniPlan& p, int depth, int length) {
    if (depth == length) return;
    for (int op = 0; op < NOPS; op++) {
        g_ops[depth] = op;
        g_nops = depth + 1;
        MiniPlan q = p;
        q.hits = 0;
        apply(q, op);
        g_sequences++;
        g_hits += q.hits;
        walk(q, depth + 1, length);
    }
}

int cmd_walk() {
    constexpr int LENGTH = 7;
    const auto t0 = std::chrono::steady_clock::now();
    walk(MiniPlan(), 0, LENGTH);
    g_nops = 0;
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int i = 0; i < NOPS; i++) printf("op %d: %s\n", i, kOps[i]);
    printf("length %d over %d operations: %ld sequences (every prefix counted), %ld hits, %.2f s\n", LENGTH, NOPS, g_sequences, g_hits, s);
    CHECK(g_hits > 0, "no sequence hit: the walk checks nothing");
    printf("walk: %ld checks ok, %d failed\n", g_ok, g_failures);
    return g_failures ? 1 : 0;
}

int cmd_hits() {
    {   // prepare, then convolve of the same set: one column pass, in the prepare
        MiniPlan p;
        p.prepare(0, false);
        CHECK(p.convolve(0, 1, "prepare, convolve") && p.kernel_col_launches == 1, "prepare then convolve: %d column passes", p.kernel_col_launches);
        // ... and consumed: the second convolve transforms its kernels again (mutation 2 of tests/test_plan_walk_gpu.py)
        CHECK(!p.convolve(0, 1, "prepare, convolve, convolve") && p.kernel_col_launches == 2, "a consumed record hit again");
    }
    {   // deferred prepare, then convolve: the request is launched by the convolve, once
        MiniPlan p;
        p.prepare(0, true);
        CHECK(p.a_holds.pending() && p.kernel_col_launches == 0, "a deferred prepare launched or did not record");
        CHECK(p.convolve(0, 1, "request, convolve") && p.kernel_col_launches == 1 && !p.a_holds.pending(), "request then convolve");
    }
    {   // a request whose launch fails leaves nothing behind: taken is gone, whether or not ready() follows
        MiniPlan p;
        p.prepare(0, true);
        ColumnCache::Request pd;
        CHECK(p.a_holds.take_pending(pd) && pd.dk == &g_mem[0] && pd.na == CHUNK && pd.stream == &g_streams[0], "take_pending did not return the request");
        CHECK(!p.a_holds.pending() && !p.a_holds.take_pending(pd), "a taken request is still pending");
        CHECK(!p.convolve(0, 1, "request, failed launch, convolve"), "a request that was never launched hit");
    }
    {   // deferred prepare, then set_image, then convolve: ONE pair launch and no column pass of the kernels' own
        MiniPlan p;
        p.prepare(0, true);
        p.set_image();
        CHECK(!p.a_holds.pending() && p.pair_launches == 1, "set_image did not take the request");
        CHECK(p.convolve(0, 1, "request, set_image, convolve") && p.kernel_col_launches == 0 && p.pair_launches == 1, "request, set_image, convolve");
    }
    {   // a deferred prepare on stream 0, a switch away (launches it, on stream 0) and back, then convolve
        MiniPlan p;
        p.prepare(0, true);
        p.set_stream(1);
        CHECK(!p.a_holds.pending() && p.kernel_col_launches == 1 && p.A.set.stream == &g_streams[0], "the switch did not launch the request on its own stream");
        {
            MiniPlan q = p;      // on the other stream the record does not count ...
            CHECK(!q.convolve(0, 1, "request, switch, convolve"), "a record of stream 0 hit on stream 1");
        }
        p.set_image();           // (the multi-GPU step: an image on the side stream leaves the record alone)
        p.set_stream(0);         // ... and counts again once the plan is back
        CHECK(p.convolve(0, 1, "request, switch, switch, convolve") && p.kernel_col_launches == 1, "request, switch away and back, convolve");
    }
    {   // a request on another stream than the image's: flushed on its own stream, no pair launch
        MiniPlan p;
        p.prepare(0, true);
        p.cur = 1;               // (the stream changed behind the record: what pending_off_stream is for)
        p.set_image();
        CHECK(p.pair_launches == 0 && p.kernel_col_launches == 1 && p.A.set.stream == &g_streams[0], "a request of stream 0 rode in an image launch on stream 1");
    }
    {   // adopt across blocks: block 0 transforms, every later block reuses
        MiniPlan p;
        CHECK(!p.convolve(0, 1, "block 0"), "block 0 hit on an empty record");
        for (int b = 1; b < 4; b++) {
            p.adopt(0);
            CHECK(p.convolve(0, 1, "block b"), "block %d did not reuse block 0's column spectra", b);
        }
        CHECK(p.kernel_col_launches == 1, "%d column passes over four blocks", p.kernel_col_launches);
        // ... but a recorded request stands, and adopt leaves it alone
        p.prepare(1, true);
        p.A.valid = true; p.A.set = p.set(0);      // (as if A held X)
        p.a_holds.adopt(p.set(0));
        CHECK(p.a_holds.pending(), "adopt dropped a pending request");
    }
    {   // the kernels behind a record are overwritten: neither a ready record nor a request survives
        MiniPlan p;
        p.prepare(0, false);
        p.kernels_overwritten(0);
        CHECK(!p.convolve(0, 1, "prepare, overwrite, convolve"), "a record of overwritten kernels hit");
        p.prepare(0, true);
        p.kernels_overwritten(0);
        CHECK(!p.a_holds.pending(), "a request for overwritten kernels stands");
        p.prepare(1, true);
        p.kernels_overwritten(0);
        CHECK(p.a_holds.pending(), "a request for other kernels was dropped");
    }
    {   // forget: an option the column spectra depend on (mutations 1 and 5)
        MiniPlan p;
        p.prepare(0, false);
        p.option_changed();
        CHECK(!p.convolve(0, 1, "prepare, forget, convolve"), "a forgotten record hit");
        p.prepare(0, true);
        p.option_changed();
        CHECK(!p.a_holds.pending(), "a forgotten request stands");
    }
    printf("hits: %ld checks ok, %d failed\n", g_ok, g_failures);
    return g_failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "walk")) return cmd_walk();
    if (!strcmp(mode, "hits")) return cmd_hits();
    fprintf(stderr, "usage: column_cache_host walk|hits\n");
    return 2;
}
