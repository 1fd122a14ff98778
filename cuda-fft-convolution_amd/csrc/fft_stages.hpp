// fft_stages.hpp -- the pieces of the three-stage in-LDS transform that the specialised workgroup bodies share
// (fast_rows_multi.hpp, fast_rows_fwd.hpp, fast_cols.hpp, fast_cols_fwd.hpp), written once.
//
// A transform of R1 * R2 * R3 points lives in LDS as R1 stage-1 blocks S1 cells apart; a stage-2 butterfly works on cells R3
// apart, a stage-3 butterfly on a contiguous run of R3 cells.  Each helper gets a pointer to the first cell of its butterfly
// and registers, nothing else: which butterfly a thread takes, the guards around it, the phase it runs in and where the
// results go in global memory stay with the bodies.  The helpers are forced inline and add no instruction of their own: a
// body that uses one compiles to the device code it had with the lines spelled out (tools/isa_same.py against the parent
// commit's listings is how that is checked; history/stage_helpers.md has the form lessons).
#pragma once
#include "butterflies.hpp"
#include "fc_common.hpp"

namespace fc {

// ---- stage 3: a run of R cells, 16 bytes (two cells) at a time
template <int R>
FC_HD void run_load(const c32* p, c32 (&v)[R]) {
    static_for<0, R / 2>([&](auto h_) {
        constexpr int h = decltype(h_)::value;
        c32x2 w = *reinterpret_cast<const c32x2*>(p + 2 * h);
        v[2 * h] = w.a;
        v[2 * h + 1] = w.b;
    });
}
template <int R>
FC_HD void run_store(c32* p, const c32 (&v)[R]) {
    static_for<0, R / 2>([&](auto h_) {
        constexpr int h = decltype(h_)::value;
        c32x2 w;
        w.a = v[2 * h];
        w.b = v[2 * h + 1];
        *reinterpret_cast<c32x2*>(p + 2 * h) = w;
    });
}

// ---- stage-2 twiddles of the butterfly at offset b of its block: each(f) calls f(IC<c>, w_c) for c = 1 .. R2 - 1.
// The plain LDS table [(c - 1) * R3 + b] of the column kernels ...
template <int R2, int R3>
struct Tw2Plain {
    const c32* tw2;
    int b;
    template <class F>
    FC_HD void each(F&& f) const {
        static_for<1, R2>([&](auto c_) {
            constexpr int c = decltype(c_)::value;
            f(c_, tw2[(c - 1) * R3 + b]);
        });
    }
};
// ... and the row kernels' image of it that is read two twiddles at a time (fc_common.hpp: fc_tw2_fill)
template <int R2>
struct Tw2Paired {
    const c32* tw2;
    int b;
    template <class F>
    FC_HD void each(F&& f) const { fc_tw2_each<R2>(tw2, b, f); }
};

// ---- forward stage 2, output side: butterfly of the R2 inputs in v (inputs a >= NZ2 structural zeros; NZ2 == R2: unpruned, the
// plain butterfly), results times their twiddles to cells R3 apart
template <int R2, int R3, int NZ2, class Tw>
FC_HD void fwd_stage2_out(c32* p, c32 (&v)[R2], const Tw& tw) {
    if constexpr (NZ2 < R2) Dft<R2, -1>::template run_nz<NZ2>(v);
    else Dft<R2, -1>::run(v);
    p[0] = v[0];
    tw.each([&](auto c_, c32 w) {
        constexpr int c = decltype(c_)::value;
        p[c * R3] = cmul(v[c], w);
    });
}
// ---- inverse stage 2 of one butterfly, in place
template <int R2, int R3, class Tw>
FC_HD void inv_stage2(c32* p, const Tw& tw) {
    c32 v[R2];
    v[0] = p[0];
    tw.each([&](auto c_, c32 w) {
        constexpr int c = decltype(c_)::value;
        v[c] = cmulc(p[c * R3], w);
    });
    Dft<R2, +1>::run(v);
    static_for<0, R2>([&](auto a_) {
        constexpr int a = decltype(a_)::value;
        p[a * R3] = v[a];
    });
}

// ---- forward stage 1, output side: block c of the row gets x[c] * pw[c] (pw[c] = w^c of this butterfly, power_chain) ...
template <int R1, int S1>
FC_HD void fwd_stage1_out(c32* q, int j, const c32 (&x)[R1], const c32 (&pw)[R1]) {
    q[j] = x[0];
    static_for<1, R1>([&](auto c_) {
        constexpr int c = decltype(c_)::value;
        q[c * S1 + j] = cmul(x[c], pw[c]);
    });
}
// ... and pruned: the butterfly has one non-zero input x, so every output is x
template <int R1, int S1>
FC_HD void fwd_stage1_out_pruned(c32* q, int j, c32 x, const c32 (&pw)[R1]) {
    q[j] = x;
    static_for<1, R1>([&](auto c_) {
        constexpr int c = decltype(c_)::value;
        q[c * S1 + j] = cmul(x, pw[c]);
    });
}
// ---- inverse stage 1, input side and butterfly
template <int R1, int S1>
FC_HD void inv_stage1_in(const c32* p, int j, const c32 (&pw)[R1], c32 (&v)[R1]) {
    v[0] = p[j];
    static_for<1, R1>([&](auto c_) {
        constexpr int c = decltype(c_)::value;
        v[c] = cmulc(p[c * S1 + j], pw[c]);
    });
    Dft<R1, +1>::run(v);
}

}  // namespace fc
