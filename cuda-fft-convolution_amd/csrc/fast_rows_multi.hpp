// fast_rows_multi.hpp -- spectral-row kernel, several maps per workgroup.
//
// A workgroup per (row group, kernel) pair pays the launch, the stage-2 twiddle fill, the exposed latency of its
// kernel-row load and a fresh fetch of the image-spectrum row, and it retires only after its stores have
// drained.  Here a workgroup keeps its image-spectrum row IN REGISTERS and walks G consecutive
// kernels with it (G = 1: the one-map launch of small problems):
//   * the image-spectrum row is fetched once per G maps instead of once per map (the largest
//     read of this kernel: 8*C bytes per map -> 8*C/G);
//   * the next kernel's row (kw complex values: one or two registers per thread) is prefetched
//     right after stage 1 has consumed the current one, so its latency hides behind four phases;
//   * the stores of map m drain while map m + 1 is transformed.
// P5 ends with a barrier because the next
// map's P1 overwrites the LDS row.
// MULTIF (F > 1, the reference's sumAlongFeatures case): the walk runs over (map, feature) pairs.  The
// image-spectrum row of feature f cannot stay in registers (F rows), so it is fetched at the start of
// P3 -- from the XCD's L2: the workgroups walking the same row for other maps run beside this one --
// and lands while the stage-3 butterfly is computed; the feature sum is kept in registers and only
// the last feature runs the inverse phases.  What the walk still saves per map: the launch, the
// twiddle fill, the store drain and the exposed kernel-row load of every (map, feature) step.
#pragma once
#include "fast_rows.hpp"

namespace fc {

// Does the walk keep the even powers of the stage-1 twiddle (w^2, w^4, ...: R1 / 2 - 1 values per round) in registers instead of
// forming the whole chain again for every map?  Where the registers are there: one row per workgroup, F = 1 (the F > 1 walk
// holds a feature sum besides), at most FC_ROWS_KEEP_REGS registers of them, and a stage 3 of 14 to 24 points: these kernels
// run three or four waves per SIMD with registers to spare, whereas 4160 = 8.20.26 spills 24 registers with the powers kept and
// 1088 = 8.17.8 drops from five waves to four (the build's *.rpt files, tools/rpt_summary.py).
#ifndef FC_ROWS_KEEP_REGS
#define FC_ROWS_KEEP_REGS 18
#endif
template <class C, bool MULTIF>
constexpr bool row_multi_keeps_even_powers() {
    return !MULTIF && C::RPW == 1 && C::R1 >= 4 && 2 * (C::R1 / 2 - 1) * C::RND1 <= FC_ROWS_KEEP_REGS && C::R3 >= 14 && C::R3 <= 24;
}

// (FILTER: the registers are not there -- 4224 and 3520 spill 9 with the powers kept beside the filter's temporaries; the chain
//  formed again is the same bits, power_chain_from_even)
template <class C, bool MULTIF = false, bool FILTER = false>
struct RowMultiState {
    static constexpr bool KEEP = !FILTER && row_multi_keeps_even_powers<C, MULTIF>();
    static constexpr int NEVEN = C::R1 / 2 - 1;
    c32 s[C::R3];        // image spectrum of this thread's stage-3 butterfly (F = 1: whole walk; MULTIF: one step)
    c32 acc[MULTIF ? C::R3 : 1];   // feature sum of the current map (MULTIF)
    c32 x[C::RND1];      // kernel row of the current / next map
    c32 w1[C::RND1];     // stage-1 base twiddle w_L^j of this thread's butterflies (same for every map)
    c32 w1even[KEEP ? C::RND1 * NEVEN : 1];   // KEEP: its even powers, round by round
    // where this thread's stage-1 outputs go within a map (same for every map): the BYTE offset of output 0 of round r's
    // butterfly, row and column summed once (see P5)
    int yoff[C::RND1];
    int xoff;            // one row per workgroup: byte offset of this thread's round-0 element in a kernel row
};

// LINEAR: always true (fast_rows_visit_linear, fast_paths.hpp).  It once chose between two forms of P5; the other one (per-output
// tile arithmetic, for an m1 that is no whole number of half layout tiles) had no configuration and is gone: RowCfg asserts
// the condition.  The argument itself is still to be deleted, together with the visitor and the argument of the two kernels.
// FILTER (F = 1; k_fast_rows_filter, fftconv_plan_set_spectral_filter): the product of P3 is the pointwise function of
// spectral_filter.hpp that g.filter_mode names -- one instantiation per configuration for all modes, everything else as it is.

// Issue priority by phase (F = 1, no filter; FC_ROWS_PRIO, fc_common.hpp).  The SIMD's arbiter takes the oldest ready wave first, so
// of the workgroups resident on a CU the old ones run ahead and the young ones wait, whatever phase they are in.  A wave in P3
// (butterflies of 22 points and the product: arithmetic for every free slot) that wins against a wave in a stage-2 phase
// leaves the LDS pipe idle.  FC_ROWS_PRIO_POLICY:
//   0  every phase at the default priority (the kernels before this switch, instruction for instruction)
//   1  the phases that feed the LDS and the memory pipes -- the prefetch and P2, P4, P5 -- at priority 1, P3 at 0: two s_setprio
//      per map.  19.46 -> 18.27 us per map at 4224, 5.02 -> 4.78 at 2112 (medians of five alternating legs a side, spreads 0.15
//      and 0.34; profiles/rows_issue_slots_ab.txt).
// (P5 alone at priority 1 measured 19.22 at 4224 and is gone)
#ifndef FC_ROWS_PRIO_POLICY
#define FC_ROWS_PRIO_POLICY 1
#endif

template <class C, int NZ2, bool LINEAR, bool MULTIF = false, bool FILTER = false, class Ctx>
FC_HD void fast_rows_multi_body(Ctx& ctx, c32* lds, const FastRowsArgs& g, int group, int kernel0, int nk, int rows) {
    static_assert(LINEAR, "the row kernel has one form of its last phase");
    static_assert(!(FILTER && MULTIF), "the filter of a feature sum is another formula");
    constexpr int L = C::L, R1 = C::R1, R2 = C::R2, R3 = C::R3, NT = C::NT, m1 = C::m1, RPW = C::RPW, S1 = C::S1, LR = C::LR;
    using State = RowMultiState<C, MULTIF, FILTER>;
    const int nF = MULTIF ? g.F : 1;
    c32* tw2 = lds + RPW * LR;
    const int kw = g.kw;
    const int row0 = group * RPW;
    const bool tiled = g.y_row_of != nullptr;
    constexpr int PRIO = (MULTIF || FILTER) ? 0 : FC_ROWS_PRIO_POLICY;

    // st.x is zeroed once (below) and only the lanes that hold a kernel element ever load into it: no zero is materialised per map
    auto load_x = [&](int t, State& st, int kernel, int f) {
        const c32* abase = g.A + (size_t)kernel * g.a_kernel_stride + (MULTIF ? (size_t)f * g.a_feat_stride : 0);
        static_for<0, C::RND1>([&](auto r_) {
            constexpr int r = decltype(r_)::value;
            int u = t + NT * r;
            if constexpr (MULTIF) FC_OPAQUE(u);   // F > 1: index arithmetic recomputed per step, not hoisted out of the walk and spilled
            int rr, j;
            const bool slot = row_slot<RPW, C::NB1, NT, r>(u, rr, j);
            const int row = row0 + rr;
            if (slot && row < rows && j < kw) {
                if constexpr (RPW == 1) {
                    // one row per workgroup: the uniform row address, the thread's 32-bit byte offset and the round as an immediate --
                    // the load takes all three as they are (FC_OPAQUE, in place and free: see the stores of P5)
                    FC_OPAQUE(st.xoff);
                    st.x[r] = *reinterpret_cast<const c32*>(reinterpret_cast<const char*>(abase + (size_t)row * g.a_pitch) + (size_t)(unsigned)st.xoff + (size_t)(NT * r) * sizeof(c32));
                } else {
                    st.x[r] = abase[(size_t)row * g.a_pitch + j];
                }
            }
        });
    };
    // MULTIF, P3: register pairs [H0, H1) of feature f's image-spectrum row for stage-3 butterfly q of row rr (zeros past the last row)
    auto load_s = [&](State& st, int f, int rr, int q, auto h0_, auto h1_) {
        constexpr int H0 = decltype(h0_)::value, H1 = decltype(h1_)::value;
        if (row0 + rr < rows) {
            const c32* srow = g.S + (size_t)f * g.s_feat_stride + (size_t)(row0 + rr) * g.s_pitch;
            static_for<H0, H1>([&](auto h_) {
                constexpr int h = decltype(h_)::value;
                c32x2 w = *reinterpret_cast<const c32x2*>(srow + (size_t)(h * C::NB3 + q) * 2);
                st.s[2 * h] = w.a;
                st.s[2 * h + 1] = w.b;
            });
        } else {
            static_for<2 * H0, 2 * H1>([&](auto a_) { st.s[decltype(a_)::value] = mk(0.f, 0.f); });
        }
    };

    // p[c] = w1^c of round r's butterfly
    auto stage1_chain = [&](auto r_, State& st, c32 (&p)[R1]) {
        constexpr int r = decltype(r_)::value;
        if constexpr (State::KEEP) power_chain_from_even<R1>(st.w1[r], &st.w1even[r * State::NEVEN], p);
        else power_chain<R1>(st.w1[r], p);
    };

    // once per workgroup: stage-2 twiddles into LDS, first kernel row, image-spectrum row
    ctx.phase_nosync([&](int t, State& st) {
        fc_tw2_fill<R2, R3, NT>(tw2, g.tw2, t);
        static_for<0, C::RND1>([&](auto r_) { st.x[decltype(r_)::value] = mk(0.f, 0.f); });
        st.xoff = t * (int)sizeof(c32);
        load_x(t, st, kernel0, 0);
        // loaded once: inside the walk a global load in P5 would have to be waited for together
        // with the stores issued just before it (one in-order memory counter)
        static_for<0, C::RND1>([&](auto r_) {
            constexpr int r = decltype(r_)::value;
            const int u = t + NT * r;
            int rr, j;
            const bool slot = row_slot<RPW, C::NB1, NT, r>(u, rr, j);
            const int row = row0 + rr;
            const bool live = slot && row < rows;
            st.w1[r] = live ? g.tw1[j] : mk(1.f, 0.f);
            if constexpr (State::KEEP) {
                c32 p[R1];
                power_chain<R1>(st.w1[r], p);
                static_for<0, State::NEVEN>([&](auto k_) {
                    constexpr int k = decltype(k_)::value;
                    st.w1even[r * State::NEVEN + k] = p[2 * k + 2];
                });
            }
            const int yrow = live ? (tiled ? (g.y_row_of[row] << g.y_tile_shift) : row * g.y_pitch) : 0;
            auto col = [&](int w) { return tiled ? (w >> g.y_tile_shift) * g.y_tile_elems + (w & ((1 << g.y_tile_shift) - 1)) : w; };
            st.yoff[r] = live ? (int)((unsigned)(yrow + col(j)) * (unsigned)sizeof(c32)) : 0;
        });
        if constexpr (!MULTIF) {
            int rr, q;
            if (row_slot<RPW, C::NB3, NT, 0>(t, rr, q) && row0 + rr < rows) {
                const c32* srow = g.S + (size_t)(row0 + rr) * g.s_pitch;
                static_for<0, R3 / 2>([&](auto h_) {
                    constexpr int h = decltype(h_)::value;
                    c32x2 v = *reinterpret_cast<const c32x2*>(srow + (size_t)(h * C::NB3 + q) * 2);
                    st.s[2 * h] = v.a;
                    st.s[2 * h + 1] = v.b;
                });
            } else {
                static_for<0, R3>([&](auto a_) { st.s[decltype(a_)::value] = mk(0.f, 0.f); });
            }
        }
    });

    for (int m = 0; m < nk; m++) {
        const int kernel = kernel0 + m;
        FC_ROWS_STAMP(0);

        // P1: forward stage 1, pruned (one non-zero input per butterfly) -- as a phase of its own
        // only for the first map of the walk; for the others it is folded into the previous map's P5:
        // the thread that has just read the R1 LDS cells of butterfly j for the inverse
        // stage 1 is the only one that ever touches them, so it writes the next map's stage-1
        // outputs into them right away, with the twiddle chain it has at hand -- one phase and one
        // barrier fewer per map
        for (int f = 0; f < nF; f++) {
        if (m == 0 || f > 0) ctx.phase([&](int t, State& st) {
            static_for<0, C::RND1>([&](auto r_) {
                constexpr int r = decltype(r_)::value;
                int u = t + NT * r;
                if constexpr (MULTIF) FC_OPAQUE(u);
                int rr, j;
                // (F > 1, where this phase runs for every feature, keeps the general form of the slot: 1088 = 8.17.8 comes out with 109
                // instead of 95 registers, four waves per SIMD instead of five, with the short form in THIS phase -- and only in this one)
                if (row_slot<RPW, C::NB1, NT, r, MULTIF>(u, rr, j) && j < kw) {
                    c32* buf = lds + rr * LR;
                    c32 p[R1];
                    stage1_chain(r_, st, p);
                    fwd_stage1_out_pruned<R1, S1>(buf, j, st.x[r], p);
                }
            });
        });

        if constexpr (PRIO == 1) FC_ROWS_PRIO(1);
        // the next kernel row (next feature of this map, or the next map's first) flies during P2..P5
        if (f + 1 < nF) ctx.phase_nosync([&](int t, State& st) { load_x(t, st, kernel, f + 1); });
        else if (m + 1 < nk) ctx.phase_nosync([&](int t, State& st) { load_x(t, st, kernel + 1, 0); });

        FC_ROWS_STAMP(1);
        // P2: forward stage 2
        ctx.phase([&](int t, State&) {
            static_for<0, C::RND2>([&](auto r_) {
                constexpr int r = decltype(r_)::value;
                int u = t + NT * r;
                if constexpr (MULTIF) FC_OPAQUE(u);
                int rr, w;
                if (row_slot<RPW, C::NB2, NT, r>(u, rr, w)) {
                    const int c1 = w / R3, b = w - c1 * R3;
                    c32* p = lds + rr * LR + c1 * S1 + b;
                    c32 v[R2];
                    static_for<0, R2>([&](auto a_) {
                        constexpr int a = decltype(a_)::value;
                        if constexpr (a < NZ2) v[a] = (a * R3 + b < kw) ? p[a * R3] : mk(0.f, 0.f);
                        else v[a] = mk(0.f, 0.f);
                    });
                    fwd_stage2_out<R2, R3, NZ2>(p, v, Tw2Paired<R2>{tw2, b});   // inputs a >= NZ2 are structural zeros
                }
            });
        });

        FC_ROWS_STAMP(2);
        // P3: forward stage 3, product with the image spectrum (registers), inverse stage 3
        const bool last_f = (f == nF - 1);
        if constexpr (PRIO == 1) FC_ROWS_PRIO(0);
        ctx.phase([&](int t_, State& st) {
            int t = t_;
            if constexpr (MULTIF) FC_OPAQUE(t);
            int rr, q;
            if (row_slot<RPW, C::NB3, NT, 0>(t, rr, q)) {
                // MULTIF: this feature's image-spectrum row.  Only its first S_EARLY register pairs are requested
                // ahead of the forward butterfly, the rest right after it: with the whole row in flight beside the
                // radix-22 butterfly (its in-register composite form needs ~70 registers of its own) and the feature
                // sum, the kernel spilled 27-50 registers at L = 4224 (all 11 pairs early, rounds 1-2), differently in
                // every translation unit, and a scratch reload shares the in-order memory counter with these very loads
                // (59.7 -> 56.6 us per map at F = 4 with none early and no spills).  0 / 4 / 8 pairs early: no spills, and
                // 56.7 / 53.2 / 54.6 us per map at F = 4 on one box (profiles/r03i_f4_image_row_load_placement.txt).
                // Configurations with several rows per workgroup or a stage 3 above radix 22 keep more per-thread state:
                // nothing early there.
                constexpr int S_EARLY_PAIRS = 4;
                constexpr int S_EARLY = (RPW > 1 || R3 > 22) ? 0 : (S_EARLY_PAIRS < R3 / 2 ? S_EARLY_PAIRS : R3 / 2);
                if constexpr (MULTIF && 0 < S_EARLY) load_s(st, f, rr, q, IC<0>{}, IC<S_EARLY>{});
                c32* p = lds + rr * LR + (q / R2) * S1 + (q % R2) * R3;     // run c of stage-1 block c1: q = c1 * R2 + c
                c32 v[R3];
                run_load<R3>(p, v);
                if constexpr (MULTIF) {
                    // The R3 LDS cells this thread has just read are its own until the next barrier: the
                    // feature sum is parked there while the butterfly runs beside the in-flight image row
                    // (sum + image row + butterfly do not fit the register file together: 58-100 spilled
                    // registers otherwise) and comes back, pair by pair, into the accumulation.
                    if (f > 0) run_store<R3>(p, st.acc);
                    FC_SCHED_FENCE();
                }
                Dft<R3, -1>::run(v);
                if constexpr (MULTIF && S_EARLY < R3 / 2) load_s(st, f, rr, q, IC<S_EARLY>{}, IC<R3 / 2>{});
                if constexpr (FILTER) {
                    // one of three unrolled loops, picked by the launch's mode (uniform: a scalar branch around the loop, not in it)
                    const float fp = g.filter_param;
                    if (g.filter_mode == FC_FILTER_PHASE) {
                        static_for<0, R3>([&](auto a_) {
                            constexpr int a = decltype(a_)::value;
                            v[a] = spectral_filter_phase(v[a], st.s[a], fp);
                        });
                    } else if (g.filter_mode == FC_FILTER_WIENER) {
                        static_for<0, R3>([&](auto a_) {
                            constexpr int a = decltype(a_)::value;
                            v[a] = spectral_filter_wiener(v[a], st.s[a], fp);
                        });
                    } else {
                        static_for<0, R3>([&](auto a_) {
                            constexpr int a = decltype(a_)::value;
                            v[a] = cmul(v[a], st.s[a]);
                        });
                    }
                } else if constexpr (!MULTIF) {
                    static_for<0, R3>([&](auto a_) {
                        constexpr int a = decltype(a_)::value;
                        v[a] = cmul(v[a], st.s[a]);
                    });
                } else {
                    FC_SCHED_FENCE();
                    static_for<0, R3 / 2>([&](auto h_) {
                        constexpr int h = decltype(h_)::value;
                        c32 pa = cmul(v[2 * h], st.s[2 * h]);
                        c32 pb = cmul(v[2 * h + 1], st.s[2 * h + 1]);
                        if (f > 0) {
                            const c32x2 w = *reinterpret_cast<const c32x2*>(p + 2 * h);
                            pa = pa + w.a;
                            pb = pb + w.b;
                        }
                        st.acc[2 * h] = pa;
                        st.acc[2 * h + 1] = pb;
                        v[2 * h] = pa;
                        v[2 * h + 1] = pb;
                    });
                }
                if (!MULTIF || last_f) {
                    Dft<R3, +1>::run(v);
                    run_store<R3>(p, v);
                }
            }
        });
        }   // features

        FC_ROWS_STAMP(3);
        // P4: inverse stage 2
        if constexpr (PRIO == 1) FC_ROWS_PRIO(1);
        ctx.phase([&](int t, State&) {
            static_for<0, C::RND2>([&](auto r_) {
                constexpr int r = decltype(r_)::value;
                int u = t + NT * r;
                if constexpr (MULTIF) FC_OPAQUE(u);
                int rr, w;
                if (row_slot<RPW, C::NB2, NT, r>(u, rr, w)) {
                    const int c1 = w / R3, b = w - c1 * R3;
                    inv_stage2<R2, R3>(lds + rr * LR + c1 * S1 + b, Tw2Paired<R2>{tw2, b});
                }
            });
        });

        FC_ROWS_STAMP(4);
        // P5: inverse stage 1 straight to global memory; the barrier protects the LDS row
        // against the next map's P1
        c32* ybase = g.Y + (size_t)kernel * g.y_kernel_stride;
        ctx.phase([&](int t, State& st) {
            // the next kernel row (prefetched after P1) has had three phases to arrive: take it off
            // the memory counter before the store burst, or the next P1 would wait for these stores
            FC_WAIT_VMEM();
            // The R1 outputs of a butterfly are m1 columns apart, and m1 is a whole number of layout tiles or of HALF tiles (RowCfg
            // asserts it), so whether the intermediate is tiled or row-major, output a sits at base + a * stride: a scalar base per
            // output, the thread's 32-bit offset, no 64-bit tile arithmetic (once a fifth of this kernel's VALU instructions; a
            // cropped window adds a compare).
            // Where m1 is an odd number of HALF tiles (2112 = 8.12.22: 264 columns = 16.5 tiles; 288 = 4.6.12: 72) the even and the
            // odd outputs form two such chains, 2 * m1 columns apart each: two bases instead of one.
            char* yb = reinterpret_cast<char*>(ybase);
            constexpr bool TWO_CHAINS = (m1 % FC_Y_TILE_W) != 0;
            constexpr int SA = TWO_CHAINS ? 2 : 1;            // outputs a and a + SA are SA * m1 columns = whole tiles apart
            const unsigned stride_b = (unsigned)((tiled ? ((SA * m1) >> g.y_tile_shift) * g.y_tile_elems : SA * m1) * (int)sizeof(c32));
            // The store of output a: the uniform address yb + (a / SA) * stride_b, formed on the scalar unit, plus the thread's
            // 32-bit byte offset of its chain (State::yoff, summed once per walk) -- the scalar-base + vector-offset form of the
            // store, no vector add per store.  (stride_b is a launch argument: it cannot be the store's immediate, and at cfg3's
            // tile stride it would not fit one.)  A cropped window compares the thread's column against wout - a * m1.
            static_for<0, C::RND1>([&](auto r_) {
                constexpr int r = decltype(r_)::value;
                int u = t + NT * r;
                FC_OPAQUE(u);   // the twiddle chain is recomputed per map, not kept (spilled) across the loop
                int rr, j;
                if (row_slot<RPW, C::NB1, NT, r>(u, rr, j) && row0 + rr < rows) {
                    const c32* buf = lds + rr * LR;
                    c32 p[R1];
                    c32 v[R1];
                    if constexpr (FC_ROWSM_DBG & 1) {
                        static_for<0, R1>([&](auto c_) { v[decltype(c_)::value] = st.s[decltype(c_)::value]; });
                        if (m + 1 < nk && j < kw) stage1_chain(r_, st, p);
                    } else {
                    stage1_chain(r_, st, p);
                    inv_stage1_in<R1, S1>(buf, j, p, v);
                    }
                    // (FC_OPAQUE on the offset, in place and free: its zero-extension stays beside the store instead of being
                    // hoisted out of the walk as a 64-bit pair, which the store could only take through a 64-bit vector add)
                    // TWO_CHAINS: the odd chain starts m1 = k tiles + h columns further on -- the same tile row k (+ 1 where the
                    // column wraps into the next tile) and h columns on (or TL - h back): one of two uniform distances
                    int yoff1 = 0;
                    if constexpr (TWO_CHAINS) {
                        const int TL = 1 << g.y_tile_shift, h = m1 & (TL - 1), k = m1 >> g.y_tile_shift;
                        const int near = tiled ? k * g.y_tile_elems + h : m1, far = tiled ? (k + 1) * g.y_tile_elems + h - TL : m1;
                        yoff1 = st.yoff[r] + (((j & (TL - 1)) + h >= TL) ? far : near) * (int)sizeof(c32);
                    }
                    auto store = [&](auto a_) {
                        constexpr int a = decltype(a_)::value;
                        int& base = (TWO_CHAINS && (a & 1)) ? yoff1 : st.yoff[r];
                        FC_OPAQUE(base);
                        FC_ROWSM_STORE(reinterpret_cast<c32*>(yb + (size_t)((unsigned)(a / SA) * stride_b) + (size_t)(unsigned)base), v[a]);
                    };
                    if (g.wout >= L) {   // nothing cropped (uniform)
                        static_for<0, R1>(store);
                    } else {             // cropped window (cfg4: 4160 columns of the 4224 transform)
                        static_for<0, R1>([&](auto a_) {
                            if (j < g.wout - decltype(a_)::value * m1) store(a_);
                        });
                    }
                    if (m + 1 < nk && j < kw)     // forward stage 1 of the next map into the cells just read
                        fwd_stage1_out_pruned<R1, S1>(lds + rr * LR, j, st.x[r], p);
                }
                FC_SCHED_FENCE();
            });
        });
        FC_ROWS_STAMP(5);
    }
}

}  // namespace fc
