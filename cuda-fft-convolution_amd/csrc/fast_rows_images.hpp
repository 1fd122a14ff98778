// fast_rows_images.hpp -- spectral-row kernel that walks over IMAGES (plan option "image_walk" 1, image batches, F = 1).
//
// fast_rows_multi_body keeps an image-spectrum row in registers and walks over kernels: every map pays the whole forward
// transform of its kernel row (pruned stage 1, stage 2 with its barrier and LDS round trip, the forward stage-3 butterfly).
// A batch of many images against few kernels has short kernel walks (one map at N = 1) and pays that transform of the SAME
// kernel row once per image.  Here the roles are swapped: a workgroup of (row group, kernel) transforms its kernel row once,
// keeps the result IN REGISTERS in stage-3 order -- kf[a] of butterfly q, the very values the product with the image spectrum
// takes -- and walks over the images of the launch.  Per map what is left is
//   P3'  one load of the image-spectrum row (register order, 16 B per lane; requested a map ahead), R3 complex products,
//        inverse stage 3, the run back into LDS;
//   P4   inverse stage 2;
//   P5   inverse stage 1 straight to the intermediate;
// three phases instead of four and no forward arithmetic after the first map.  The price: the image-spectrum row (8 * C bytes)
// is read once per MAP -- the kernel walk reads it once per walk -- by kernels_per_image workgroups side by side on one L2
// (fast_paths.hpp: rows_walk_images).
//
// After the once-per-walk part a map's arithmetic does not depend on its place in the walk: the maps of (image, kernel) are
// the same bits whatever the walk length and whatever the batch.  They are NOT the bits of the kernel walk: the forward
// stage 2 runs unpruned here (one instantiation per length; it runs once per walk), a different summation order.
//
// P4 and P5 are the phases of fast_rows_multi_body (same helpers, same store form); P5 does not fold in a next map's forward
// stage 1 -- there is none -- and ends with a barrier because the next map's P3' overwrites the LDS rows.  The even powers of
// the stage-1 twiddle are not kept (RowMultiState::KEEP): P4 and P5 already hold kf beside their own state.
#pragma once
#include "fast_rows.hpp"

namespace fc {

template <class C>
struct RowImagesState {
    c32 kf[C::R3];       // transformed kernel row of this thread's stage-3 butterfly: the whole walk
    c32 s[C::R3];        // image spectrum of the same butterfly: the current map's, then the next one's in flight
    c32 x[C::RND1];      // kernel row (until forward stage 1 has consumed it)
    c32 w1[C::RND1];     // stage-1 base twiddle w_L^j of this thread's butterflies (same for every map)
    int yoff[C::RND1];   // byte offset of output 0 of round r's butterfly within a map (same for every map)
    int soff;            // byte offset of this thread's first register pair within an image's spectrum; < 0: no row to read
};

// Maps (image0 + m, kernel), m < ni, of row group `group`.  g.S / g.Y: image 0 and slot 0 of the LAUNCH (the body resolves the
// image itself: S + b * s_image_stride, slot b * kernels_per_image + kernel).
template <class C, class Ctx>
FC_HD void fast_rows_images_body(Ctx& ctx, c32* lds, const FastRowsArgs& g, int group, int kernel, int image0, int ni, int rows) {
    constexpr int L = C::L, R1 = C::R1, R2 = C::R2, R3 = C::R3, NT = C::NT, m1 = C::m1, RPW = C::RPW, S1 = C::S1, LR = C::LR;
    using State = RowImagesState<C>;
    c32* tw2 = lds + RPW * LR;
    const int kw = g.kw;
    const int row0 = group * RPW;
    const bool tiled = g.y_row_of != nullptr;

    // the image-spectrum row of image b for this thread's stage-3 butterfly: the uniform address of the image's register pair h,
    // formed on the scalar unit, plus the thread's 32-bit byte offset (State::soff; FC_OPAQUE keeps its zero-extension beside
    // the load) -- R3 / 2 per-lane 64-bit addresses held across the walk otherwise.  Threads without a row to read (soff < 0)
    // keep the zeros of the start.
    auto load_s = [&](State& st, int b) {
        if (st.soff < 0) return;
        const char* sb = reinterpret_cast<const char*>(g.S + (size_t)b * g.s_image_stride);
        static_for<0, R3 / 2>([&](auto h_) {
            constexpr int h = decltype(h_)::value;
            FC_OPAQUE(st.soff);
            c32x2 w = *reinterpret_cast<const c32x2*>(sb + (size_t)(h * C::NB3 * 2) * sizeof(c32) + (size_t)(unsigned)st.soff);
            st.s[2 * h] = w.a;
            st.s[2 * h + 1] = w.b;
        });
    };

    // once per workgroup: stage-2 twiddles into LDS, the kernel row, the per-thread constants of P5
    ctx.phase_nosync([&](int t, State& st) {
        fc_tw2_fill<R2, R3, NT>(tw2, g.tw2, t);
        {
            int rr, q;
            const bool reads = row_slot<RPW, C::NB3, NT, 0>(t, rr, q) && row0 + rr < rows;
            st.soff = reads ? (int)(((unsigned)(row0 + rr) * (unsigned)g.s_pitch + 2u * (unsigned)q) * (unsigned)sizeof(c32)) : -1;
            static_for<0, R3>([&](auto a_) { st.s[decltype(a_)::value] = mk(0.f, 0.f); });
        }
        const c32* abase = g.A + (size_t)kernel * g.a_kernel_stride;
        static_for<0, C::RND1>([&](auto r_) {
            constexpr int r = decltype(r_)::value;
            const int u = t + NT * r;
            int rr, j;
            const bool slot = row_slot<RPW, C::NB1, NT, r>(u, rr, j);
            const int row = row0 + rr;
            const bool live = slot && row < rows;
            st.x[r] = (live && j < kw) ? abase[(size_t)row * g.a_pitch + j] : mk(0.f, 0.f);
            st.w1[r] = live ? g.tw1[j] : mk(1.f, 0.f);
            const int yrow = live ? (tiled ? (g.y_row_of[row] << g.y_tile_shift) : row * g.y_pitch) : 0;
            auto col = [&](int w) { return tiled ? (w >> g.y_tile_shift) * g.y_tile_elems + (w & ((1 << g.y_tile_shift) - 1)) : w; };
            st.yoff[r] = live ? (int)((unsigned)(yrow + col(j)) * (unsigned)sizeof(c32)) : 0;
        });
    });

    // forward stage 1, pruned (one non-zero input per butterfly)
    ctx.phase([&](int t, State& st) {
        static_for<0, C::RND1>([&](auto r_) {
            constexpr int r = decltype(r_)::value;
            const int u = t + NT * r;
            int rr, j;
            if (row_slot<RPW, C::NB1, NT, r>(u, rr, j) && j < kw) {
                c32 p[R1];
                power_chain<R1>(st.w1[r], p);
                fwd_stage1_out_pruned<R1, S1>(lds + rr * LR, j, st.x[r], p);
            }
        });
    });

    // forward stage 2, unpruned: every input enters (the cells past the kernel row were never written and count as zeros)
    ctx.phase([&](int t, State&) {
        static_for<0, C::RND2>([&](auto r_) {
            constexpr int r = decltype(r_)::value;
            const int u = t + NT * r;
            int rr, w;
            if (row_slot<RPW, C::NB2, NT, r>(u, rr, w)) {
                const int c1 = w / R3, b = w - c1 * R3;
                c32* p = lds + rr * LR + c1 * S1 + b;
                c32 v[R2];
                static_for<0, R2>([&](auto a_) {
                    constexpr int a = decltype(a_)::value;
                    v[a] = (a * R3 + b < kw) ? p[a * R3] : mk(0.f, 0.f);
                });
                fwd_stage2_out<R2, R3, R2>(p, v, Tw2Paired<R2>{tw2, b});
            }
        });
    });

    // forward stage 3 into registers (the thread's own run: no barrier before P3' writes it), and the first image's row
    ctx.phase_nosync([&](int t, State& st) {
        int rr, q;
        if (row_slot<RPW, C::NB3, NT, 0>(t, rr, q)) {
            const c32* p = lds + rr * LR + (q / R2) * S1 + (q % R2) * R3;
            run_load<R3>(p, st.kf);
            Dft<R3, -1>::run(st.kf);
        }
        // (the row is requested AFTER the butterfly: in flight beside it, kf + the butterfly's temporaries + the row do not fit
        //  the register file -- fast_rows_multi.hpp, S_EARLY)
        FC_SCHED_FENCE();
        load_s(st, image0);
    });

    for (int m = 0; m < ni; m++) {
        const int b = image0 + m;

        // P3': product with the image spectrum, inverse stage 3; then the next image's row flies during P4 and P5
        ctx.phase([&](int t, State& st) {
            int rr, q;
            if (row_slot<RPW, C::NB3, NT, 0>(t, rr, q)) {
                c32* p = lds + rr * LR + (q / R2) * S1 + (q % R2) * R3;
                c32 v[R3];
                static_for<0, R3>([&](auto a_) {
                    constexpr int a = decltype(a_)::value;
                    v[a] = cmul(st.kf[a], st.s[a]);
                });
                Dft<R3, +1>::run(v);
                run_store<R3>(p, v);
            }
            FC_SCHED_FENCE();      // (as above: not beside the butterfly)
            if (m + 1 < ni) load_s(st, b + 1);
        });

        // P4: inverse stage 2
        ctx.phase([&](int t, State&) {
            static_for<0, C::RND2>([&](auto r_) {
                constexpr int r = decltype(r_)::value;
                const int u = t + NT * r;
                int rr, w;
                if (row_slot<RPW, C::NB2, NT, r>(u, rr, w)) {
                    const int c1 = w / R3, bb = w - c1 * R3;
                    inv_stage2<R2, R3>(lds + rr * LR + c1 * S1 + bb, Tw2Paired<R2>{tw2, bb});
                }
            });
        });

        // P5: inverse stage 1 straight to global memory (fast_rows_multi.hpp, P5: one or two chains of equal strides, a scalar
        // base per output plus the thread's 32-bit offset); the barrier protects the LDS rows against the next map's P3'
        c32* ybase = g.Y + (size_t)(b * g.kernels_per_image + kernel) * g.y_kernel_stride;
        ctx.phase([&](int t, State& st) {
            // the next image's row (requested in P3') has had a phase to arrive: off the memory counter before the store burst,
            // or the next P3' would wait for these stores
            FC_WAIT_VMEM();
            char* yb = reinterpret_cast<char*>(ybase);
            constexpr bool TWO_CHAINS = (m1 % FC_Y_TILE_W) != 0;
            constexpr int SA = TWO_CHAINS ? 2 : 1;
            const unsigned stride_b = (unsigned)((tiled ? ((SA * m1) >> g.y_tile_shift) * g.y_tile_elems : SA * m1) * (int)sizeof(c32));
            static_for<0, C::RND1>([&](auto r_) {
                constexpr int r = decltype(r_)::value;
                int u = t + NT * r;
                FC_OPAQUE(u);   // the twiddle chain is recomputed per map, not kept (spilled) across the loop
                int rr, j;
                if (row_slot<RPW, C::NB1, NT, r>(u, rr, j) && row0 + rr < rows) {
                    c32 p[R1];
                    c32 v[R1];
                    // (the base twiddle made opaque: its power chain is formed here, per map, not hoisted out of the walk and held
                    //  -- R1 - 2 values per round -- beside kf and the row in flight)
                    c32 w1 = st.w1[r];
                    FC_OPAQUE(w1.x);
                    FC_OPAQUE(w1.y);
                    power_chain<R1>(w1, p);
                    inv_stage1_in<R1, S1>(lds + rr * LR, j, p, v);
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
                    } else {             // cropped window
                        static_for<0, R1>([&](auto a_) {
                            if (j < g.wout - decltype(a_)::value * m1) store(a_);
                        });
                    }
                }
                FC_SCHED_FENCE();
            });
        });
    }
}

}  // namespace fc
