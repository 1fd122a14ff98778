// fc_instrument.hpp -- the ablation and timeline switches of the kernels, in ONE place.
//
// Only ablations and timelines of the CURRENT kernels live here: they measure the product as built (DESIGN.md's account
// of where the time goes rests on them).  An alternative design is measured on a branch, and the losing side of that A/B
// does not stay in the tree.
//
// The product build (csrc/Makefile) never defines FC_INSTRUMENT: all switches below are then fixed at their
// product values and any attempt to set one from the command line is a compile error.  Diagnostic builds
// (tools/build_variant.sh, tools/microbench/*) pass -DFC_INSTRUMENT plus the switches they want; the ablations
// produce WRONG RESULTS by design (they remove loads, stores, barriers or arithmetic to time what is left).
#pragma once

#if !defined(FC_INSTRUMENT)
#if defined(FC_COLS_DBG) || defined(FC_ROWSM_DBG) || defined(FC_COLS_TIMELINE) || defined(FC_ROWS_TIMELINE)
#error "kernel instrumentation switches need -DFC_INSTRUMENT (diagnostic builds only; the product never sets them)"
#endif
#endif

// ---- output-column kernel (fast_cols.hpp)
#ifndef FC_COLS_DBG
#define FC_COLS_DBG 0            // wrong results: 1 skip pair pass, 2 no barriers between stages, 4 no gather loads, 8 no stores
#endif
#ifndef FC_COLS_TIMELINE
#define FC_COLS_TIMELINE 0       // 1: one workgroup stamps the 100 MHz wall clock at every phase boundary (tools/cols_timeline.py)
#endif
#ifndef FC_COLS_TIMELINE_BASE
#define FC_COLS_TIMELINE_BASE 0  // first stamped tile of that workgroup (16 tiles are stamped)
#endif
#ifndef FC_COLS_TIMELINE_WG
#define FC_COLS_TIMELINE_WG 0
#endif

// ---- spectral-row kernels (fast_rows.hpp, fast_rows_multi.hpp)
#ifndef FC_ROWSM_DBG
#define FC_ROWSM_DBG 0           // multi-map kernel, wrong results: 1 P5 without its LDS reads and stage-1 arithmetic, 2 no stores
#endif
#ifndef FC_ROWS_TIMELINE
#define FC_ROWS_TIMELINE 0       // 1: one workgroup stamps the wall clock at every phase boundary (tools/rows_timeline.py)
#endif
#ifndef FC_ROWS_TIMELINE_WG
#define FC_ROWS_TIMELINE_WG 1000
#endif

// ---- stamps (expand to nothing in the product)
#if FC_COLS_TIMELINE && defined(__HIP_DEVICE_COMPILE__)
#define FC_COLS_STAMP(slot) do { if (wg == FC_COLS_TIMELINE_WG && threadIdx.x == 0 && g.timeline && it >= FC_COLS_TIMELINE_BASE && it < FC_COLS_TIMELINE_BASE + 16) g.timeline[(it - FC_COLS_TIMELINE_BASE) * 8 + (slot)] = wall_clock64(); } while (0)
#else
#define FC_COLS_STAMP(slot) ((void)0)
#endif
#if FC_ROWS_TIMELINE && defined(__HIP_DEVICE_COMPILE__)
// (slot 0 of a map also leaves the shader-cycle counter in slot 6: delta s_memtime / delta wall clock x 100 MHz = the clock the workgroup ran at)
#define FC_ROWS_STAMP(slot) do { if (group == FC_ROWS_TIMELINE_WG && kernel0 == 0 && threadIdx.x == 0 && g.timeline && m < 16) { g.timeline[m * 8 + (slot)] = wall_clock64(); if ((slot) == 0) g.timeline[m * 8 + 6] = __builtin_amdgcn_s_memtime(); } } while (0)
#else
#define FC_ROWS_STAMP(slot) ((void)0)
#endif

// store of the multi-map row kernel: the "no stores" ablation keeps the address arithmetic and a never-true guard
#if (FC_ROWSM_DBG & 2)
#define FC_ROWSM_STORE(ptr, val) do { const ::fc::c32 fc_w_ = (val); if (fc_w_.x == 1.2345e-30f) *(ptr) = fc_w_; } while (0)
#else
#define FC_ROWSM_STORE(ptr, val) FC_STREAM_STORE(ptr, val)
#endif
