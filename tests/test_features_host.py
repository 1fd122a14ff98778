"""CPU tier of test_features_gpu.py: its generated case list reaches every F > 1 row-kernel instantiation of fast_paths.hpp.

A new row-table entry fails here until test_features_gpu.ROW_CASES has a case that launches it at F > 1."""
import ctypes

import pytest

import test_features_gpu as tf
import util


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(util.build_emu())
    yield lib
    lib.emu_set_exact_window(0)


def test_parsed_table_is_the_compiled_table(emu):
    """the (L, NZ2) the cases are generated from are exactly the configurations the kernels are instantiated for (the
    FC_FAST_ROW_CONFIGS list as g++ sees it), in the same order: no row of the table escapes the parse"""
    n = emu.emu_row_configs(None, None, 0)
    Ls, nz2 = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    assert emu.emu_row_configs(Ls, nz2, n) == n
    parsed = [(L, e[5]) for L, entries in tf.ROW_TABLE.items() for e in entries]
    assert parsed == list(zip(Ls, nz2))
    assert sorted(parsed) == tf.row_instantiations()


def test_feature_row_cases_cover_every_instantiation():
    """every (L, NZ2) of the table is launched at F > 1 by some case: a width whose dispatched entry is that NZ2"""
    covered = {(L, tf.dispatched_nz2(L, kw)) for L, F, walk, widths in tf.ROW_CASES if F > 1 for kw in widths}
    missing = sorted(set(tf.row_instantiations()) - covered)
    assert not missing, "no F > 1 GPU case launches (L, NZ2) %s" % missing


def test_feature_row_cases_reach_the_grid_decode_and_partial_walks():
    """each case: more than 8 row groups and not a multiple of 8 (the decode's gl >= 1 and its group >= groups exit), the last
    walk of every launch partial, the kernels within what the plan's row kernel accepts"""
    rows = tf.H_WINDOW // 2 + 1
    for L, F, walk, widths in tf.ROW_CASES:
        R1, R2, R3, NT, RPW, NZ2 = tf.ROW_TABLE[L][0]
        groups = -(-rows // RPW)
        assert groups > 8 and groups % 8, (L, RPW, groups)
        assert walk > 1 and tf.KERNELS_PER_WIDTH % walk, (L, walk)
        assert max(widths) <= L // R1, L
        assert len(set(widths)) == len(widths) == len(tf.ROW_TABLE[L])


def test_dispatch_rule_matches_the_table():
    """the first entry with NZ2 >= ceil(kw / R3): one width just above an entry's reach goes to the next entry"""
    for L, entries in tf.ROW_TABLE.items():
        R3 = entries[0][2]
        assert [e[2] for e in entries] == [R3] * len(entries) and [e[5] for e in entries] == sorted({e[5] for e in entries})
        for lo, hi in zip(entries, entries[1:]):
            assert tf.dispatched_nz2(L, lo[5] * R3) == lo[5] and tf.dispatched_nz2(L, lo[5] * R3 + 1) == hi[5]
        assert tf.dispatched_nz2(L, 1) == entries[0][5]


def test_diagnostic_shift_add_reference():
    """the diagnostic's reference (a float64 shift-and-add, no transform) against numpy's float64 FFT convolution"""
    import numpy as np
    F = 8
    data = np.random.default_rng(1).standard_normal((20, 30, F)).astype(np.float32)
    for what, k in tf.diagnostic_kernels(F):
        want = util.numpy_fft_conv(data, tf.DIAG_K, tf.DIAG_K, [k])[0]
        got = tf.shift_add(data, k, *want.shape)
        assert np.abs(got - want).max() < 1e-9 * max(1.0, np.abs(want).max()), what


def test_numpy_reference_matches_util():
    """test_features_gpu.numpy_reference (feature sum in the spectrum) against util.numpy_fft_conv (sum of the maps)"""
    import numpy as np
    rng = np.random.default_rng(2)
    data = rng.standard_normal((30, 41, 5)).astype(np.float32)
    ks = [rng.standard_normal((7, 9, 5)).astype(np.float32), rng.standard_normal((3, 4, 5)).astype(np.float32)]
    for got, want in zip(tf.numpy_reference(data, 7, 9, ks), util.numpy_fft_conv(data, 7, 9, ks)):
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-10 * np.abs(want).max()


def test_plan_form_cases_take_the_named_path(emu):
    """the planner (the product's make_geometry, through the emulator) puts test_features_gpu's plan-form cases where their
    ids say: 16 x 8368 at F = 16 is a Bluestein row summing its features in the intermediate (acc_in_y); 12 x 10500 with 3 x 5
    kernels has a single-pass plan (10648 points) at F = 1 and none at F = 4, where the accumulator no longer fits the LDS"""
    H, W, F, kh, kw = tf.BLUESTEIN_ACC_SHAPE
    emu.emu_set_exact_window(1)
    try:
        assert emu.emu_plan_rows_form(H, W, F, kh, kw) == 3
        assert emu.emu_plan_rows_form(H, W, 1, kh, kw) == 1          # (F = 1: no feature sum)
    finally:
        emu.emu_set_exact_window(0)
    H, W, kh, kw = tf.SINGLE_PASS_SHAPE
    lh, lw = ctypes.c_int(0), ctypes.c_int(0)
    assert emu.emu_plan_lengths(H, W, 1, kh, kw, ctypes.byref(lh), ctypes.byref(lw)) == 0 and lw.value == 10648
    assert emu.emu_plan_rows_form(H, W, 1, kh, kw) == 0
    assert emu.emu_plan_rows_form(H, W, 4, kh, kw) == -1
    # the chunked batching case: a 384 x 480 plan (193 spectrum rows), 593 KB of column spectra per kernel
    assert emu.emu_plan_lengths(300, 400, 16, 21, 21, ctypes.byref(lh), ctypes.byref(lw)) == 0 and (lh.value, lw.value) == (384, 480)
