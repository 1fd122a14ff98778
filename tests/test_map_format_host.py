"""16-bit result maps (plan option "map_format": 1 = IEEE fp16, 2 = bfloat16) on the CPU tier.

The output kernels convert each fp32 value once, in the store: round to nearest even, subnormal results kept, fp16 overflow
to +-inf.  Checked here without a GPU:
  * the kernel bodies: tests/map_format_host/map_format_host.cpp, a stand-alone host program over the product's kernel headers
    (built here with the host compiler), runs fast_cols_body and cols_c2r_body in fp32 and in both 16-bit formats on the same
    intermediate; the 16-bit maps must be the fp32 maps converted by a routine of its own, bit for bit;
  * the conversion helpers of csrc/fc_common.hpp (the host side: integer arithmetic) and that routine against NumPy;
  * the build's resource reports: the new kernels spill where their fp32 siblings are documented to, and nowhere else;
  * the option: its validation, the versioned field of fftconv_plan_options, what can be refused without a device."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import util

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "map_format_host")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_format_host") / "map_format_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(util.ROOT, "tests", "emu"),
                    os.path.join(HOST_DIR, "map_format_host.cpp"), "-o", exe], check=True)
    return exe


def test_kernel_bodies_store_the_rounded_fp32_value(host_program):
    """fast_cols_body<..., OUT16> for T = 16, 8 and 4, tiled and row-major, a sliced tail round and the dynamic tile queue, and the
    generic cols_c2r_body (direct and Bluestein): every element of the fp16 / bf16 maps equals the fp32 map's element rounded to
    nearest even by the program's own floating-point routine.  The inputs sweep 2^-30 .. 2^20 over the columns, so subnormal
    halves, zeros and overflows to inf are all in the maps."""
    r = subprocess.run([host_program, "bodies"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    ok = [line for line in r.stdout.splitlines() if line.startswith("ok ")]
    assert len(ok) == 20 and "all bit-equal" in r.stdout           # 8 specialised launches + 2 generic, two formats each
    for what in ("T=16 tiled f", "T=16 row-major", "sliced tail round", "T=8 tiled", "T=8 row-major", "T=4 tiled f", "T=4 row-major",
                 "dynamic tile queue", "generic f", "Bluestein"):
        assert sum(what in line for line in ok) == 2, what


def conversion_inputs():
    """float32 values around everything the conversions decide: ties (exactly between two neighbours, with an even and with an
    odd neighbour below), the floats just above and below each tie, subnormal results down to the smallest and the ties around
    it, the largest finite value and the first that rounds to inf, +-0, a few ordinary values and a random sweep of exponents"""
    v = []

    def around(x):
        x = np.float32(x)
        v.extend([np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))])

    for mant_bits, e_min, e_max in ((10, -14, 15), (7, -126, 127)):
        ulp = lambda e: 2.0 ** (e - mant_bits)
        for e in (e_min, e_min + 1, -3, 0, 1, 7, e_max - 1, e_max):
            for k in (0, 1, 2, 3, 2 ** mant_bits - 2, 2 ** mant_bits - 1):
                x = (2 ** mant_bits + k) * ulp(e)             # a representable value ...
                around(x)
                if e < 127 or k < 2 ** mant_bits - 1:
                    around(x + 0.5 * ulp(e))                  # ... and the tie above it (k even: down, k odd: up)
        sub = 2.0 ** (e_min - mant_bits)                      # the subnormal grid
        for k in (0, 1, 2, 3, 4, 5, 2 ** mant_bits - 2, 2 ** mant_bits - 1, 2 ** mant_bits):
            around(k * sub)
            around((k + 0.5) * sub)
        around(0.25 * sub)
        around(0.75 * sub)
        top = (2 ** (mant_bits + 1) - 1) * ulp(e_max)         # largest finite; the tie above it rounds to inf
        around(top)
        if e_max < 127:
            around(top + 0.5 * ulp(e_max))
            around(2.0 ** (e_max + 1))
            around(1e6)
    v.extend(np.float32(x) for x in (0.0, 1.0, 1.5, 1.0 / 3.0, 3.1415927, 65504.0, 65519.996, 65520.0, 1e-8, 6e-8, 3.3e38,
                                     np.float32(np.inf), np.finfo(np.float32).tiny, np.finfo(np.float32).max, 1e-45, 1e-40))
    rng = np.random.default_rng(5)
    v.extend((rng.standard_normal(4096) * 2.0 ** rng.integers(-30, 20, 4096)).astype(np.float32))
    a = np.array(v, dtype=np.float32)
    a = a[np.isfinite(a) | np.isinf(a)]
    return np.concatenate([a, -a])


def numpy_bf16(x):
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def test_conversion_helpers_match_numpy(host_program, tmp_path):
    """fc_map16 and both halves of fc_pack_map16 (csrc/fc_common.hpp, host side): fp16 against astype(np.float16), bf16 against
    ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) on the uint32 view; the host program's own reference routine against the same"""
    x = conversion_inputs()
    assert x.size > 9000 and (x == 0).sum() >= 2 and np.signbit(x[x == 0]).any()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    x.tofile(fin)
    subprocess.run([host_program, "convert", fin, fout], check=True)
    got = np.fromfile(fout, dtype=np.uint16).reshape(-1, 8)
    assert got.shape[0] == x.size
    with np.errstate(over="ignore"):
        want16 = x.astype(np.float16).view(np.uint16)
        want16_neg = (-x).astype(np.float16).view(np.uint16)
    wantbf, wantbf_neg = numpy_bf16(x), numpy_bf16(-x)
    # the set really holds what it claims: results that are subnormal, that overflow, and ties (fp32 values exactly between two halves)
    h = want16 & 0x7FFF
    assert ((h > 0) & (h < 0x400)).sum() > 50 and (h == 0x7C00).sum() > 10 and (h == 0x7BFF).sum() >= 2 and (h == 0).sum() > 10
    assert ((x.view(np.uint32) & 0x1FFF) == 0x1000).sum() > 50 and ((x.view(np.uint32) & 0xFFFF) == 0x8000).sum() > 50
    names = ("fc_map16 fp16", "fc_map16 bf16", "fc_pack_map16 fp16 low", "fc_pack_map16 fp16 high", "fc_pack_map16 bf16 low",
             "fc_pack_map16 bf16 high", "reference fp16", "reference bf16")
    wants = (want16, wantbf, want16, want16_neg, wantbf, wantbf_neg, want16, wantbf)
    for col, (name, want) in enumerate(zip(names, wants)):
        bad = np.flatnonzero(got[:, col] != want)
        assert bad.size == 0, (name, [(float(x[i]), hex(got[i, col]), hex(want[i])) for i in bad[:5]])


def _resource_reports():
    """{kernel symbol: {vgpr, spill, scratch, occ}} from the build's csrc/*.rpt (as tests/test_host_logic.py reads them)"""
    subprocess.run(["make", "-C", CSRC], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = {}
    for path in glob.glob(os.path.join(CSRC, "*.rpt")):
        cur = None
        for line in open(path):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, line)
                if m and cur is not None:
                    cur[key] = int(m.group(1))
    return out


def test_map16_kernels_do_not_spill():
    """The 16-bit output kernels (k_fast_cols16: one instantiation per fp32 one, the fp16 / bf16 choice a uniform run-time value;
    k_cols_c2r16; the crop / pad kernels) in the build's own report: no spilled register, no scratch, 3 waves per SIMD -- except
    where the fp32 kernel of the same configuration is documented to spill (tests/test_host_logic.py:
    test_hot_kernels_do_not_spill: M = 2080, and the row-major variant of M = 3072 / 2560), and there never more than it does."""
    rep = _resource_reports()
    if not rep:
        pytest.skip("no csrc/*.rpt resource reports beside the objects (a library built without csrc/Makefile)")
    hot32 = {k: v for k, v in rep.items() if "k_fast_colsI" in k}
    hot16 = {k: v for k, v in rep.items() if "k_fast_cols16I" in k}
    assert len(hot32) > 40 and len(hot16) == len(hot32), (len(hot16), len(hot32))
    for k, v in hot16.items():
        sib = hot32[k.replace("13k_fast_cols16I", "11k_fast_colsI")]          # (the length prefix of the mangled name)
        assert v["occ"] >= 3 and v["spill"] <= sib["spill"] and v["scratch"] <= sib["scratch"], (k, v, sib)
    bad = {k: v for k, v in hot16.items() if v["spill"] or v["scratch"]}
    known = {k: v for k, v in bad.items() if ("k_fast_cols16INS_6ColCfgILi2080E" in k and v["spill"] <= (12 if "ELb0ELb0EEEv" in k else 5)) or
             (("k_fast_cols16INS_6ColCfgILi3072E" in k or "k_fast_cols16INS_6ColCfgILi2560E" in k) and "ELb0ELb0ELb0EEEv" in k and v["spill"] <= 6)}
    assert not {k: v for k, v in bad.items() if k not in known}, bad
    # the configurations the benchmark's main shapes run (cfg3: M = 2112, cfg2: 576, cfg1: 144) are spill-free in every variant
    for m in (2112, 576, 144):
        mine = {k: v for k, v in hot16.items() if "ColCfgILi%dE" % m in k}
        assert len(mine) >= 3 and not any(v["spill"] or v["scratch"] for v in mine.values()), mine
    small = {k: v for k, v in rep.items() if any(s in k for s in ("k_cols_c2r16I", "k_crop_maps16", "k_pad_maps16"))}
    assert len(small) == 4, sorted(small)
    assert not {k: v for k, v in small.items() if v["spill"] or v["scratch"]}, small


def test_map_format_validation(host_program):
    """pipeline.hpp: map_format_error, the one place that says which values the option takes -- the library's set_option and
    plan creation both ask it: 0 / 1 / 2, and nothing but 0 on a block-wise plan, with a message that says why"""
    out = subprocess.run([host_program, "options"], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    res = {(int(l.split()[0]), int(l.split()[1])): l.split(None, 2)[2] for l in out if not l.startswith("bytes")}
    assert [res[(v, 0)] == "ok" for v in (-1, 0, 1, 2, 3)] == [False, True, True, True, False]
    assert [res[(v, 1)] == "ok" for v in (-1, 0, 1, 2, 3)] == [False, True, False, False, False]
    for v in (1, 2):
        assert "block-wise" in res[(v, 1)] and "fp32" in res[(v, 1)]
    assert out[-1] == "bytes 4 2 2"


def test_plan_options_field_and_what_needs_no_device(fftconv):
    """fftconv_plan_options.map_format is appended behind `verbose` and versioned by struct_size.  Without a device a plan
    cannot exist, but plan creation checks the new field before it looks for one: a value out of range, and a 16-bit format on
    sizes the planner takes block-wise, are argument errors (-1) with the reason; everything else about the field gets as far as
    the device check (FFTCONV_ERR_NO_DEVICE = -6 here, success on a GPU box), including a struct_size that ends before the field
    whatever bytes follow it."""
    lib = fftconv.load_library()
    o = fftconv.PlanOptions(map_format=2)
    assert ctypes.sizeof(fftconv.PlanOptions) == 40 and fftconv.PlanOptions.map_format.offset == 32
    assert o.struct_size == 40 and o.map_format == 2 and o.verbose == 0
    assert fftconv.PlanOptions().map_format == 0
    assert fftconv.MAP_DTYPES == {0: np.dtype(np.float32), 1: np.dtype(np.float16), 2: np.dtype(np.uint16)}
    # the header agrees about the layout
    hdr = open(os.path.join(util.ROOT, "include", "fftconv.h")).read()
    fields = re.findall(r"^\s+(?:size_t|int)\s+(\w+);", hdr[hdr.index("typedef struct fftconv_plan_options {"):hdr.index("} fftconv_plan_options;")], re.M)
    assert fields == [n for n, _ in fftconv.PlanOptions._fields_]
    have_gpu = fftconv.device_count() > 0

    def create(H, W, kh, kw, opts):
        h = ctypes.c_void_p(None)
        rc = lib.fftconv_plan_create_ex(ctypes.byref(h), H, W, 1, kh, kw, 0, None, ctypes.byref(opts))
        msg = lib.fftconv_last_error().decode()
        if rc == 0:
            assert lib.fftconv_plan_destroy(h) == 0
        return rc, msg

    passed = 0 if have_gpu else -6
    for fmt in (3, -1, 70000):
        rc, msg = create(64, 64, 3, 3, fftconv.PlanOptions(map_format=fmt))
        assert rc == -1 and "map_format is 0 (fp32), 1 (fp16) or 2 (bfloat16)" in msg
    for fmt in (0, 1, 2):
        assert create(64, 64, 3, 3, fftconv.PlanOptions(map_format=fmt))[0] == passed
    # sizes beyond max_transform make the plan block-wise: refused with a 16-bit format, and only then
    for fmt in (1, 2):
        rc, msg = create(600, 600, 9, 9, fftconv.PlanOptions(max_transform=512, map_format=fmt))
        assert rc == -1 and "block-wise" in msg and "map_format" in msg, (rc, msg)
    assert create(600, 600, 9, 9, fftconv.PlanOptions(max_transform=512))[0] == passed
    # ... as are large sizes that the planner prefers to run in blocks; opting out of blocks (blockwise = 1) lifts it
    # (7062 samples run on the long-row kernels: the cost model takes blocks of a mid-sized transform instead)
    rc, msg = create(7000, 7000, 63, 63, fftconv.PlanOptions(map_format=1))
    assert rc == -1 and "block-wise" in msg, (rc, msg)
    if not have_gpu:      # (on a GPU box this would set up a 7040 x 7040 plan: the GPU tier has its own one-pass cases)
        assert create(7000, 7000, 63, 63, fftconv.PlanOptions(map_format=1, blockwise=1))[0] == passed
    # a struct that ends before the field: the bytes behind it are not read
    o = fftconv.PlanOptions(map_format=3)
    o.struct_size = fftconv.PlanOptions.map_format.offset
    assert create(64, 64, 3, 3, o)[0] == passed
    o = fftconv.PlanOptions(max_transform=512, map_format=1)
    o.struct_size = fftconv.PlanOptions.verbose.offset         # (before `verbose` too)
    assert create(600, 600, 9, 9, o)[0] == passed
    # the option on a plan that is not one
    assert lib.fftconv_plan_set_option(None, b"map_format", 1) == -1
    # the one-shot binding sizes its maps by the format, and refuses one it does not know before the library is asked
    with pytest.raises(fftconv.FFTConvError):
        fftconv.cudaConvolutionFFT(np.zeros((8, 8, 1), np.float32), 3, 3, [np.zeros((3, 3, 1), np.float32)], options={"map_format": 5})
