"""CPU tier: the in-register butterflies of csrc/butterflies.hpp (Dft<R, SGN>::run and the pruned run_nz<NZ>) built by g++
(the host path of fc_common.hpp, as tests/emu) for every radix the fast-kernel tables of fast_paths.hpp use, against a
float64 DFT -- in the product form (prime-factor butterflies for coprime composites) and under -DFC_DFT_PFA=0 (Cooley-Tukey
for every composite)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import util

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")


def table_radices():
    """every R1, R2, R3 of the row and column configuration tables: X(L, R1, R2, R3, ...)"""
    src = open(os.path.join(CSRC, "fast_paths.hpp")).read()
    rs = set()
    for m in re.finditer(r"^\s*X\((\d+),\s*(\d+),\s*(\d+),\s*(\d+),", src, re.M):
        rs.update(int(g) for g in m.groups()[1:])
    return sorted(rs)


RADICES = table_radices()

HARNESS = r"""
#include <cstdio>
#include "butterflies.hpp"
using namespace fc;
static unsigned lcg = 12345u;
static float rnd() { lcg = lcg * 1664525u + 1013904223u; return (float)((lcg >> 8) & 0xffff) / 32768.f - 1.f; }
// full transform: "full R SGN" + the input and the output (re im pairs)
template <int R, int SGN> void full() {
    c32 v[R];
    for (int i = 0; i < R; ++i) v[i] = mk(rnd(), rnd());
    printf("full %d %d", R, SGN);
    for (int i = 0; i < R; ++i) printf(" %.9g %.9g", v[i].x, v[i].y);
    Dft<R, SGN>::run(v);
    for (int i = 0; i < R; ++i) printf(" %.9g %.9g", v[i].x, v[i].y);
    printf("\n");
}
// pruned transform: "nz R SGN NZ" + the input (zero from NZ on), run_nz<NZ>'s output and run's output on the same input
template <int R, int SGN, int NZ> void pruned() {
    c32 v[R], w[R];
    for (int i = 0; i < R; ++i) v[i] = w[i] = i < NZ ? mk(rnd(), rnd()) : mk(0.f, 0.f);
    printf("nz %d %d %d", R, SGN, NZ);
    for (int i = 0; i < R; ++i) printf(" %.9g %.9g", v[i].x, v[i].y);
    Dft<R, SGN>::template run_nz<NZ>(v);
    Dft<R, SGN>::run(w);
    for (int i = 0; i < R; ++i) printf(" %.9g %.9g", v[i].x, v[i].y);
    for (int i = 0; i < R; ++i) printf(" %.9g %.9g", w[i].x, w[i].y);
    printf("\n");
}
template <int R> void radix() {
    full<R, -1>();
    full<R, +1>();
    static_for<1, R + 1>([&](auto nz_) {
        pruned<R, -1, decltype(nz_)::value>();
        pruned<R, +1, decltype(nz_)::value>();
    });
}
int main() {
RADIX_CALLS
    return 0;
}
"""


@pytest.fixture(scope="module", params=[1, 0], ids=["pfa", "ct"])
def butterfly_runs(request, tmp_path_factory):
    """{kind: [(R, SGN, NZ, arrays...)]} from the harness built with -DFC_DFT_PFA=<param>"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++) for the butterfly harness")
    d = tmp_path_factory.mktemp("butterflies_%d" % request.param)
    src = d / "harness.cpp"
    src.write_text(HARNESS.replace("RADIX_CALLS", "\n".join("    radix<%d>();" % r for r in RADICES)))
    exe = d / "harness"
    subprocess.run([cxx, "-O1", "-std=c++17", "-DFC_DFT_PFA=%d" % request.param, "-I", CSRC, str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    runs = {"full": [], "nz": []}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "full":
            r, sgn = int(f[1]), int(f[2])
            a = np.array(f[3:], dtype=np.float64).view(np.complex128)
            runs["full"].append((r, sgn, a[:r], a[r:]))
        else:
            r, sgn, nz = int(f[1]), int(f[2]), int(f[3])
            a = np.array(f[4:], dtype=np.float64).view(np.complex128)
            runs["nz"].append((r, sgn, nz, a[:r], a[r:2 * r], a[2 * r:]))
    return runs


def dft64(x, sgn):
    n = np.arange(len(x))
    return np.exp(sgn * 2j * np.pi * np.outer(n, n) / len(x)) @ x


def test_every_table_radix_is_covered(butterfly_runs):
    assert {4, 6, 8, 12, 16, 20, 22, 24} <= set(RADICES)
    assert sorted({(r, s) for r, s, _, _ in butterfly_runs["full"]}) == sorted((r, s) for r in RADICES for s in (-1, 1))
    assert len(butterfly_runs["nz"]) == 2 * sum(RADICES)


def test_full_transform_matches_float64_dft(butterfly_runs):
    bad = []
    for r, sgn, x, got in butterfly_runs["full"]:
        ref = dft64(x, sgn)
        err = np.max(np.abs(got - ref))
        if not err <= 4e-7 * r * np.max(np.abs(x)):
            bad.append((r, sgn, float(err)))
    assert not bad, bad


def test_pruned_transform_matches_full_run_and_float64_dft(butterfly_runs):
    bad = []
    for r, sgn, nz, x, got, full in butterfly_runs["nz"]:
        assert np.all(x[nz:] == 0)
        scale = 4e-7 * r * max(np.max(np.abs(x)), 1e-30)
        e_full = np.max(np.abs(got - full))
        e_ref = np.max(np.abs(got - dft64(x, sgn)))
        if not (e_full <= scale and e_ref <= scale):
            bad.append((r, sgn, nz, float(e_full), float(e_ref)))
    assert not bad, bad
