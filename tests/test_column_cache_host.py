"""The record of what a plan's column-spectrum buffer A holds (csrc/column_cache.hpp: ColumnCache) on the CPU tier.

tests/column_cache_host/column_cache_host.cpp, a stand-alone host program over the product's header (built here with the host
compiler), drives the cache through the library's call sites next to a ground-truth model of A -- which set's first chunk it holds,
written on which stream, or garbage."""
import os
import re
import subprocess

import pytest

import util

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "column_cache_host")


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("column_cache_host") / "column_cache_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HOST_DIR, "column_cache_host.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, mode):
    r = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:]
    assert not any(line.startswith("FAIL") for line in r.stdout.splitlines())
    return r.stdout


def test_every_short_call_sequence_is_safe(host_program):
    """every sequence of up to 7 of the 12 calls that touch the record (deferred and direct preparation, flush, set_image's pair
    launch, convolves of two sets in one and two chunks, block-wise adopt, an option that forgets, overwritten kernels, a stream
    switch): a convolve skips its kernels' column pass only where A holds exactly that set's first chunk, of the set's present
    contents, written on the plan's present stream; nothing hits while a request is pending; a consumed record never hits again"""
    out = _run(host_program, "walk")
    m = re.search(r"length (\d+) over (\d+) operations: (\d+) sequences \(every prefix counted\), (\d+) hits", out)
    assert m, out
    length, nops, sequences, hits = map(int, m.groups())
    assert length >= 6 and nops >= 10
    assert sequences == sum(nops ** k for k in range(1, length + 1)) and sequences >= 10 ** 6
    assert hits > 0 and " 0 failed" in out


def test_documented_hits_happen(host_program):
    """prepare then convolve; a deferred prepare then convolve, or set_image (ONE pair launch, no column pass of the kernels' own)
    then convolve; a deferred prepare on one stream, a switch away (launched there) and back, then convolve; block 0's column
    spectra adopted by blocks 1..3 -- each skips the column pass; a consumed, forgotten or overwritten record, a record of another
    stream and a request whose launch failed do not"""
    out = _run(host_program, "hits")
    assert " 0 failed" in out
