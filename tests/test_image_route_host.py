"""The way of an image into a one-pass plan (csrc/image_route.hpp: plan_image_route) on the CPU tier.

tests/image_route_host/image_route_host.cpp, a stand-alone host program over the product's headers (built here with the host
compiler), holds the route against a literal transcription of the conditions set_images_impl had before the route existed, over
the full product of what the decision depends on, and against hand-written expectations for the documented routes."""
import os
import re
import subprocess

import pytest

import util

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "image_route_host")

# the axes of the table walk: formats, locations, host_pinned, byte sizes (at and one element past both pin limits), pixel_store,
# border_store, fast_fwd, {bordered kernel built, not built}, (border, normalise) in {off/0, off/1, on/0}, request states
AXES = (5, 2, 2, 4, 2, 2, 2, 2, 3, 3)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("image_route_host") / "image_route_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HOST_DIR, "image_route_host.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, mode):
    r = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:]
    assert not any(line.startswith("FAIL") for line in r.stdout.splitlines())
    return r.stdout


def test_route_equals_the_conditions_it_replaced(host_program):
    """plan_image_route gives, for every combination of pixel format, location, host_pinned, batch bytes at and one element past
    both pin limits, pixel_store, border_store, specialised or generic column pass, a length with and without the bordered kernel,
    border or normalisation or neither, and the three states of a recorded kernel preparation, what the interleaved conditions of
    the former set_images_impl gave: source, landing buffer, conversion, extension, column launch, flush, buffer sizes, the
    statistics' format, the pinned mark and the final sync.  The count is the product of the axes: no axis is skipped."""
    out = _run(host_program, "table")
    m = re.search(r"table: (\d+) combinations compared, (\d+) differ", out)
    assert m, out
    compared, differ = map(int, m.groups())
    product = 1
    for a in AXES:
        product *= a
    assert compared == product == 11520
    assert differ == 0


def test_documented_routes(host_program):
    """the routes DESIGN.md states, one line each: fp32 device; fp32 host pinned in place, pinned then copied, pageable with a sync;
    uint8 direct in place and staged through IT and I; uint8 with a border, direct and staged; a border staged on a generic plan;
    a recorded preparation riding in the pair launch, flushed from another stream, and flushed by itself ahead of a typed-direct or
    bordered launch; the statistics of normalised maps reading the typed pixels"""
    out = _run(host_program, "named")
    assert out.count("\nok  ") + out.startswith("ok  ") >= 20 and "named: 0 failed" in out
