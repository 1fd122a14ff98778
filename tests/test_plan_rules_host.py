"""The plan setters' two tables (csrc/plan_rules.hpp: kPlanRules / plan_refusal, kSetterEffects) on the CPU tier.

tests/plan_rules_host/plan_rules_host.cpp, a stand-alone host program over the product's headers (built here with the host compiler),
holds the rule function against a literal transcription of the `if` chains that were spread over set_score, fftconv_plan_set_border,
fftconv_plan_set_spectral_filter, the spectrum import and fftconv_plan_mark_spectrum_valid before the table existed, over the full
product of the state the rules read and every request, and the effects table against a literal list of what each entry point did.
tests/test_plan_setters_gpu.py pins what a caller sees of both on the GPU."""
import os
import re
import subprocess

import pytest

import util

CSRC = os.path.join(util.ROOT, "cuda-fft-convolution_amd", "csrc")
HOST_DIR = os.path.join(util.ROOT, "tests", "plan_rules_host")

# the state axes: block-wise {0, 1}, F {1, 2}, score 0-4, border 0-5, filter 0-2, rows {generic, specialised with the filter kernel,
# specialised at 7040}
STATES = (2, 2, 5, 6, 3, 3)
# the requests: score 0-4, border 0-5, filter 0-2, import, mark-valid
REQUESTS = 5 + 6 + 3 + 1 + 1


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_rules_host") / "plan_rules_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(HOST_DIR, "plan_rules_host.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, mode):
    r = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:]
    assert not any(line.startswith("FAIL") for line in r.stdout.splitlines())
    return r.stdout


def test_rules_equal_the_conditions_they_replaced(host_program):
    """plan_refusal gives, for every state -- the ones the entry points make unreachable (a score on a block-wise plan, a score beside
    a border) included -- and every request, what the former conditions gave: whether the request is refused, the error code, and
    the formatted message byte for byte.  Every row of the table refuses at least one combination.  The count is the product of the
    axes: no axis is skipped."""
    out = _run(host_program, "rules")
    m = re.search(r"rules: (\d+) comparisons, (\d+) refused, (\d+) differ", out)
    assert m, out
    compared, refused, differ = map(int, m.groups())
    states = 1
    for a in STATES:
        states *= a
    assert states == 1080 and REQUESTS == 16
    assert compared == states * REQUESTS == 17280
    assert 0 < refused < compared
    assert differ == 0


def test_effects_equal_the_sequences_they_replaced(host_program):
    """kSetterEffects states, per entry point, what the setter did ahead of its assignments: the asymmetries included (a score keeps
    the ring, the rectangle and the region have no early return, the filter waits for nothing)"""
    out = _run(host_program, "effects")
    assert out.count("\nok  ") + out.startswith("ok  ") == 6 and "effects: 0 failed" in out
