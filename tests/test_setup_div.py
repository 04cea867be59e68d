"""The DDA setup's quotients over one reciprocal per axis (csrc/rt_setup_div.h) on the CPU.
tests/setup_div_check.cpp compiles the header librt_tracer.so runs -- setup_div_operand_ok (the window of the
wave vote) and setup_div -- with g++ -ffp-contract=off and holds the new quotient against the IEEE n / d, bit
for bit, with the reciprocal 1.0f / d (which the device reciprocal equals wherever the window admits d):

  * real frames: every (n, d) pair dda_setup forms for every 16th tile of scenes 1, 4, 5 and 8 at
    1920x1080x4;
  * seven seeded families of 10^7 pairs each: d with an all-ones mantissa, d a power of two, n an exact
    multiple of d, quotients within 2 ulp of a binade edge, quotients within 2^-24 (relative) of a rounding
    midpoint (constructed from d), magnitudes 2^-140 .. 2^127, pairs that straddle the window on both sides.

Required: 0 mismatches inside the window, and every pair outside it takes the fall-back (the checker restates
the window on the operands' bit patterns and counts any disagreement with the header's decision).
"""
import json
import os
import subprocess

import pytest

from conftest import ROOT

SCENES = (1, 4, 5, 8)
FAMILIES = ("d_all_ones_mantissa", "d_power_of_two", "n_multiple_of_d", "quotient_near_binade_edge",
            "quotient_near_midpoint", "magnitudes_2^-140_to_2^127", "window_straddle")
PAIRS = 10_000_000


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("setupdiv") / "setup_div_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "setup_div_check.cpp"), "-o", exe], check=True)
    return exe


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def families(checker):
    return run(checker, "families", 20261019, PAIRS)["families"]


@pytest.mark.parametrize("scene", SCENES)
def test_setup_quotients_of_shipped_frames(checker, scene):
    rep = run(checker, "scene", os.path.join(ROOT, "data", "scenes", f"scene{scene}.rtscene"), 1920, 1080, 4, 16)
    print(rep)
    assert rep["tiles"] >= 8100 // 16
    s = rep["setup"]
    assert s["pairs"] > 1_000_000 and s["pairs"] == s["fast"] + s["fallback"], rep
    assert s["mismatches"] == 0 and s["window_errors"] == 0, rep
    # the reciprocal form is the common path of real frames, not a corner of them
    assert s["fast"] >= 0.99 * s["pairs"], rep


@pytest.mark.parametrize("family", FAMILIES)
def test_setup_quotients_of_crafted_family(families, family):
    assert set(families) == set(FAMILIES)
    rep = families[family]
    print(family, rep)
    assert rep["pairs"] >= PAIRS and rep["pairs"] == rep["fast"] + rep["fallback"], rep
    assert rep["mismatches"] == 0, rep
    assert rep["window_errors"] == 0, rep           # inside <=> reciprocal form, outside <=> fall-back
    assert rep["fast"] > 100_000, rep               # the family does reach the reciprocal form
    if family in ("magnitudes_2^-140_to_2^127", "window_straddle"):
        assert rep["fallback"] > 100_000, rep       # ... and these two the fall-back
        # the window is not decoration: outside it the reciprocal form does differ from n / d
        assert rep["outside_would_differ"] > 0, rep
