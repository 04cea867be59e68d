"""The record gate (csrc/rt_record_gate.h) on the CPU.  tests/record_gate_check.cpp compiles
the header librt_tracer.so runs -- make_gate (k_origin_pre) and gate_rejects (the wave-uniform record loop)
-- with g++ and holds it against the first half of the per-camera-record test (rtd::mt_rec_first: det and u,
restated operation for operation):

  * soundness: NO (ray, record) pair has ok1 true and the gate rejecting -- over every lane test of every
    16th tile of scenes 1, 4, 5 and 8 at 1920x1080x4, and over eight seeded adversarial families of 10^6
    cases each (det at the 1e-8 threshold, rays a few ulp from the lines u = 0 and u = 1, vertex and edge
    hits, zero direction components, the origin in the triangle's plane, degenerate triangles, scales 2^-30
    .. 2^39, components above 2^40 where the bound must be +inf);
  * selectivity: on scene 8 the wave-level pass rate of the gate over wave-uniform lists of 8 records or
    more exceeds the ok1 vote's by at most 0.01 absolute (an always-pass gate would be sound too).
"""
import json
import os
import subprocess

import pytest

from conftest import ROOT

SCENES = (1, 4, 5, 8)
FAMILIES = ("det_near_1e-8", "u_lines", "vertex_edge_hits", "zero_direction_components", "origin_in_plane",
            "degenerate_triangles", "uniform_scales", "components_above_2^40")
CASES = 1_000_000


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("recgate") / "record_gate_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "record_gate_check.cpp"), "-o", exe], check=True)
    return exe


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def scene_reports(checker):
    return {n: run(checker, "scene", os.path.join(ROOT, "data", "scenes", f"scene{n}.rtscene"), 1920, 1080, 4, 16)
            for n in SCENES}


@pytest.fixture(scope="module")
def adversarial(checker):
    return run(checker, "adversarial", 20261019, CASES)["families"]


@pytest.mark.parametrize("scene", SCENES)
def test_gate_never_rejects_a_passing_lane_on_shipped_scenes(scene_reports, scene):
    rep = scene_reports[scene]
    print(rep)
    assert rep["one_origin"] and rep["tiles"] >= 8100 // 16
    assert rep["lane_tests"] > 100_000 and rep["ok1_true"] > 0 and rep["gate_rejects"] > 0, rep
    assert rep["violations"] == 0, rep


def test_gate_is_selective_on_killeroo(scene_reports):
    rep = scene_reports[8]
    assert rep["min_list"] == 8 and rep["long_records"] > 100_000, rep
    ok1 = rep["long_ok1_votes"] / rep["long_records"]
    gate = rep["long_gate_votes"] / rep["long_records"]
    print(f"wave votes over uniform lists >= 8: ok1 {ok1:.4f}, gate {gate:.4f}")
    assert 0.0 <= gate - ok1 <= 0.01, (ok1, gate)


@pytest.mark.parametrize("family", FAMILIES)
def test_gate_never_rejects_a_passing_lane_on_adversarial_family(adversarial, family):
    assert set(adversarial) == set(FAMILIES)
    rep = adversarial[family]
    print(family, rep)
    assert rep["cases"] >= CASES, rep
    assert rep["violations"] == 0, rep
    if family == "components_above_2^40":
        assert rep["e_finite"] == 0 and rep["gate_rejects"] == 0, rep
    else:
        assert rep["e_finite"] > 0 and rep["ok1_true"] > 0, rep       # the family does reach passing lanes
