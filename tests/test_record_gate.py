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

The bound E of a gate record holds for direction components up to kGateDmax = 1.0001.  rt_frame.cam's 3x3 need not
be orthonormal and the direction is normalised BEFORE it, so the library bounds |D_i| per frame from the matrix
(csrc/rt_cam_bound.h, rtk::cam_dir_bound -- the checker compiles the same function and reports it) and launches a
frame above the bound without gate records.  With tests/camera_matrices.py's matrices:

  * every matrix the library keeps the gate for is sound on all eight families (200,000 cases each);
  * at S = 1024 the gate is NOT sound (u_lines, vertex_edge_hits): why the fall-back exists;
  * on the frozen sliver scene (tests/golden/cameras.json) the wave vote skips a record a lane passes at S = 1024 --
    the wrong pixel of tests/test_gpu_camera_matrices.py -- and none at S = 1.
"""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import camera_matrices as C
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


# ------------------------------------------------------------------ cameras whose 3x3 is not orthonormal
CAM_CASES = 200_000
FX = C.fixture()
MATRICES = [(base, n, C.from_bits(cams[n])) for base, cams in sorted(FX["cams"].items()) for n in C.FACTOR_NAMES if n in cams]
CAM_OF = {(base, n): cam for base, n, cam in MATRICES}


@pytest.fixture(scope="module")
def bounds(checker):
    """{(base, factor): the checker's `bound` report}: rtk::cam_dir_bound and what the library does with it."""
    return {(base, n): run(checker, "bound", *C.hexf(C.m9_of(cam))) for base, n, cam in MATRICES}


@pytest.fixture(scope="module")
def gated_matrices(checker, bounds):
    """The adversarial families through every matrix that keeps the gate, eight runs at a time."""
    keep = [(base, n, cam) for base, n, cam in MATRICES if bounds[(base, n)]["gate_ok"]]
    with ThreadPoolExecutor(max_workers=8) as pool:
        reps = list(pool.map(lambda m: run(checker, "adversarial", 20261019, CAM_CASES, *C.hexf(C.m9_of(m[2]))), keep))
    return {(base, n): r for (base, n, _), r in zip(keep, reps)}


def test_cam_bound_sorts_the_matrices(bounds):
    """Which factors keep the gate and the fast reciprocal, by the function the library calls: the column norm of
    the 3x3 times (1 + 2^-20).  1 + 2^-14 is inside kGateDmax, 1 + 2^-13 and 1 + 2^-12 are not."""
    gate = {"identity", "scale_2^-45", "scale_2^-20", "scale_2^-10", "scale_2^-1", "scale_1/3", "scale_1+2^-14", "mirror",
            "rank2"}
    fast = gate | {"scale_2^1", "scale_3", "scale_1+2^-13", "scale_1+2^-12", "diag_1_4_1/4", "shear"}
    for (base, n), b in bounds.items():
        assert b["finite"] and b["gate_dmax"] == 1.0001 and b["rcp_max_dir"] == 8.0, b
        assert b["gate_ok"] == (n in gate), (base, n, b)
        assert b["fast_rcp_ok"] == (n in fast), (base, n, b)
        m = C.m9_of(CAM_OF[(base, n)]).astype("f8").reshape(3, 3)
        norm = float((m * m).sum(0).max() ** 0.5)
        assert norm <= b["cam_bound"] <= norm * (1 + 2.0 ** -19), (base, n, b, norm)


def test_cam_bound_of_a_non_finite_matrix_fails_both(checker):
    for bad in ("nan", "inf", "-inf"):
        for at in range(9):
            m = ["1", "0", "0", "0", "1", "0", "0", "0", "1"]
            m[at] = bad
            b = run(checker, "bound", *m)
            assert not b["gate_ok"] and not b["fast_rcp_ok"] and not b["finite"], (bad, at, b)


def test_gate_is_sound_for_every_matrix_that_keeps_it(gated_matrices):
    assert len(gated_matrices) == 9 * 6              # nine factors keep the gate, on six base cameras
    for key, rep in gated_matrices.items():
        assert rep["gate_ok"], key
        assert set(rep["families"]) == set(FAMILIES)
        for fam, r in rep["families"].items():
            assert r["cases"] >= CAM_CASES and r["violations"] == 0, (key, fam, r)
    # ... and not vacuously: the checker aims each family through the inverse matrix, so it reaches passing lanes
    # under a rotated, a mirrored and a shrinking camera alike
    for key in (("sliver", "identity"), ("scene8", "mirror"), ("inside", "scale_1/3"), ("scene1", "scale_2^-1")):
        for fam, r in gated_matrices[key]["families"].items():
            if fam != "components_above_2^40":
                assert r["ok1_true"] > 0 and r["e_finite"] > 0, (key, fam, r)


def test_gate_is_not_sound_at_1024(checker, bounds):
    """The gate's bound E is computed for unit directions: at S = 1024 it rejects lanes the first half passes.  This
    is why the library drops the gate for such frames; a guard "simplified" away would leave these violations in
    the kernel."""
    for base in ("sliver", "look_at"):
        assert not bounds[(base, C.S1024)]["gate_ok"]
        cam = CAM_OF[(base, C.S1024)]
        rep = run(checker, "adversarial", 20261019, CAM_CASES, *C.hexf(C.m9_of(cam)))
        assert not rep["gate_ok"]
        for fam in ("u_lines", "vertex_edge_hits"):
            print(base, fam, rep["families"][fam])
            assert rep["families"][fam]["violations"] > 0, (base, fam)


def test_wave_vote_skips_a_passing_record_on_the_sliver_scene(checker, tmp_path):
    """Scene mode on the frozen sliver scene (nine records, the sliver in the middle; 64x64x4, the suite's sample
    offsets, one cell): at S = 1024 the gate vote of some wave rejects the sliver's record in every lane while a
    lane's first half passes it -- the gated loop would skip it unloaded; with the orthonormal camera, none."""
    tris, cam = C.cell_scenes(FX)["sliver9_4"]
    hs = C.host_scene(tris, cam)
    path = str(tmp_path / "sliver.rtscene")
    try:
        hs.save(path)
    finally:
        hs.close()
    reps = {}
    for n in ("identity", C.S1024, "scale_2^20"):
        m = C.from_bits(FX["cams"]["sliver"][n])
        reps[n] = run(checker, "scene", path, C.W, C.H, C.SPP, 1, 8, "--cam", *C.hexf(m), "--grid-res", 1,
                      "--offsets", *C.hexf(C.OFFSETS))
        print(n, reps[n])
        assert reps[n]["one_origin"] and reps[n]["long_records"] == 9 * (C.W // 4) * (C.H // 4), reps[n]
        assert reps[n]["ok1_true"] > 0
    assert reps["identity"]["gate_ok"] and reps["identity"]["wholly_gated_ok1"] == 0 and reps["identity"]["violations"] == 0
    assert not reps[C.S1024]["gate_ok"] and reps[C.S1024]["wholly_gated_ok1"] >= 1
    assert reps["scale_2^20"]["wholly_gated_ok1"] >= 1
    assert {n: {k: r[k] for k in FX["sliver"]["gate_check"][n]} for n, r in reps.items()} == FX["sliver"]["gate_check"]
