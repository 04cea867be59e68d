"""The miss skip's proof (csrc/rt_miss_mask.h) on the CPU.  tests/miss_mask_check.cpp compiles the
header librt_tracer.so runs -- provably_misses -- with g++ -ffp-contract=off over the oracle (oracle/cpu_tracer.cpp)
and walks the kernel's own work items, 64 consecutive sample slots of a 16x16 tile in Morton order:

  * whole 1920x1080x4 frames of scenes 0, 1, 4, 5 and 8; spp 1, 2, 8 and 16 at 480x270;
  * the orbit cameras of the moving_views fixtures and every matrix of tests/camera_matrices.py;
  * seeded families: the origin a few ulp outside each box face and in its plane, exactly-zero direction
    components, the box behind the camera, a box seen edge-on, the 3x3 scaled by 2^-45 .. 2^45 (and sheared, and
    with a zero row), unaligned regions whose last tile overhangs the frame.

Required: NO flagged item holds a sample that passes PointAABB or RayAABB (a flagged item is not traced).
Coverage -- flagged items over items whose samples all miss -- must be at least 0.95 for scenes 0, 1 and 4 at
1080p x 4 (measured: 0.995, 0.989, 0.989); scenes 5 (camera inside the box) and 8 (the ground's box fills the
frame) must flag nothing.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import camera_matrices as cm
from conftest import ROOT

SCENES = (0, 1, 4, 5, 8)
FAMILIES = ("origin_at_faces", "zero_direction_components", "box_behind_camera", "box_edge_on", "matrix_scales",
            "unaligned_regions")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("missmask") / "miss_mask_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "miss_mask_check.cpp"),
                    "-o", exe], check=True)
    return exe


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def scene_file(sid):
    return os.path.join(ROOT, "data", "scenes", f"scene{sid}.rtscene")


def cam_args(cam_bits):
    return [float(x).hex() for x in cm.from_bits(cam_bits)]


@pytest.mark.parametrize("sid", SCENES)
def test_whole_frames_1080p4(checker, sid):
    m = run(checker, "scene", scene_file(sid), 1920, 1080, 4)["mask"]
    print(sid, m)
    assert m["items"] == 129600 and m["flagged_with_hit"] == 0, m
    assert m["flagged"] <= m["all_miss"], m
    if sid in (5, 8):
        assert m["flagged"] == 0 and m["all_miss"] == 0, m
    else:
        assert m["all_miss"] > 30000 and m["flagged"] >= 0.95 * m["all_miss"], m


@pytest.mark.parametrize("spp", [1, 2, 8, 16])
def test_other_sample_counts(checker, spp):
    for sid in (1, 4):
        m = run(checker, "scene", scene_file(sid), 480, 270, spp)["mask"]
        print(sid, spp, m)
        full = 30 * 17 * 4 * spp            # (270 rows: items of the last tile row without a valid lane are not counted)
        assert 0.9 * full < m["items"] <= full and m["flagged_with_hit"] == 0, m
        assert 0 < m["flagged"] <= m["all_miss"], m


def test_orbit_cameras(checker, golden):
    mv = golden["moving_views"]
    assert len(mv) >= 4
    for name, v in sorted(mv.items()):
        m = run(checker, "scene", scene_file(v["scene"]), 480, 270, 4, 0, 0, 480, 270, *cam_args(v["cam_bits"]))["mask"]
        print(name, m)
        assert m["flagged_with_hit"] == 0 and m["flagged"] <= m["all_miss"], (name, m)


def test_every_camera_matrix(checker, tmp_path):
    """Every base camera of the fixture (the 64-cell scenes', the sliver scenes' seeded rotation, look_at) times
    every factor, each over the box of a scene it is used with."""
    import synth_scenes as ss
    fx = cm.fixture()
    assert set(fx["cams"]) == set(cm.GRID_SCENES) | {"sliver", "look_at"}
    files = {s: (ss.scene_file({"scene": s}, tmp_path), cm.CAM_FRAME) for s in cm.GRID_SCENES}
    cells = cm.cell_scenes(fx)
    for base, name in (("sliver", "sliver9_4"), ("look_at", "facing9")):
        hs = cm.host_scene(*cells[name])
        files[base] = (str(tmp_path / f"{name}.rtscene"), (cm.W, cm.H, cm.SPP))
        hs.save(files[base][0])
        hs.close()
    flagged = 0
    for base, (path, (W, H, spp)) in files.items():
        for factor in cm.FACTOR_NAMES:
            m = run(checker, "scene", path, W, H, spp, 0, 0, W, H, *cam_args(fx["cams"][base][factor]))["mask"]
            print(base, factor, m)
            assert m["flagged_with_hit"] == 0 and m["flagged"] <= m["all_miss"], (base, factor, m)
            flagged += m["flagged"]
    assert flagged > 0


@pytest.fixture(scope="module")
def families(checker):
    return run(checker, "families", 20261020)["families"]


@pytest.mark.parametrize("family", FAMILIES)
def test_seeded_family(families, family):
    assert set(families) == set(FAMILIES)
    m = families[family]
    print(family, m)
    assert m["items"] > 300 and m["flagged_with_hit"] == 0 and m["flagged"] <= m["all_miss"], m
    if family != "origin_at_faces":
        assert m["flagged"] > 0, m          # the family does reach the proof, not only its refusals
