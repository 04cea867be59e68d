"""The CPU restatement (oracle/liboracle_tracer.so) reproduces every synthetic fixture of
oracle/gen_golden_synth.py, i.e. the reference's own code on scenes that are none of the ten shipped ones:
cells of 1,500 and 2,100 triangles, exact axis rays, eyes on grid faces and cell planes, grids one cell
thick, all-negative coordinates, degenerate triangles, NaN normals.  The GPU tests compare live against this
restatement where a mismatch should be printed per pixel, so it has to be pinned on the same scenes first.
Needs no GPU and no reference tree: the scenes are loaded from tests/golden/synth through orc_scene_load.
"""
import hashlib

import numpy as np
import pytest

import synth_scenes as S
from conftest import ALT_REC_DTYPE, ISECT

META = S.meta()
CASES = sorted(META["cases"])


@pytest.fixture(scope="module")
def scenes(oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("synth")
    cache = {}

    def get(entry):
        key = entry["scene"]
        if key not in cache:
            cache[key] = S.OracleScene(oracle, S.scene_file(entry, tmp))
        return cache[key]
    yield get
    for s in cache.values():
        s.close()


def test_every_case_of_the_issue_exists():
    """No case was dropped by the generator, and each one that is not all-miss by design has at least 100 hit
    and 100 miss samples in the reference's records."""
    assert META["dropped"] == {}
    assert set(CASES) == set(S.cases())
    for name, e in META["cases"].items():
        if e["all_miss"]:
            assert e["hit_samples"] == 0, name
        else:
            assert e["hit_samples"] >= 100 and e["miss_samples"] >= 100, name
    assert META["cases"]["stack1500"]["max_refs_per_cell"] == 1500     # >= wg64_max_refs, wh_auto_refs; packable
    assert META["cases"]["stack2100"]["max_refs_per_cell"] == 2100     # >= 2048: not packable
    assert META["cases"]["zero_normals"]["nan_samples"] > 0


def test_committed_scenes_are_what_the_builders_make(tmp_path):
    """The .rtscene files come from tests/synth_scenes.py's fixed seeds: rebuilding three of them here gives
    the committed bytes (the generator's reproducibility, checked where it is cheap)."""
    import gzip
    import os
    for name in ("fan_axis", "thin_y", "stack2100"):
        with gzip.open(os.path.join(S.SYNTH, name + ".rtscene.gz"), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == META["cases"][name]["rtscene_sha256"]
        hs = S.build_host(S.cases()[name])
        try:
            assert hs.grid()[0]["dims"] == META["cases"][name]["dims"]
            path = str(tmp_path / (name + ".rtscene"))
            hs.save(path)
            with open(path, "rb") as f:
                assert hashlib.sha256(f.read()).hexdigest() == META["cases"][name]["rtscene_sha256"], name
        finally:
            hs.close()


def check_frame(sc, e, tri_test=0):
    img, hid = sc.render(e["W"], e["H"], e["spp"], tri_test)
    if "bgra" in e:
        np.testing.assert_array_equal(img.reshape(-1), S.read_synth(e["bgra"], "<u4"), err_msg=e["name"])
    assert hashlib.sha256(img.tobytes()).hexdigest() == e["bgra_sha256"], e["name"]
    assert hashlib.sha256(hid.tobytes()).hexdigest() == e["hits_sha256"], e["name"]


@pytest.mark.parametrize("name", CASES)
def test_case_frames_and_records(scenes, name):
    """Frame, per-sample hit IDs and all 11 record columns (hit, tri, t, u, v, colour, voxel, DDA steps,
    tests) of every sample, at 62x46x4 and for the axis cases at 63x47x4."""
    e = META["cases"][name]
    for fr in [e] + ([e["axis_frame"]] if "axis_frame" in e else []):
        sc = scenes(fr)
        check_frame(sc, fr)
        S.check_rec11(S.to_rec11(sc.records(fr["W"], fr["H"], fr["spp"])), fr, what="oracle")


def test_axis_rays_do_what_the_cases_are_for():
    """The reference's own record of pixel (32, 24) sample 0 at 63x47: the fan's shared vertex is hit with
    u = v = 0 by the first triangle of the fan (strict '<' on equal t), and the axis ray of axis_x crosses
    all 64 cells of an empty row."""
    a = np.array([int(x, 16) for x in META["cases"]["fan_axis"]["axis_frame"]["axis_sample"]], np.uint32)
    assert a[0] == 1 and a[1] == 0 and a[3] == 0 and a[4] == 0
    b = np.array([int(x, 16) for x in META["cases"]["axis_x"]["axis_frame"]["axis_sample"]], np.uint32)
    assert b[0] == 0 and b[9] == 64 and b[10] == 0


@pytest.mark.parametrize("name", S.BARY_ALT)
def test_bary_and_alt(scenes, name):
    """IntersectRayTriBarycentric over the whole frame; brute force and the ray march on their windows."""
    e = dict(META["bary_alt"][name]["bary"], scene=name, W=S.W, H=S.H, spp=S.SPP)
    sc = scenes(e)
    check_frame(sc, e, tri_test=1)
    S.check_rec11(S.to_rec11(sc.records(S.W, S.H, S.SPP, tri_test=1)), e, what="oracle bary")
    for mode in ("brute", "march"):
        a = META["bary_alt"][name][mode]
        got = sc.records(S.W, S.H, S.SPP, (a["x0"], a["y0"], a["w"], a["h"]), tri_test=ISECT[mode] << 8)
        S.check_alt(got, S.read_synth(a["rec"], ALT_REC_DTYPE), mode, f"{name} {mode}")


@pytest.mark.parametrize("name", S.BIG)
def test_big_frames(scenes, name):
    b = dict(META["big"][name], scene=name, name=name + " 1920x1080x2")
    check_frame(scenes(b), b)


@pytest.mark.parametrize("scene", S.CAM_SCENES)
def test_seeded_cameras(scenes, golden, scene):
    """Sixteen seeded cameras per scene: the six exact axis directions, two eyes inside the grid, two on a
    grid face, one looking away, five random; the view bits are the ones tests/synth_scenes.py makes today."""
    views = {k: v for k, v in META["cameras"].items() if v["scene"] == scene}
    assert len(views) == 16
    names = [v["view"] for v in views.values()]
    assert sum(n.startswith("axis") for n in names) == 6 and sum(n.startswith("inside") for n in names) == 2
    assert sum(n.startswith("face") for n in names) == 2 and "away" in names
    assert views[f"{scene}_away"]["hit_samples"] == 0
    lo, hi = S.camera_box(scene, golden["scenes"], META)
    made = {n: c for n, c, _ in S.seeded_cameras(lo, hi, 45.0)}
    for v in views.values():
        assert [f"{x:08x}" for x in made[v["view"]].view(np.uint32)] == v["cam_bits"], v["view"]
        cam, fov = S.bits_f32(v["cam_bits"]), S.bits_f32([v["fov_bits"]])[0]
        img, hid = scenes(v).render(v["W"], v["H"], v["spp"], cam=cam, fov=fov)
        assert hashlib.sha256(img.tobytes()).hexdigest() == v["bgra_sha256"], v["view"]
        assert hashlib.sha256(hid.tobytes()).hexdigest() == v["hits_sha256"], v["view"]
