"""What the miss skip's device tests lean on, held on the CPU (tests/miss_skip_cases.py).

  * tests/miss_mask_check.cpp's new arguments (fov=, samples=, rank= / nranks=, the batch mode), on a checker built
    with the address and undefined-behaviour sanitizers where g++ links them: each against what it must reduce to.
  * The oracle's two additions: orc_render_smp (a caller's sample table) against orc_render_cam on the Hammersley table
    and -- on the single-cell scenes of tests/golden/cameras.json, whose hit IDs are the reference's own under
    camera_matrices.OFFSETS -- against the fixture; orc_scene_load_res against orc_scene_load.
  * The per-case flagged counts written into tests/test_gpu_miss_reach.py and tests/test_gpu_miss_sequences.py,
    re-derived: the groups' "reaches the skip" minima are chosen here, by the checker, not by the device.
"""
import os
import subprocess

import numpy as np
import pytest

import camera_matrices as cm
import miss_skip_cases as mk
import synth_scenes as ss
import test_gpu_miss_reach as reach
import test_gpu_miss_sequences as seq
from conftest import load_package

rtm = load_package()
SCENE4 = rtm.scene_path(4)
KEYS = ("items", "all_miss", "flagged")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return mk.build_checker(tmp_path_factory.mktemp("missargs"), sanitize=True)


def test_fov_argument(checker):
    own = mk.cpu_mask(checker, SCENE4, 256, 144, 4)
    hs = rtm.HostScene.load(4)
    try:
        assert mk.cpu_mask(checker, SCENE4, 256, 144, 4, fov=hs.fov) == own
        narrow, wide = (mk.cpu_mask(checker, SCENE4, 256, 144, 4, fov=f) for f in (hs.fov * 0.5, hs.fov * 1.5))
    finally:
        hs.close()
    assert narrow["flagged"] < own["flagged"] < wide["flagged"], (narrow, own, wide)


def test_samples_argument(checker, tmp_path):
    for spp in (1, 4, 16, 64):
        own = mk.cpu_mask(checker, SCENE4, 96, 54, spp)
        ham = mk.samples_file(tmp_path, f"hammersley{spp}", rtm.sample_table(spp))
        assert mk.cpu_mask(checker, SCENE4, 96, 54, spp, samples=ham) == own, spp
    wide = mk.samples_file(tmp_path, "wide", reach.sample_tables()["outside"])
    assert mk.cpu_mask(checker, SCENE4, 96, 54, 4, samples=wide)["flagged"] < mk.cpu_mask(checker, SCENE4, 96, 54, 4)["flagged"]
    short = mk.samples_file(tmp_path, "short", np.zeros((3, 2), np.float32))
    r = subprocess.run([checker, "scene", SCENE4, "96", "54", "4", "samples=" + short], capture_output=True, text=True)
    assert r.returncode == 2 and "float32" in r.stderr


@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
def test_shard_arguments(checker, nranks):
    """The ranks' items are the frame's, each once -- and a rank's item count is what rtm.shard_tile_ids (the Python
    statement of the deal, which tests/test_abi.py holds to the library) gives it."""
    W, H, spp = 250, 139, 4                  # ragged last tile column and row: 16 x 9 tiles
    whole = mk.cpu_mask(checker, SCENE4, W, H, spp)
    parts = [mk.cpu_mask(checker, SCENE4, W, H, spp, rank=r, nranks=nranks) for r in range(nranks)]
    for k in KEYS:
        assert sum(p[k] for p in parts) == whole[k], k
    tiles_x = (W + 15) // 16
    for r, p in enumerate(parts):
        n = 0
        for t in rtm.shard_tile_ids(W, H, r, nranks):
            tw, th = min(16, W - (t % tiles_x) * 16), min(16, H - (t // tiles_x) * 16)
            # a 4 x 4-pixel item (64 slots at spp 4) of the tile has a valid lane when its corner pixel is inside the frame
            n += ((tw + 3) // 4) * ((th + 3) // 4)
        assert p["items"] == n, (r, p, n)
    assert whole["flagged"] > 0


def test_batch_mode_and_bad_arguments(checker, tmp_path):
    cam = rtm.look_at((3.0, 2.0, 4.0), (0.0, 0.0, 0.0))
    smp = mk.samples_file(tmp_path, "t", reach.sample_tables()["seeded"])
    cases = [mk.case_args(96, 54, 4), mk.case_args(96, 54, 8, rect=(5, 3, 61, 47)), mk.case_args(64, 48, 4, cam=cam, fov=30.0),
             mk.case_args(96, 54, 4, cam=cam, samples=smp), mk.case_args(96, 54, 4, rank=1, nranks=2)]
    got = mk.cpu_masks(checker, SCENE4, cases, tmp_path)
    for c, g in zip(cases, got):
        r = subprocess.run([checker, "scene", SCENE4] + c, capture_output=True, text=True, check=True)
        assert '"flagged": %d,' % g["flagged"] in r.stdout and '"items": %d,' % g["items"] in r.stdout, (c, g, r.stdout)
    for bad in (["96", "54"], ["96", "54", "3"], ["96", "54", "128"], ["96", "54", "4", "rank=2", "nranks=2"],
                ["96", "54", "4", "1", "1", "96", "54"], ["96", "54", "4", "0", "0", "48", "54", "rank=0", "nranks=2"],
                ["96", "54", "4", "colour=1"]):
        r = subprocess.run([checker, "scene", SCENE4] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stdout, r.stderr)


def test_bounds_above_2_to_100_are_refused(checker):
    """No scene of the device tests has a bound above 2^100 (the caller-built grids keep their base scene's box), so the
    refusal is held here: the same view from 2^101 away along the camera's axis, and under a 3x3 times 2^101, leaves
    items that miss entirely and flags none of them; the same view from nearby does flag."""
    cam = rtm.look_at((1.8, 1.2, 5.0), (1.1, 0.6, 0.0)).reshape(4, 4)
    near = mk.cpu_mask(checker, SCENE4, 96, 54, 4, cam=cam.reshape(16))
    assert near["flagged"] > 0
    far = cam.copy()
    far[3, :3] = cam[3, :3] + np.float32(2.0 ** 101) * cam[2, :3]
    big = cam.copy()
    big[:3, :3] *= np.float32(2.0 ** 101)
    for c in (far, big):
        m = mk.cpu_mask(checker, SCENE4, 96, 54, 4, cam=c.reshape(16))
        assert m["flagged"] == 0 and m["all_miss"] > 0, m


# ------------------------------------------------------------------ the oracle's additions
def test_orc_render_smp_and_load_res(oracle, tmp_path):
    path = ss.gunzip_scene("axis_z", tmp_path)
    osc = ss.OracleScene(oracle, path)
    o16 = mk.oracle_scene(oracle, path, 16)
    try:
        cam = rtm.look_at((1.8, 1.2, 5.0), (1.1, 0.6, 0.0))
        for spp in (1, 4, 8):
            want = osc.render(96, 54, spp, cam=cam, fov=30.0)
            for tbl in (None, rtm.sample_table(spp)):
                got = mk.oracle_frame(oracle, osc.h, 96, 54, spp, cam, 30.0, tbl)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (spp, tbl is None)
        moved = mk.oracle_frame(oracle, osc.h, 96, 54, 4, cam, 30.0, rtm.sample_table(4) + np.float32(0.25))
        assert not np.array_equal(moved[0], want[0])
        a, b = osc.render(62, 46, 4), o16.render(62, 46, 4)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        osc.close()
        o16.close()


@pytest.mark.parametrize("scene", [s for s in reach.CAM_SCENES if s not in cm.GRID_SCENES])
def test_orc_render_smp_against_the_reference_hit_ids(oracle, tmp_path, scene, monkeypatch):
    """The single-cell scenes of tests/golden/cameras.json carry the reference's own hit IDs under a caller's sample table
    (camera_matrices.OFFSETS, `refdriver rays`): orc_render_smp's hit IDs must hash to them for all 19 matrices (CamScene
    .expected asserts it).  This is what makes its frames a reference for the caller-supplied tables."""
    monkeypatch.setattr(mk, "gpu_scene", lambda hs, skip: _NoDevice())
    sc = reach.CamScene(oracle, scene, tmp_path)
    try:
        for factor in cm.FACTOR_NAMES:
            sc.expected(factor)
    finally:
        sc.close()


class _NoDevice:
    def close(self):
        pass


# ------------------------------------------------------------------ the counts written into the GPU tests
@pytest.fixture(scope="module")
def fast_checker(tmp_path_factory):
    return mk.build_checker(tmp_path_factory.mktemp("misscounts"))


def test_reach_counts_cameras(oracle, fast_checker, tmp_path, monkeypatch):
    monkeypatch.setattr(mk, "gpu_scene", lambda hs, skip: _NoDevice())
    reached = 0
    for scene in reach.CAM_SCENES:
        sc = reach.CamScene(oracle, scene, tmp_path)
        try:
            cpus = mk.cpu_masks(fast_checker, sc.path, sc.checker_cases(), tmp_path, scene)
        finally:
            sc.close()
        for factor, cpu in zip(cm.FACTOR_NAMES, cpus):
            assert cpu["flagged"] == reach.CAM_FLAGGED.get(scene, {}).get(factor, 0), (scene, factor, cpu)
            assert cpu["flagged"] or cpu["all_miss"] == 0 or (scene, factor) in reach.CAM_REFUSED, (scene, factor, cpu)
            reached += cpu["flagged"] > 0
    assert reached == reach.CAM_MIN_FLAGGING
    bounds = {f: mk.cam_dir_bound(cm.from_bits(reach.FX["cams"]["scene1"][f])) for f in reach.CAM_FLAGGED["scene1"]}
    assert sum(mk.GATE_DMAX < b <= mk.RCP_MAX_DIR for b in bounds.values()) >= 2 and sum(b > mk.RCP_MAX_DIR for b in bounds.values()) >= 2
    assert mk.GATE_DMAX < bounds["scale_1+2^-13"] <= mk.RCP_MAX_DIR < bounds["scale_2^4"]


def test_reach_counts_synthetic_views_and_shipped_scenes(fast_checker, tmp_path):
    for name in reach.SYNTH_CASES:
        e0 = reach.META["cases"][name]
        for e in [e0] + ([e0["axis_frame"]] if "axis_frame" in e0 else []):
            cpu = mk.cpu_mask(fast_checker, ss.scene_file(e, tmp_path), e["W"], e["H"], e["spp"])
            if name in reach.SYNTH_ZERO:
                assert cpu["flagged"] == 0 and cpu["all_miss"] == 0, (e["name"], cpu)
            else:
                assert cpu["flagged"] == reach.SYNTH_FLAGGED[name], (e["name"], cpu)
    for sid in range(10):
        cpu = mk.cpu_mask(fast_checker, rtm.scene_path(sid), 256, 144, 4)
        if sid in reach.SHIPPED_ZERO:
            assert cpu["flagged"] == 0 and cpu["all_miss"] == 0, (sid, cpu)
        else:
            assert cpu["flagged"] == reach.SHIPPED_FLAGGED[sid] == seq.SHIPPED_FLAGGING[sid], (sid, cpu)
    assert sorted(list(reach.SHIPPED_ZERO) + list(reach.SHIPPED_FLAGGED)) == list(range(10))


def test_reach_counts_variants(oracle, fast_checker, tmp_path):
    from ray_variant_scenes import CallerBuilt
    for name in reach.FILE_VARIANTS:
        hs, _, ores = reach.variant_host(name, tmp_path)
        path = os.path.join(str(tmp_path), name + ".rtscene")
        hs.save(path)
        hs.close()
        assert mk.cpu_mask(fast_checker, path, reach.VW, reach.VH, reach.VSPP)["flagged"] == reach.VARIANT_FLAGGED[name], name
        osc = mk.oracle_scene(oracle, path, ores)
        try:
            assert (osc.render(reach.VW, reach.VH, reach.VSPP)[1] != cm.NOTRI).any(), name
        finally:
            osc.close()
    assert set(reach.VARIANT_FLAGGED) == set(reach.FILE_VARIANTS + reach.HUGE_VARIANTS) and min(reach.VARIANT_FLAGGED.values()) > 0
    assert CallerBuilt is reach.CallerBuilt


def test_reach_counts_spp_tables_and_fov(fast_checker, tmp_path):
    cam = mk.cam16(reach.CAM_A)
    for k, (name, (tris, res)) in enumerate(mk.synth_meshes().items()):
        hs = cm.host_scene(tris, rtm.look_at(*reach.CAM_A), fov=reach.FOV, grid_res=res)
        path = os.path.join(str(tmp_path), name + ".rtscene")
        hs.save(path)
        hs.close()
        for spp in (32, 64):
            assert mk.cpu_mask(fast_checker, path, 64, 48, spp, cam=cam)["flagged"] == reach.SPP_FLAGGED[(name, spp)]
        for tn, tbl in reach.sample_tables().items():
            got = mk.cpu_mask(fast_checker, path, 96, 54, 4, cam=cam, samples=mk.samples_file(tmp_path, tn, tbl))
            assert got["flagged"] == reach.TABLE_FLAGGED[tn][k], (name, tn, got)
        if name == "grid64":
            for fov in set(seq.FOVS):
                for spp in (4, 8):
                    assert mk.cpu_mask(fast_checker, path, seq.W, seq.H, spp, cam=cam, fov=fov)["flagged"] > 0
                for i, tbl in enumerate(seq.tables()):
                    smp = mk.samples_file(tmp_path, f"seq{i}", tbl)
                    assert mk.cpu_mask(fast_checker, path, seq.W, seq.H, 4, cam=cam, fov=fov, samples=smp)["flagged"] > 0
