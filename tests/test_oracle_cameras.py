"""tests/golden/cameras.json (oracle/gen_golden_cameras.py: the reference's own frames and hit IDs under cameras whose
3x3 is not orthonormal) against the CPU restatements the GPU tests compare with first -- liboracle_tracer.so
(OracleScene.render(cam=, fov=)) for the 64-cell scenes, tests/occlusion_ref.py's walk on the numpy GenerateRay's
rays for the single-cell scenes -- and the fixture's own consistency.  CPU only."""
import hashlib
import json

import numpy as np
import pytest

import camera_matrices as C
import occlusion_ref as R
import synth_scenes as S

FX = C.fixture()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_fixture_is_complete():
    """Every factor on every scene, nothing dropped for the uniform scales and the mirror, every matrix is the factor
    applied to its base camera, bit for bit."""
    assert FX["factors"] == C.FACTOR_NAMES
    for k in FX["dropped"]:
        assert k.split("|")[1] not in C.NO_SKIP, k
    cells = C.cell_scenes(FX)
    for scene in list(cells) + list(C.GRID_SCENES):
        for n in C.FACTOR_NAMES:
            assert f"{scene}|{n}" in FX["cases"] or f"{scene}|{n}" in FX["dropped"], (scene, n)
    fac = dict(C.factors())
    bases = {b: C.from_bits(v["cam_bits"]) for b, v in FX["bases"].items()}
    assert C.bits(cells["facing9"][1]) == FX["bases"]["look_at"]["cam_bits"]
    assert FX["sliver"]["cam_bits"] == FX["bases"]["sliver"]["cam_bits"]
    for base, cams in FX["cams"].items():
        for n, f in fac.items():
            if n in cams:
                assert C.bits(C.apply_factor(bases[base], f)) == cams[n], (base, n)


def test_sliver_scene_regenerates_from_its_seed():
    """The frozen bits are what camera_matrices builds from the recorded seed and width."""
    s = FX["sliver"]
    cam = C.sliver_camera(s["seed"])
    assert C.bits(cam) == s["cam_bits"]
    for nt, pos in C.SLIVER_LISTS:
        assert C.bits(C.sliver_scene(cam, s["width"], nt, pos)) == s["scenes"][f"{nt}_{pos}"]


def test_background_only_at_2_to_the_minus_45():
    """At 2^-45 every |det| is below the 1e-8 threshold: the reference's frames are background only."""
    n = 0
    for k, e in FX["cases"].items():
        if e["factor"] == "scale_2^-45":
            assert e["hit_samples"] == 0, k
            n += 1
    assert n == len(C.cell_scenes(FX)) + len(C.GRID_SCENES)


def test_numpy_generate_ray_matches_the_pinned_restatement(oracle):
    """camera_matrices.generate_rays against orc_kat_genray (pinned to the reference's recorded rays by
    test_oracle_golden.py) on every matrix of the fixture, every fifth pixel of a 64x64x4 frame."""
    smp = C.OFFSETS.reshape(-1, 2)
    y, x, s = [a.reshape(-1) for a in np.meshgrid(np.arange(4, C.H, 5), np.arange(4, C.W, 5), np.arange(C.SPP), indexing="ij")]
    for base, cams in FX["cams"].items():
        fov = float(C.from_bits([cams["fov_bits"]])[0]) if "fov_bits" in cams else 45.0
        for n in C.FACTOR_NAMES:
            if n not in cams:
                continue
            cam = C.from_bits(cams[n])
            rin = np.zeros((x.size, 23), np.float32)
            rin[:, :16] = cam
            b = rin.view(np.uint32)
            b[:, 16], b[:, 17], b[:, 18], b[:, 19] = x, y, C.W, C.H
            rin[:, 20], rin[:, 21], rin[:, 22] = smp[s, 0], smp[s, 1], np.float32(fov)
            want = oracle.kat("genray", rin, 6)
            got = C.generate_rays(cam, fov, C.W, C.H, smp).reshape(C.H, C.W, C.SPP, 6)[4::5, 4::5].reshape(-1, 6)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (base, n)


@pytest.mark.parametrize("scene", C.GRID_SCENES)
def test_restatement_renders_the_reference_frames(oracle, scene, tmp_path):
    osc = S.OracleScene(oracle, S.scene_file({"scene": scene}, tmp_path))
    try:
        fov = float(C.from_bits([FX["cams"][scene]["fov_bits"]])[0])
        for n in C.FACTOR_NAMES:
            e = FX["cases"].get(f"{scene}|{n}")
            if e is None:
                continue
            img, hid = osc.render(e["W"], e["H"], e["spp"], cam=C.from_bits(FX["cams"][scene][n]), fov=fov)
            assert sha(img) == e["bgra_sha256"] and sha(hid) == e["hits_sha256"], (scene, n)
            assert int((hid != C.NOTRI).sum()) == e["hit_samples"]
    finally:
        osc.close()


@pytest.mark.parametrize("scene", ["facing9", "edge_on17", "sliver8_0", "sliver9_4", "sliver17_16"])
def test_walk_restatement_finds_the_reference_hits(scene):
    tris, _ = C.cell_scenes(FX)[scene]
    hs = C.host_scene(tris, C.cell_scenes(FX)[scene][1])
    try:
        sc = R.RefScene.from_host(hs)
    finally:
        hs.close()
    for k, e in FX["cases"].items():
        if e["scene"] != scene:
            continue
        cam = C.from_bits(FX["cams"][e["cam"]][e["factor"]])
        res = R.walk(sc, C.generate_rays(cam, 45.0, C.W, C.H, C.OFFSETS.reshape(-1, 2)))
        hid = np.where(res["hit"], res["tri"], np.uint32(C.NOTRI)).astype(np.uint32)
        assert sha(hid) == e["hits_sha256"], k


def test_fixture_is_canonical_json():
    with open(C.FIXTURE) as f:
        text = f.read()
    assert text == C.fixture_text(FX)
    assert C.expand(json.loads(text)) == FX
