"""Off-camera rays against the REFERENCE, without a GPU.

tests/golden/rays holds, per scene of tests/ray_sets.py, about 2,700 rays that no camera makes and the records the
reference's own Grid::Intersect wrote for them (oracle/gen_golden_rays.py, `refdriver rays`).  Here:

1. the fixture is intact (SHA-256s, family boundaries, the non-vacuity conditions on the reference's records) and has
   the structure the families promise (lattice origins bit for bit, both signs of zero);
2. tests/occlusion_ref.py -- the numpy restatement tests/test_gpu_occlusion.py holds the any-hit kernel to -- reproduces
   all eight record columns on every pinned ray, and its occlusion mode over (-inf, +inf) the reference's hit;
3. oracle/cpu_tracer.cpp (orc_trace_rays: the C++ restatement, the fallback CPU baseline) does the same;
4. where oracle/_ref/refdriver_instr is present, the reference itself still writes the committed records.

A ray is "pinned" unless rays.json lists it under "excluded": its reference result rests on undefined behaviour (an
int() of a NaN at grid.h:46).  At most 0.5 % of a scene may be listed.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import occlusion_ref as R
import ray_sets as RS
import synth_scenes as S
from conftest import ROOT, load_package

rtm = load_package()
META = RS.meta()
REFDRIVER_INSTR = os.path.join(ROOT, "oracle", "_ref", "refdriver_instr")
need_ref = pytest.mark.skipif(not os.access(REFDRIVER_INSTR, os.X_OK), reason="oracle/_ref/refdriver_instr not built")
FLOAT_COLS = (2, 3, 4)


def canon(rec):
    """8-word records with every NaN of t, u, v replaced by one pattern (synth_scenes.nan_canonical)."""
    out = np.array(rec, np.uint32)
    out[:, 2:5] = S.nan_canonical(out[:, 2:5])
    return out


def assert_records(got, want, keep, what):
    got, want = canon(got)[keep], canon(want)[keep]
    for j, c in enumerate(RS.REC_COLS):
        bad = np.flatnonzero(got[:, j] != want[:, j])
        assert bad.size == 0, (what, c, f"{bad.size} rays differ; first pinned row {int(bad[0])}: "
                               f"got {got[bad[0]]}, reference {want[bad[0]]}")


def rec8(res):
    """occlusion_ref's closest-mode result as the 8-word record."""
    r11 = R.rec11(res)
    return r11[:, [0, 1, 2, 3, 4, 8, 9, 10]]


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    """Per scene: (rays.json entry, rays, records, pinned mask, RefScene, scene path) -- loaded once, never changed."""
    tmp = tmp_path_factory.mktemp("raysets")
    cache = {}

    def get(scene):
        if scene not in cache:
            e = META["scenes"][scene]
            rays, rec = RS.load(scene)
            path = RS.scene_file(scene, tmp)
            hs = rtm.HostScene.load(path)
            try:
                sc = R.RefScene.from_host(hs)
                gm = hs.grid()[0]
            finally:
                hs.close()
            cache[scene] = (e, rays, rec, RS.pinned(e), sc, path, gm)
        return cache[scene]
    return get


# ------------------------------------------------------------------ 1. the fixture
def test_fixture_is_intact():
    assert tuple(META["scenes"]) == tuple(sorted(RS.SCENES)) and tuple(META["record"]) == RS.REC_COLS
    total = 0
    for scene in RS.SCENES:
        e = META["scenes"][scene]
        for key in ("rays", "rec"):
            with open(os.path.join(RS.RAYS, e[key]), "rb") as f:
                data = f.read()
            assert RS.sha256(data) == e[key + "_sha256"], (scene, key)
            assert len(data) < 100_000
            total += len(data)
        assert e["n"] == RS.TOTAL and {k: tuple(v) for k, v in e["families"].items()} == RS.bounds()
        rays, rec = RS.load(scene)
        assert np.isfinite(rays).all()
        assert RS.counts(rec, RS.pinned(e)) == {k: list(v) for k, v in e["counts"].items()}
        assert len(e["excluded"]) <= RS.MAX_EXCLUDED_SHARE * RS.TOTAL
        for x in e["excluded"]:
            assert x["reference"] and x["reason"] and 0 <= x["index"] < RS.TOTAL
        miss = rec[:, 0] == 0
        assert set(np.unique(rec[:, 0])) <= {0, 1}
        assert (rec[miss, 1] == RS.NOTRI).all() and (rec[miss, 2:5] == 0).all()
    assert total < 1_500_000


def test_reference_records_are_not_vacuous():
    """At least 20 % hits and 20 % misses per scene; A, B, E, G at least 32 of each per scene, D 16; C, F, H at least
    200 of each across the scenes -- all by the reference's records.  The only waiver: scene 1 is a closed box, so its
    interior family B cannot miss 32 times."""
    waived = [(s, f) for s in RS.SCENES for f in META["scenes"][s]["waived"]]
    assert waived == [("scene1", "B")], waived
    per_scene = {s: {k: list(v) for k, v in META["scenes"][s]["counts"].items()} for s in RS.SCENES}
    for s in RS.SCENES:
        print(s, " ".join(f"{n} {per_scene[s][n][0]}/{per_scene[s][n][1]}" for n in RS.NAMES))
    assert RS.check_non_vacuity(per_scene, waived) == []
    assert min(per_scene["scene1"]["B"]) > 0


@pytest.mark.parametrize("scene", RS.SCENES)
def test_family_structure(loaded, scene):
    e, rays, rec, keep, sc, path, gm = loaded(scene)
    g = e["grid"]
    assert g["dims"] == [int(x) for x in gm["dims"]]
    assert np.array_equal(S.bits_f32(g["aabb_min_bits"]), gm["aabb_min"]) and np.array_equal(S.bits_f32(g["aabb_max_bits"]), gm["aabb_max"])
    assert S.bits_f32([g["cell_wdh_bits"]])[0] == gm["cell_wdh"]
    box, b = RS.Box(gm), RS.bounds()
    o, d = rays[:, :3], rays[:, 3:]
    inside = ((o >= box.lo) & (o <= box.hi)).all(1)
    assert not (d == 0).all(1).any()
    # B inside, C and F outside, A at most a few cells outside (o + t d rounds)
    assert inside[slice(*b["B"])].all() and not inside[slice(*b["C"])].any() and not inside[slice(*b["F"])].any()
    # D: one or two exactly-zero components per ray, both signs of zero, and on-plane origins on a zeroed axis
    dd, do = d[slice(*b["D"])], o[slice(*b["D"])]
    nz = dd == 0
    assert (nz.sum(1) >= 1).all() and (nz.sum(1) <= 2).all()
    assert (nz & np.signbit(dd)).sum() >= 32 and (nz & ~np.signbit(dd)).sum() >= 32
    assert (nz[:128].sum(1) == 2).all() and (np.abs(dd[:128][~nz[:128]]) == 1).all()
    lat = np.stack([np.isin(do[:, a].view(np.uint32), RS.lattice_values(box, a).view(np.uint32)) for a in range(3)], axis=1)
    assert ((lat & nz).any(1)[3::4]).all()
    assert inside[slice(*b["D"])].any() and not inside[slice(*b["D"])].all()
    # E: 1 + i % 3 coordinates equal lo, hi or ToPos(k) bit for bit; a quarter with a zero component on such an axis
    eo, ed = o[slice(*b["E"])], d[slice(*b["E"])]
    lat = np.stack([np.isin(eo[:, a].view(np.uint32), RS.lattice_values(box, a).view(np.uint32)) for a in range(3)], axis=1)
    assert (lat.sum(1) >= 1 + np.arange(eo.shape[0]) % 3).all()
    assert inside[slice(*b["E"])].all()
    zero_on = (lat & (ed == 0)).any(1)
    assert 0.2 * eo.shape[0] <= zero_on.sum()
    assert (lat & (ed < 0)).any(1).sum() >= 0.25 * eo.shape[0]
    for k in (1, 2, 3):
        assert (lat.sum(1) == k).sum() >= 64
    # G: |d|_inf on both sides of 8
    dm = np.abs(d[slice(*b["G"])]).max(1)
    assert (dm > 8).sum() >= 48 and (dm <= 8).sum() >= 48
    # H: far origins
    far = np.abs(o[slice(*b["H"])] - box.ctr).max(1)
    assert (far > 30 * box.diag).all() and (far > 2.0 ** 19 * box.diag).sum() >= 40


# ------------------------------------------------------------------ 2. the numpy restatement
@pytest.mark.parametrize("scene", RS.SCENES)
def test_numpy_restatement_reproduces_the_reference(loaded, scene):
    """occlusion_ref.walk, closest mode: hit, tri, t, u, v, voxel, steps, tests of every pinned ray, bit for bit; any
    mode over (-inf, +inf), NULL and explicit: the reference's hit."""
    e, rays, rec, keep, sc, path, gm = loaded(scene)
    assert_records(rec8(R.walk(sc, rays, mode="closest")), rec, keep, f"{scene}: occlusion_ref closest mode")
    occ = R.walk(sc, rays, None, mode="any")["occluded"]
    np.testing.assert_array_equal(occ[keep], rec[keep, 0] == 1, err_msg=f"{scene}: occlusion over (-inf, +inf)")
    inf = np.tile(np.array([-np.inf, np.inf], np.float32), (rays.shape[0], 1))
    np.testing.assert_array_equal(R.walk(sc, rays, inf, mode="any")["occluded"], occ)


# ------------------------------------------------------------------ 3. the C++ restatement
def orc_trace_rays(oracle, path, rays):
    L = oracle.L
    L.orc_trace_rays.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    L.orc_trace_rays.restype = ctypes.c_int
    h = ctypes.c_void_p(L.orc_scene_load(path.encode()))
    assert h
    try:
        rays = np.ascontiguousarray(rays, np.float32)
        out = np.full((rays.shape[0] + 1, 8), S.SENTINEL, np.uint32)
        assert L.orc_trace_rays(h, ctypes.c_void_p(rays.ctypes.data), rays.shape[0], ctypes.c_void_p(out.ctypes.data)) == 0
        assert (out[-1] == S.SENTINEL).all()
        return out[:-1]
    finally:
        L.orc_scene_free(h)


@pytest.mark.parametrize("scene", RS.SCENES)
def test_cpp_restatement_reproduces_the_reference(loaded, oracle, scene):
    e, rays, rec, keep, sc, path, gm = loaded(scene)
    assert_records(orc_trace_rays(oracle, path, rays), rec, keep, f"{scene}: orc_trace_rays")


def test_orc_trace_rays_argument_checks(oracle, loaded):
    L = oracle.L
    L.orc_trace_rays.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    assert L.orc_trace_rays(None, None, 0, None) == 1
    path = loaded("inside")[5]
    h = ctypes.c_void_p(L.orc_scene_load(path.encode()))
    try:
        assert L.orc_trace_rays(h, None, 1, None) == 1 and L.orc_trace_rays(h, None, 0, None) == 0
    finally:
        L.orc_scene_free(h)


# ------------------------------------------------------------------ 4. the reference itself, where it is built
@need_ref
def test_reference_still_writes_the_committed_records(loaded, tmp_path):
    # a driver built before the `rays` command existed (a kept oracle/_ref that make did not refresh) is as good as
    # none: its usage line, printed when it is called without a command, does not name the command
    usage = subprocess.run([REFDRIVER_INSTR], capture_output=True, text=True, timeout=60).stderr
    if "rays" not in usage:
        pytest.skip("oracle/_ref/refdriver_instr predates the rays command: make -C oracle ref")
    e, rays, rec, keep, sc, path, gm = loaded("inside")
    rp, op = str(tmp_path / "in.f32"), str(tmp_path / "out.rec")
    rays.astype("<f4").tofile(rp)
    subprocess.run([REFDRIVER_INSTR, "rays", path, rp, op], check=True, capture_output=True, timeout=120)
    np.testing.assert_array_equal(np.fromfile(op, "<u4").reshape(-1, 8), rec)


# ------------------------------------------------------------------ 5. the comparison can fail
def test_one_flipped_word_is_noticed(loaded):
    """One bit of one record word flipped in a copy: the comparison used above fails, for every column."""
    e, rays, rec, keep, sc, path, gm = loaded("inside")
    row = int(np.flatnonzero(keep & (rec[:, 0] == 1))[7])
    for j in range(8):
        bad = rec.copy()
        bad[row, j] ^= 1
        with pytest.raises(AssertionError):
            assert_records(rec, bad, keep, "flipped")
    # ... and so does the comparison tests/test_gpu_ray_sets.py makes, on a faultless stand-in for the GPU's output
    rec12, hits = RS.expected_rec12(rec), RS.expected_hits(rec)
    RS.assert_words(rec12, RS.expected_rec12(rec), (5, 6, 7), keep, "stand-in records")
    RS.assert_words(hits, RS.expected_hits(rec), (1, 2, 3), keep, "stand-in hits")
    for j in range(8):
        bad = rec.copy()
        bad[row, j] ^= 1
        with pytest.raises(AssertionError):
            RS.assert_words(rec12, RS.expected_rec12(bad), (5, 6, 7), keep, "flipped")
        if 1 <= j <= 4:
            with pytest.raises(AssertionError):
                RS.assert_words(hits, RS.expected_hits(bad), (1, 2, 3), keep, "flipped")
    for j in range(8, 12):                             # colour and pad must be 0
        bad12 = rec12.copy()
        bad12[row, j] = 1
        with pytest.raises(AssertionError):
            RS.assert_words(bad12, rec12, (5, 6, 7), keep, "colour / pad")
    # an excluded row is the only place a difference may sit
    loose = keep.copy()
    loose[row] = False
    bad = rec.copy()
    bad[row, 2] ^= 1
    RS.assert_words(rec12, RS.expected_rec12(bad), (5, 6, 7), loose, "excluded row")


@pytest.mark.parametrize("scene", RS.SCENES)
def test_intervals_around_the_reference_t(loaded, scene):
    """The intervals tests/test_gpu_ray_sets.py uses, through the restatement's any-hit walk: with tmin = -inf an
    occluded ray has ref.hit && ref.t < tmax (include/rt_tracer.h), a ray over (-inf, +inf) is the reference's hit,
    and the intervals decide: some of the reference's hits are occluded and some are not."""
    e, rays, rec, keep, sc, path, gm = loaded(scene)
    tmm = RS.intervals(rays, rec, sc.diagonal())
    assert np.isnan(tmm).sum() == 0
    occ = R.walk(sc, rays, tmm, mode="any")["occluded"]
    hit, t = rec[:, 0] == 1, rec[:, 2].view(np.float32)
    open_below = keep & (tmm[:, 0] == -np.inf)
    assert not (occ & open_below & ~(hit & (t < tmm[:, 1]))).any()
    whole = open_below & (tmm[:, 1] == np.inf)
    assert whole.sum() >= 100
    np.testing.assert_array_equal(occ[whole], hit[whole])
    assert 0 < int(occ[keep & hit].sum()) < int((keep & hit).sum())
    # tmax = t exactly (strict bound) and tmax = nextafter(t, 0): never occluded by the hit at t itself
    i = np.arange(rays.shape[0])
    at_t = open_below & hit & np.isin((i // 3) % 6, (0, 1))
    assert at_t.sum() >= 20 and not occ[at_t].any()
