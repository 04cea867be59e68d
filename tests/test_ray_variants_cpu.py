"""The ray-variant scenes (tests/ray_variant_scenes.py) and their fixtures (tests/golden/ray_variants), without a GPU.

1. the fixture is intact: SHA-256s, shapes, family boundaries, counts, the non-vacuity conditions; the meshes
   regenerated from their seeds have the recorded SHA-256s and the grids the recorded meta (a mismatch fails);
2. the rays have the structure the families promise on these boxes too (test_ray_sets_cpu.test_family_structure);
3. tests/occlusion_ref.py's walk, closest mode, reproduces all eight columns of the reference's records on the ribbons
   and sheets16 (grids of 513 x 3 x 3, 3 x 3 x 512 and 16^3 cells; pinned rays, NaN == NaN);
4. on the two huge scenes, whose grids the reference cannot build, the walk reproduces the committed records (drift),
   and its ray/triangle half is anchored: occlusion_ref.ray_tri and orc_kat_ray_tri equal `refdriver tri`'s committed
   answers on every (ray, appended triangle) pair -- the hit flag on all, t, u, v on the hits, non-finite u and v included;
5. the interval contract: any-hit over ray_sets.intervals against the records;
6. where oracle/_ref is built, the drivers still write the committed records;
7. one flipped word, byte or vertex is noticed.
"""
import os
import subprocess

import numpy as np
import pytest

import occlusion_ref as R
import ray_sets as RS
import ray_variant_scenes as V
import synth_scenes as S
import test_ray_sets_cpu as T
from conftest import ROOT

META = V.meta()
REFDRIVER = os.path.join(ROOT, "oracle", "_ref", "refdriver")
REFDRIVER_INSTR = os.path.join(ROOT, "oracle", "_ref", "refdriver_instr")
need_ref = pytest.mark.skipif(not (os.access(REFDRIVER, os.X_OK) and os.access(REFDRIVER_INSTR, os.X_OK)),
                              reason="oracle/_ref drivers not built")


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    """Per scene: (json entry, rays, records, pinned mask, RefScene, the Scene, grid meta) -- built once, never changed."""
    tmp = tmp_path_factory.mktemp("rayvariants")
    cache = {}

    def get(name):
        if name not in cache:
            e = META["scenes"][name]
            rays, rec = V.load(name)
            sc = V.Scene(name, tmp)
            cache[name] = (e, rays, rec, RS.pinned(e), sc.ref, sc, sc.gm)
        return cache[name]
    yield get
    for c in cache.values():
        c[5].close()


# ------------------------------------------------------------------ 1. the fixture
def test_fixture_is_intact():
    assert tuple(META["scenes"]) == tuple(sorted(V.SCENES)) and tuple(META["record"]) == RS.REC_COLS
    assert set(os.listdir(V.DIR)) == {"ray_variants.json", META["huge_tri"]} | {s + x for s in V.SCENES for x in (".rays.gz", ".rec.gz")}
    for scene in V.SCENES:
        e = META["scenes"][scene]
        for key in ("rays", "rec"):
            with open(os.path.join(V.DIR, e[key]), "rb") as f:
                data = f.read()
            assert RS.sha256(data) == e[key + "_sha256"], (scene, key)
            assert len(data) < V.MAX_FILE
        assert e["n"] == RS.TOTAL and {k: tuple(v) for k, v in e["families"].items()} == RS.bounds()
        assert e["info"] == V.INFO[scene] and e["grid_res"] == V.GRID_RES.get(scene, 64)
        rays, rec = V.load(scene)
        assert np.isfinite(rays).all() and rays.shape[0] % 64 != 0
        keep = RS.pinned(e)
        assert RS.counts(rec, keep) == {k: list(v) for k, v in e["counts"].items()}
        assert len(e["excluded"]) <= RS.MAX_EXCLUDED_SHARE * RS.TOTAL
        for x in e["excluded"]:
            assert x["reference"] and x["reason"] and 0 <= x["index"] < RS.TOTAL
        miss = rec[:, 0] == 0
        assert set(np.unique(rec[:, 0])) <= {0, 1}
        assert (rec[miss, 1] == RS.NOTRI).all() and (rec[miss, 2:5] == 0).all()
        assert int(rec[keep, 6].max()) == e["longest_walk"]
    with open(os.path.join(V.DIR, META["huge_tri"]), "rb") as f:
        data = f.read()
    assert RS.sha256(data) == META["huge_tri_sha256"] and len(data) < V.MAX_FILE
    assert set(V.load_huge_tri()) == set(V.HUGE_SCENES)


def test_records_are_not_vacuous():
    """Per scene: hits and misses each >= 20 % of the pinned rays; A, B, E, G >= 32 of each, D >= 16; the only waiver
    is sheets16's B (every interior ray hits one of 7,000 sheets); each huge scene has >= 100 closest hits on the
    appended triangle, and at least one with a non-finite u or v.  The 513-cell walks are longer than 512 cells."""
    for s in V.SCENES:
        e = META["scenes"][s]
        c = {k: list(v) for k, v in e["counts"].items()}
        print(s, " ".join(f"{n} {c[n][0]}/{c[n][1]}" for n in RS.NAMES), "occluded", e["occluded"], "excluded", len(e["excluded"]))
        assert e["waived"] == [f for w, f in V.WAIVED if w == s]
        assert V.check_non_vacuity(s, c) == []
        hits = sum(v[0] for v in c.values())
        assert 0 < e["occluded_hits"] < hits
    assert META["scenes"]["sheets16"]["counts"]["B"] == [384, 0]
    for s in ("ribbon_x513", "ribbon_y513", "ribbon_z513"):
        assert META["scenes"][s]["longest_walk"] > 512
    tri = V.load_huge_tri()
    for s in V.HUGE_SCENES:
        e = META["scenes"][s]
        rays, rec = V.load(s)
        keep = RS.pinned(e)
        hit = keep & (rec[:, 0] == 1)
        big = int(rec[hit, 1].max())
        assert int((hit & (rec[:, 1] == big)).sum()) == e["big_tri_hits"] >= V.MIN_BIG_TRI_HITS
        on = tri[s][:, 0] == 1
        odd = on & ~np.isfinite(tri[s][:, 2:].view(np.float32)).all(1)
        assert int(on.sum()) == e["big_tri_pair_hits"] and int(odd.sum()) == e["nonfinite_uv_pair_hits"] >= V.MIN_NONFINITE_UV.get(s, 0)
        assert int((hit & ~np.isfinite(rec[:, 3:5].view(np.float32)).all(1)).sum()) == e["nonfinite_uv_records"] >= 1


@pytest.mark.parametrize("scene", V.SCENES)
def test_scene_regenerates(loaded, scene):
    """The mesh from its seed has the recorded SHA-256s, the grid the recorded meta and reference count."""
    e, rays, rec, keep, ref, sc, gm = loaded(scene)
    assert sc.mesh_shas() == e["mesh"], scene
    sc.check_static()
    g = e["grid"]
    assert g["dims"] == [int(x) for x in gm["dims"]] and e["num_refs"] == sc.num_refs
    assert np.array_equal(S.bits_f32(g["aabb_min_bits"]), gm["aabb_min"]) and np.array_equal(S.bits_f32(g["aabb_max_bits"]), gm["aabb_max"])
    assert S.bits_f32([g["cell_wdh_bits"]])[0] == gm["cell_wdh"]
    if scene in V.HUGE_SCENES:
        assert sc.big == sc.t.shape[0] - 1 and int((ref.cell_tris == sc.big).sum()) == sc.host.listed == 625


# ------------------------------------------------------------------ 2. the families on these boxes
@pytest.mark.parametrize("scene", V.SCENES)
def test_family_structure(loaded, scene):
    T.test_family_structure(lambda s: loaded(s)[:5] + (None, loaded(s)[6]), scene)


# ------------------------------------------------------------------ 3. the restatement against the reference
@pytest.mark.parametrize("scene", V.REFERENCE_SCENES)
def test_numpy_restatement_reproduces_the_reference(loaded, scene):
    e, rays, rec, keep, ref, sc, gm = loaded(scene)
    assert e["records_from"].startswith("Grid::Intersect")
    T.assert_records(V.rec8(R.walk(ref, rays, mode="closest")), rec, keep, f"{scene}: occlusion_ref closest mode")
    occ = R.walk(ref, rays, None, mode="any")["occluded"]
    np.testing.assert_array_equal(occ[keep], rec[keep, 0] == 1, err_msg=f"{scene}: occlusion over (-inf, +inf)")


# ------------------------------------------------------------------ 4. the huge scenes
@pytest.mark.parametrize("scene", V.HUGE_SCENES)
def test_walk_reproduces_the_committed_records(loaded, scene):
    e, rays, rec, keep, ref, sc, gm = loaded(scene)
    T.assert_records(V.rec8(R.walk(ref, rays, mode="closest")), rec, keep, f"{scene}: occlusion_ref closest mode (drift)")


def canon3(words):
    return S.nan_canonical(np.array(words, np.uint32))


@pytest.mark.parametrize("scene", V.HUGE_SCENES)
def test_ray_tri_is_anchored_to_the_reference(loaded, oracle, scene):
    """occlusion_ref.ray_tri and orc_kat_ray_tri against the reference's IntersectRayTri (`refdriver tri`, committed)
    on every (ray, appended triangle) pair: the hit flag on all pairs, t, u, v on the hits."""
    e, rays, rec, keep, ref, sc, gm = loaded(scene)
    want = V.load_huge_tri()[scene]
    on = want[:, 0] == 1
    k = np.full(rays.shape[0], sc.big)
    with np.errstate(all="ignore"):
        h, t, u, v = R.ray_tri(rays[:, :3].copy(), rays[:, 3:].copy(), ref.v0[k], ref.v1[k], ref.v2[k])
    np.testing.assert_array_equal(h, on, err_msg="occlusion_ref.ray_tri: hit")
    mine = np.stack([t, u, v], axis=1).astype(np.float32).view(np.uint32)
    np.testing.assert_array_equal(canon3(mine[on]), canon3(want[on, 1:]), err_msg="occlusion_ref.ray_tri: t, u, v")
    pairs = sc.big_pairs(rays)
    rin = np.concatenate([pairs, np.zeros((pairs.shape[0], 3), np.float32)], axis=1)
    out = oracle.kat("ray_tri", rin, 8).view(np.uint32)
    np.testing.assert_array_equal(out[:, 0], want[:, 0], err_msg="orc_kat_ray_tri: hit")
    np.testing.assert_array_equal(canon3(out[on, 1:4]), canon3(want[on, 1:]), err_msg="orc_kat_ray_tri: t, u, v")
    # every closest hit the records put on the appended triangle is one of these pairs, with these t, u, v
    big = keep & (rec[:, 0] == 1) & (rec[:, 1] == sc.big)
    assert on[big].all()
    np.testing.assert_array_equal(canon3(rec[big, 2:5]), canon3(want[big, 1:]))


# ------------------------------------------------------------------ 5. the interval contract
@pytest.mark.parametrize("scene", V.SCENES)
def test_intervals_around_the_records_t(loaded, scene):
    """test_ray_sets_cpu's interval test on these scenes (tmin = -inf: occluded implies hit && t < tmax; over
    (-inf, +inf): the records' hit; some hits occluded, some not), and the occluded counts the generator recorded."""
    e, rays, rec, keep, ref, sc, gm = loaded(scene)
    T.test_intervals_around_the_reference_t(lambda s: loaded(s)[:5] + (None, loaded(s)[6]), scene)
    occ = R.walk(ref, rays, RS.intervals(rays, rec, ref.diagonal()), mode="any")["occluded"]
    assert int(occ[keep].sum()) == e["occluded"] and int(occ[keep & (rec[:, 0] == 1)].sum()) == e["occluded_hits"]


# ------------------------------------------------------------------ 6. the reference itself, where it is built
@need_ref
def test_drivers_still_write_the_committed_records(loaded, tmp_path):
    usage = subprocess.run([REFDRIVER_INSTR], capture_output=True, text=True, timeout=60).stderr
    if "tri" not in usage:
        pytest.skip("oracle/_ref/refdriver_instr predates the tri command: make -C oracle ref")
    rp, op = str(tmp_path / "in.f32"), str(tmp_path / "out.rec")
    for scene in ("ribbon_x513", "ribbon_z512"):
        e, rays, rec, keep, ref, sc, gm = loaded(scene)
        path = str(tmp_path / (scene + ".rtscene"))
        sc.save(path)
        rays.astype("<f4").tofile(rp)
        subprocess.run([REFDRIVER_INSTR, "rays", path, rp, op, str(V.GRID_RES[scene])], check=True, capture_output=True, timeout=300)
        np.testing.assert_array_equal(np.fromfile(op, "<u4").reshape(-1, 8), rec)
    for scene in V.HUGE_SCENES:
        e, rays, rec, keep, ref, sc, gm = loaded(scene)
        sc.big_pairs(rays).astype("<f4").tofile(rp)
        subprocess.run([REFDRIVER, "tri", rp, op], check=True, capture_output=True, timeout=300)
        np.testing.assert_array_equal(np.fromfile(op, "<u4").reshape(-1, 4), V.load_huge_tri()[scene])


# ------------------------------------------------------------------ 7. the comparisons can fail
def test_one_flipped_word_is_noticed(loaded):
    for scene in ("ribbon_x513", "huge_axis_z"):
        e, rays, rec, keep, ref, sc, gm = loaded(scene)
        row = int(np.flatnonzero(keep & (rec[:, 0] == 1))[7])
        rec12, hits = RS.expected_rec12(rec), RS.expected_hits(rec)
        RS.assert_words(rec12, RS.expected_rec12(rec), (5, 6, 7), keep, "stand-in records")
        for j in range(8):
            bad = rec.copy()
            bad[row, j] ^= 1
            with pytest.raises(AssertionError):
                T.assert_records(rec, bad, keep, "flipped")
            with pytest.raises(AssertionError):
                RS.assert_words(rec12, RS.expected_rec12(bad), (5, 6, 7), keep, "flipped")
            if 1 <= j <= 4:
                with pytest.raises(AssertionError):
                    RS.assert_words(hits, RS.expected_hits(bad), (1, 2, 3), keep, "flipped")
        # a fixture file with one bit flipped no longer has its SHA-256; a mesh with one vertex word flipped neither
        with open(os.path.join(V.DIR, e["rec"]), "rb") as f:
            data = bytearray(f.read())
        data[len(data) // 2] ^= 1
        assert RS.sha256(bytes(data)) != e["rec_sha256"]
        v = sc.v.copy()
        v.view(np.uint32)[v.shape[0] // 2, 1] ^= 1
        assert RS.sha256(np.ascontiguousarray(v, "<f4").tobytes()) != e["mesh"]["vertices_sha256"]
        t = sc.t.copy()
        t[t.shape[0] // 2, 0] ^= 1
        assert RS.sha256(np.ascontiguousarray(t, "<u4").tobytes()) != e["mesh"]["triangles_sha256"]
