"""The ray, occlusion and AO kernels on every scene-dependent instantiation, against the REFERENCE.

rt_trace_rays_device, rt_occluded_rays_device and rt_render_ao_device each ship four instantiations
(kRaysBase [| kVarFastRcp] [| kRaysBox], scene_traversal_bits in rt_launch.hip).  The scenes of tests/test_gpu_ray_sets.py
all run the first (stack2100: the third).  The seven scenes of tests/ray_variant_scenes.py reach the others, and what
only they reach inside the walk:

  ribbon_[xyz]513  kRaysBase | kVarFastRcp over cell words without box runs: the distance-skip loop of grid_intersect
                   with kVarAnyHit (its own copy of rule 3 while skip > 0, per-lane oct_offset, RT_DDA_ADVANCE_ADD), the
                   fast closest-hit arm on that walk, and RT_RAYS_SORT with shift = 1 (an axis of 513 cells)
  ribbon_z512      the packable side: box runs at the 9-bit z count of a box word, shift = 0
  sheets16         the same variant as the 513 ribbons; cell words whose 21-bit start field holds 2^20 and more
  huge_axis_z      kRaysBase | kRaysBox: the exact reciprocal inside the per-lane box-run walk; accepted hits whose u and v
                   are not finite pass the wave-gated det / u half of ray_tri_mt_gated
  huge_stack2100   kRaysBase: the exact reciprocal over the plain CSR walk

rt_scene_info is asserted when a scene is created, before anything is compared: the variant is a pure function of it.
One test per (scene, call family, order) -- family order (a wave holds one family) and test_gpu_ray_sets' seeded
permutation -- so that a fault can be attributed to one instantiation; each scene is created once per module.

Expected: tests/golden/ray_variants (oracle/gen_golden_ray_variants.py) -- the reference's own Grid::Intersect at the
scene's grid resolution for the ribbons and sheets16; for the huge scenes tests/occlusion_ref.py's walk, whose
ray/triangle half tests/test_ray_variants_cpu.py anchors to the reference's IntersectRayTri.  Occlusion over
ray_sets.intervals: occlusion_ref's any-hit walk.  AO: the composition of tests/test_gpu_ao.py.
Bar: bit-exact (a NaN equals any NaN in a float column).  Buffers carry sentinels and 64-element tails (raw_trace, occl,
raw_ao).
"""
import numpy as np
import pytest

import occlusion_ref as R
import ray_sets as RS
import ray_variant_scenes as V
from conftest import load_package
from test_gpu_ao import AoScene, check as check_ao
from test_gpu_occlusion import dev, occl
from test_gpu_ray_sets import HIT_FLOATS, ORDERS, REC_FLOATS
from test_gpu_rays import check_sorted, hits_as_rec12, raw_trace

pytestmark = pytest.mark.gpu
rtm = load_package()
META = V.meta()
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """Per scene, created once: the regenerated scene (mesh SHA-256s checked: a mismatch fails), its GPU copy
    (rt_scene_info checked), the fixture, the intervals and the restatement's bytes for them."""
    tmp = tmp_path_factory.mktemp("rayvariants")
    cache = {}

    def get(name):
        if name not in cache:
            e = META["scenes"][name]
            rays, rec = V.load(name)
            sc = V.Scene(name, tmp)
            assert sc.mesh_shas() == e["mesh"], f"{name}: the regenerated mesh is not the fixture's"
            sc.check_static()
            gs = rtm.GpuScene(sc.host, 0)
            cache[name] = c = dict(e=e, rays=np.ascontiguousarray(rays), rec=rec, keep=RS.pinned(e), sc=sc, gs=gs)
            c["info"] = V.assert_info(name, gs.info())
            c["tmm"] = RS.intervals(rays, rec, sc.ref.diagonal())
            c["want"] = R.walk(sc.ref, rays, c["tmm"], mode="any")["occluded"].astype(np.uint8)
            c["ao"] = AoScene(name, sc.host, gs, sc.ref)
        c = cache[name]
        assert "want" in c, f"{name}: the scene's creation failed in an earlier test"
        return c
    yield get
    for c in cache.values():
        c["gs"].close()
        c["sc"].close()


def ordered(c, order):
    """(rays, records, pinned mask, intervals, the restatement's bytes) in the given order."""
    n = c["rays"].shape[0]
    idx = np.arange(n) if order == "family" else np.random.Generator(np.random.PCG64(61)).permutation(n)
    return np.ascontiguousarray(c["rays"][idx]), c["rec"][idx], c["keep"][idx], np.ascontiguousarray(c["tmm"][idx]), c["want"][idx]


# ------------------------------------------------------------------ closest hit
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("scene", V.SCENES)
def test_closest_hit_arms_match_the_reference(sets, scene, order):
    """The counting arm's 12-word records and d_hits, the fast arm's tri, t, u, v (a miss: 0xFFFFFFFF, 0, 0, 0), the
    fast arm against the counting arm on every ray, and RT_RAYS_SORT with either arm: the same bits in input order."""
    import torch
    c = sets(scene)
    gs = c["gs"]
    rays, rec, keep, tmm, want = ordered(c, order)
    assert rays.shape[0] % 64 != 0
    d_rays = dev(torch, rays)
    what = f"{scene}, {order} order"
    hc, rc = raw_trace(torch, gs, d_rays, True)
    RS.assert_words(rc, RS.expected_rec12(rec), REC_FLOATS, keep, f"{what}: counting arm records")
    RS.assert_words(hc, RS.expected_hits(rec), HIT_FLOATS, keep, f"{what}: counting arm hits")
    np.testing.assert_array_equal(hits_as_rec12(hc)[:, [0, 1, 5, 6, 7]], rc[:, [0, 1, 5, 6, 7]], err_msg=f"{what}: d_hits vs d_recs")
    assert (rc[:, 8:] == 0).all(), what
    hf, _ = raw_trace(torch, gs, d_rays, False)
    RS.assert_words(hf, RS.expected_hits(rec), HIT_FLOATS, keep, f"{what}: fast arm")
    miss = hf[:, 0] == RS.NOTRI
    assert (hf[miss, 1:] == 0).all(), what
    hits = int((~miss & keep).sum())
    assert hits == sum(v[0] for v in c["e"]["counts"].values())
    check_sorted(torch, gs, d_rays, hf, rc)
    np.testing.assert_array_equal(hf, hc, err_msg=f"{what}: fast arm vs counting arm")
    print(f"{what}: {hits} hits, {int((miss & keep).sum())} misses, {int((~keep).sum())} rays not pinned, "
          f"longest walk {int(rc[keep, 3].max())} cells")
    if scene == "sheets16":            # the walk read cell words whose start field holds 2^20 and more
        high = c["sc"].ref.offs[rc[keep & ~miss, 2]] >= (1 << 20)
        assert high.sum() >= 32, int(high.sum())
    if scene in V.HUGE_SCENES:         # closest hits on the appended triangle, some with a non-finite u or v
        big = keep & (hf[:, 0] == c["sc"].big)
        odd = big & ~np.isfinite(hf[:, 2:].view(np.float32)).all(1)
        print(f"{what}: {int(big.sum())} closest hits on the appended triangle, {int(odd.sum())} with a non-finite u or v")
        assert big.sum() >= V.MIN_BIG_TRI_HITS and odd.sum() == c["e"]["nonfinite_uv_records"] >= 1


@pytest.mark.parametrize("n", [1, 65])
def test_sorted_prefixes_on_a_513_cell_axis(sets, n):
    """RT_RAYS_SORT with shift = 1 on the first ray alone and on the first 65 (one whole wave and one lane)."""
    import torch
    c = sets("ribbon_x513")
    gs = c["gs"]
    d_rays = dev(torch, c["rays"])
    hf, _ = raw_trace(torch, gs, d_rays, False, n=n)
    hc, rc = raw_trace(torch, gs, d_rays, True, n=n)
    keep = c["keep"][:n]
    RS.assert_words(rc, RS.expected_rec12(c["rec"][:n]), REC_FLOATS, keep, f"first {n} rays: counting arm records")
    RS.assert_words(hf, RS.expected_hits(c["rec"][:n]), HIT_FLOATS, keep, f"first {n} rays: fast arm")
    check_sorted(torch, gs, d_rays, hf, rc, n=n)


# ------------------------------------------------------------------ occlusion
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("scene", V.SCENES)
def test_occlusion_matches_the_reference(sets, scene, order):
    """A NULL interval and an explicit (-inf, +inf) array: the records' hit.  ray_sets.intervals: occlusion_ref's
    any-hit walk, and with tmin = -inf every occluded byte has hit && t < tmax.  Each plain and with RT_RAYS_SORT (occl)."""
    import torch
    c = sets(scene)
    gs = c["gs"]
    rays, rec, keep, tmm, want = ordered(c, order)
    n = rays.shape[0]
    d_rays = dev(torch, rays)
    what = f"{scene}, {order} order"
    ref_hit = (rec[:, 0] == 1).astype(np.uint8)
    got = occl(torch, gs, d_rays, None)
    np.testing.assert_array_equal(got[keep], ref_hit[keep], err_msg=f"{what}: NULL interval vs the records' hit")
    inf = dev(torch, np.tile(np.array([-INF, INF], np.float32), (n, 1)))
    np.testing.assert_array_equal(occl(torch, gs, d_rays, inf), got, err_msg=f"{what}: explicit (-inf, +inf) vs NULL")
    got = occl(torch, gs, d_rays, dev(torch, tmm))
    np.testing.assert_array_equal(got[keep], want[keep], err_msg=f"{what}: intervals vs the restatement")
    t = rec[:, 2].view(np.float32)
    open_below = keep & (tmm[:, 0] == -INF)
    implied = (ref_hit == 1) & (t < tmm[:, 1])
    assert not ((got == 1) & open_below & ~implied).any(), (what, np.flatnonzero((got == 1) & open_below & ~implied)[:8])
    whole = open_below & (tmm[:, 1] == INF)
    np.testing.assert_array_equal(got[whole], ref_hit[whole], err_msg=f"{what}: rays whose interval is (-inf, +inf)")
    hits = keep & (ref_hit == 1)
    print(f"{what}: {int(got[keep].sum())} of {int(keep.sum())} occluded over the intervals, {int(hits.sum())} hits, "
          f"{int((~keep).sum())} rays not pinned")
    assert int(got[keep].sum()) == c["e"]["occluded"]
    assert whole.sum() >= 100 and 0 < int(got[hits].sum()) < int(hits.sum())


# ------------------------------------------------------------------ AO
@pytest.mark.parametrize("scene", V.SCENES)
def test_ao_frame_is_the_composition(sets, scene):
    """rt_render_ao_device on a 62 x 46 x 4 frame of the scene's camera against the composition of tests/test_gpu_ao.py
    (counts byte for byte, pixels word for word, and the pixels again with d_counts NULL): K = 4, rotated, over
    (1e-4, 0.25) diagonals, and K = 5, unrotated, over (0, +inf)."""
    import torch
    c = sets(scene)
    W, H, spp = V.AO_FRAME
    d = c["sc"].ref.diagonal()
    f, occ1 = check_ao(torch, c["ao"], W, H, spp, 4, True, np.float32(1e-4) * d, np.float32(0.25) * d)
    f, occ2 = check_ao(torch, c["ao"], W, H, spp, 5, False, np.float32(0), INF)
    hit = int(f["hit"].sum())
    occluded, rays = int(occ1.sum()) + int(occ2.sum()), occ1.size + occ2.size
    print(f"{scene}: {hit} hit samples; occluded {int(occ1.sum())} of {occ1.size} (K = 4) and {int(occ2.sum())} of {occ2.size} (K = 5)")
    assert hit >= 16
    assert 0 < occluded < rays
