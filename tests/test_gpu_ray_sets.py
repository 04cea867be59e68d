"""Every ray path on the GPU against the REFERENCE, on rays that no camera makes.

tests/golden/rays (oracle/gen_golden_rays.py; the families are described in tests/ray_sets.py) holds about 2,700 rays
per scene and the records the reference's own Grid::Intersect wrote for them.  Per scene, in family order (a wave
holds one family) and again under a seeded permutation of the whole set (a wave holds any mix):

1. rt_trace_rays_device with RT_RAYS_COUNT: all eight geometric record columns are the reference's, colour and pad are
   0, and d_hits holds the records' tri, t, u, v;
2. the fast arm: tri, t, u, v are the reference's, a miss is 0xFFFFFFFF, 0, 0, 0;
3. RT_RAYS_SORT with either arm: the same bits, in input order;
4. rt_occluded_rays_device over the infinite interval -- d_tminmax = NULL, an explicit (-inf, +inf) array, and each
   again with RT_RAYS_SORT -- is the reference's hit;
5. over per-ray intervals around the reference's own t (ray_sets.intervals) it is tests/occlusion_ref.py's any-hit
   walk, which tests/test_ray_sets_cpu.py pins to the reference on these very rays; and, independently of that
   restatement, every occluded byte with tmin = -inf has ref.hit && ref.t < tmax (include/rt_tracer.h).

Bar: bit-exact (a NaN equals any NaN).  The output buffers carry sentinels and 64-element tails (raw_trace of
tests/test_gpu_rays.py, occl of tests/test_gpu_occlusion.py).  Only the rays rays.json lists as resting on undefined
behaviour of the reference are left out of the comparisons with it.  stack2100 (packed_cells == 0) walks the plain
CSR ranges, the other scenes the box runs.
"""
import numpy as np
import pytest

import occlusion_ref as R
import ray_sets as RS
from conftest import load_package
from test_gpu_occlusion import dev, occl
from test_gpu_rays import check_sorted, hits_as_rec12, raw_trace

pytestmark = pytest.mark.gpu
rtm = load_package()
META = RS.meta()
INF = np.float32(np.inf)
ORDERS = ("family", "shuffled")
REC_FLOATS, HIT_FLOATS = (5, 6, 7), (1, 2, 3)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """Per scene, loaded once: the GPU scene, the fixture, the intervals and the restatement's bytes for them."""
    tmp = tmp_path_factory.mktemp("raysets")
    cache = {}

    def get(scene):
        if scene not in cache:
            e = META["scenes"][scene]
            rays, rec = RS.load(scene)
            hs = rtm.HostScene.load(RS.scene_file(scene, tmp))
            gs = rtm.GpuScene(hs, 0)
            sc = R.RefScene.from_host(hs)
            tmm = RS.intervals(rays, rec, sc.diagonal())
            want = R.walk(sc, rays, tmm, mode="any")["occluded"].astype(np.uint8)
            cache[scene] = dict(e=e, rays=np.ascontiguousarray(rays), rec=rec, keep=RS.pinned(e), hs=hs, gs=gs, tmm=tmm,
                                want=want)
        return cache[scene]
    yield get
    for c in cache.values():
        c["gs"].close()
        c["hs"].close()


def ordered(c, order):
    """(index array, rays, records, pinned mask, intervals, the restatement's bytes) in the given order."""
    n = c["rays"].shape[0]
    idx = np.arange(n) if order == "family" else np.random.Generator(np.random.PCG64(61)).permutation(n)
    return idx, np.ascontiguousarray(c["rays"][idx]), c["rec"][idx], c["keep"][idx], np.ascontiguousarray(c["tmm"][idx]), c["want"][idx]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("scene", RS.SCENES)
def test_closest_hit_arms_match_the_reference(sets, scene, order):
    import torch
    c = sets(scene)
    gs = c["gs"]
    assert gs.info()["packed_cells"] == (0 if scene == "stack2100" else 1), gs.info()
    idx, rays, rec, keep, tmm, want = ordered(c, order)
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
    assert int((~miss & keep).sum()) == sum(v[0] for v in c["e"]["counts"].values())
    check_sorted(torch, gs, d_rays, hf, rc)
    np.testing.assert_array_equal(hf, hc, err_msg=f"{what}: fast arm vs counting arm")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("scene", RS.SCENES)
def test_occlusion_matches_the_reference(sets, scene, order):
    import torch
    c = sets(scene)
    gs = c["gs"]
    idx, rays, rec, keep, tmm, want = ordered(c, order)
    n = rays.shape[0]
    d_rays = dev(torch, rays)
    what = f"{scene}, {order} order"
    ref_hit = (rec[:, 0] == 1).astype(np.uint8)
    # 4. the infinite interval: NULL and explicit, each plain and sorted (occl)
    got = occl(torch, gs, d_rays, None)
    np.testing.assert_array_equal(got[keep], ref_hit[keep], err_msg=f"{what}: NULL interval vs the reference's hit")
    inf = dev(torch, np.tile(np.array([-INF, INF], np.float32), (n, 1)))
    np.testing.assert_array_equal(occl(torch, gs, d_rays, inf), got, err_msg=f"{what}: explicit (-inf, +inf) vs NULL")
    # 5. intervals around the reference's t
    got = occl(torch, gs, d_rays, dev(torch, tmm))
    np.testing.assert_array_equal(got[keep], want[keep], err_msg=f"{what}: intervals vs the restatement")
    t = rec[:, 2].view(np.float32)
    open_below = keep & (tmm[:, 0] == -INF)
    implied = (ref_hit == 1) & (t < tmm[:, 1])
    assert not ((got == 1) & open_below & ~implied).any(), (what, np.flatnonzero((got == 1) & open_below & ~implied)[:8])
    whole = open_below & (tmm[:, 1] == INF)
    np.testing.assert_array_equal(got[whole], ref_hit[whole], err_msg=f"{what}: rays whose interval is (-inf, +inf)")
    hits = keep & (ref_hit == 1)
    print(f"{what}: {int(got[keep].sum())} of {int(keep.sum())} occluded over the intervals, {int(hits.sum())} reference hits, "
          f"{int((~keep).sum())} rays not pinned")
    assert whole.sum() >= 100 and 0 < int(got[hits].sum()) < int(hits.sum())
