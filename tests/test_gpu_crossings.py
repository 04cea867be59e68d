"""rt_crossing_rays_device on the GPU, byte for byte against tests/crossing_ref.py (anchored by tests/test_crossing_cpu.py).

1. The seven scenes of tests/golden/rays (all eight families, 2,744 rays each) and the seven of tests/ray_variant_scenes.py
   (which reach the four instantiations kVarCross | kRaysBase [| kVarFastRcp] [| kRaysBox]; rt_scene_info is asserted),
   in family order and under test_gpu_ray_sets' seeded permutation, each plain and with RT_RAYS_SORT, over d_tminmax =
   NULL, an explicit (-inf, +inf) array and ray_sets.intervals.  The rays rays.json lists as resting on undefined
   behaviour of the reference are left out.  On the same rays and intervals, count >= 1 implies the device's own
   rt_occluded_rays_device.
2. Edges: n = 1, 63, 64, 65, 129; a sentinel past n untouched; waves that mix |d|_inf above and below 8; non-finite
   rays and bad intervals inside otherwise live waves.
3. GpuScene.inside and signed_distance on the closed cube and the 2,048-triangle sphere, 4,096 points: the restatement's
   vote, the analytic inside, and abs(signed) bit-equal to distance().dist.

Bar: bit-exact.  Output buffers carry a 0x5A fill and a 64-record tail.
"""
import ctypes

import numpy as np
import pytest

import crossing_ref as C
import occlusion_ref as R
import ray_sets as RS
import ray_variant_scenes as V
import synth_scenes as S
from conftest import load_package
from test_gpu_occlusion import dev, raw_occluded, stream_of, vp

pytestmark = pytest.mark.gpu
rtm = load_package()
META, VMETA = RS.meta(), V.meta()
INF = np.float32(np.inf)
ORDERS = ("family", "shuffled")
FILL, TAIL = 0x5A5A5A5A, 64
ALL_SCENES = [("rays", s) for s in RS.SCENES] + [("variant", s) for s in V.SCENES]


def raw_cross(torch, gs, d_rays, d_tmm, n=None, flags=0, expect_rc=0):
    """One rt_crossing_rays_device call into a filled buffer with a 64-record tail -> u32 [n, 2] (a rejected call: an
    empty array, after checking that nothing at all was written)."""
    n = d_rays.shape[0] if n is None else n
    out = torch.full((n + TAIL, 2), FILL, dtype=torch.int32, device="cuda")
    rc = rtm.tracer_lib().rt_crossing_rays_device(gs._h, vp(d_rays), vp(d_tmm), n, flags, vp(out),
                                                  ctypes.c_void_p(stream_of(torch)))
    assert rc == expect_rc, (rc, expect_rc)
    torch.cuda.synchronize()
    h = out.cpu().numpy().view(np.uint32)
    written = n if rc == 0 else 0
    assert (h[written:] == FILL).all(), "records written past n"
    assert (h[:written, 1] <= h[:written, 0]).all() and (h[:written, 0] < (1 << 24)).all(), "front > count, or unwritten"
    return h[:written].copy()


def cross(torch, gs, d_rays, d_tmm, n=None):
    """The plain call and the RT_RAYS_SORT call: the same bytes, in input order."""
    plain = raw_cross(torch, gs, d_rays, d_tmm, n=n)
    np.testing.assert_array_equal(raw_cross(torch, gs, d_rays, d_tmm, n=n, flags=rtm.RT_RAYS_SORT), plain,
                                  err_msg="RT_RAYS_SORT vs the plain call")
    return plain


def want_of(sc, rays, tmm):
    r = C.walk_count(sc, rays, tmm)
    return np.stack([r["count"], r["front"]], axis=1).astype(np.uint32)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """Per scene, created once and never changed: the GPU scene, the rays, the pinned mask, the intervals, and the
    restatement's records over (-inf, +inf) and over the intervals."""
    tmp = tmp_path_factory.mktemp("crossings")
    cache, owned = {}, []

    def get(kind, name):
        if (kind, name) not in cache:
            if kind == "rays":
                e = META["scenes"][name]
                rays, rec = RS.load(name)
                hs = rtm.HostScene.load(RS.scene_file(name, tmp))
                owned.append(hs)
                gs = rtm.GpuScene(hs, 0)
                owned.append(gs)
                ref = R.RefScene.from_host(hs)
                assert gs.info()["packed_cells"] == (0 if name == "stack2100" else 1), gs.info()
            else:
                e = VMETA["scenes"][name]
                rays, rec = V.load(name)
                sc = V.Scene(name, tmp)
                owned.append(sc)
                assert sc.mesh_shas() == e["mesh"], f"{name}: the regenerated mesh is not the fixture's"
                gs = rtm.GpuScene(sc.host, 0)
                owned.append(gs)
                V.assert_info(name, gs.info())
                ref = sc.ref
            rays = np.ascontiguousarray(rays)
            tmm = RS.intervals(rays, rec, ref.diagonal())
            cache[(kind, name)] = dict(gs=gs, ref=ref, rays=rays, keep=RS.pinned(e), tmm=tmm, want_inf=want_of(ref, rays, None),
                                       want_tmm=want_of(ref, rays, tmm))
        return cache[(kind, name)]
    yield get
    for o in reversed(owned):
        o.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind,scene", ALL_SCENES)
def test_crossings_match_the_restatement(sets, kind, scene, order):
    import torch
    c = sets(kind, scene)
    gs, n = c["gs"], c["rays"].shape[0]
    idx = np.arange(n) if order == "family" else np.random.Generator(np.random.PCG64(61)).permutation(n)
    keep = c["keep"][idx]
    assert n % 64 != 0
    d_rays = dev(torch, c["rays"][idx])
    what = f"{scene}, {order} order"
    got = cross(torch, gs, d_rays, None)
    np.testing.assert_array_equal(got[keep], c["want_inf"][idx][keep], err_msg=f"{what}: NULL interval")
    inf = dev(torch, np.tile(np.array([-INF, INF], np.float32), (n, 1)))
    np.testing.assert_array_equal(cross(torch, gs, d_rays, inf), got, err_msg=f"{what}: explicit (-inf, +inf) vs NULL")
    d_tmm = dev(torch, c["tmm"][idx])
    got_iv = cross(torch, gs, d_rays, d_tmm)
    np.testing.assert_array_equal(got_iv[keep], c["want_tmm"][idx][keep], err_msg=f"{what}: per-ray intervals")
    # the implication, against the device's own occlusion walk on the same rays and intervals
    for label, g, iv in (("NULL", got, None), ("intervals", got_iv, d_tmm)):
        occ = raw_occluded(torch, gs, d_rays, iv)
        bad = (g[:, 0] >= 1) & (occ == 0)
        assert not bad.any(), (what, label, np.flatnonzero(bad)[:8])
    print(f"{what}: {int((got[keep, 0] > 0).sum())} of {int(keep.sum())} rays count over (-inf, +inf) (most {int(got[keep, 0].max())}, "
          f"front on {int((got[keep, 1] > 0).sum())}), {int((got_iv[keep, 0] > 0).sum())} over the intervals")
    assert (got[keep, 0] > 1).any() and (got[keep, 1] > 0).any() and (got[keep, 1] < got[keep, 0]).any(), what
    assert 0 < int((got_iv[keep, 0] > 0).sum()) < int((got[keep, 0] > 0).sum()), what


# ------------------------------------------------------------------ 2. edges
@pytest.fixture(scope="module")
def inside_scene(sets):
    return sets("rays", "inside")


@pytest.mark.parametrize("n", (1, 63, 64, 65, 129))
def test_small_counts_and_the_sentinel(inside_scene, n):
    import torch
    c = inside_scene
    sel = np.flatnonzero(c["keep"])[:: max(1, int(c["keep"].sum()) // 129)][:129]
    d_rays, d_tmm = dev(torch, c["rays"][sel]), dev(torch, c["tmm"][sel])
    # n below the arrays' length: raw_cross checks that records n .. n + 63 keep their fill
    np.testing.assert_array_equal(cross(torch, c["gs"], d_rays, None, n=n), c["want_inf"][sel][:n])
    np.testing.assert_array_equal(cross(torch, c["gs"], d_rays, d_tmm, n=n), c["want_tmm"][sel][:n])


def test_waves_that_mix_long_and_short_directions(inside_scene):
    """|d|_inf above and below 8 in one wave: the wave's vote takes the division arm for all of its lanes, the
    neighbouring waves the reciprocal arm; the records are the restatement's either way."""
    import torch
    c = inside_scene
    sel = np.flatnonzero(c["keep"])[:320]
    rays = c["rays"][sel].copy()
    scale = np.ones(sel.size, np.float32)
    scale[64:128:3] = 16.0                  # every third lane of the second wave
    scale[200] = 1024.0                     # one lane of the fourth
    scale[256:320] = 0.001                  # a whole wave of short directions
    rays[:, 3:] *= scale[:, None]
    assert (np.abs(rays[64:128, 3:]).max(1) > 8).any() and (np.abs(rays[64:128, 3:]).max(1) <= 8).any()
    sc = c["ref"]
    tmm = np.ascontiguousarray(c["tmm"][sel] / scale[:, None], np.float32)
    got = cross(torch, c["gs"], dev(torch, rays), dev(torch, tmm))
    np.testing.assert_array_equal(got, want_of(sc, rays, tmm))
    np.testing.assert_array_equal(cross(torch, c["gs"], dev(torch, rays), None), want_of(sc, rays, None))
    assert (got[:, 0] > 0).any()


def test_dead_lanes_inside_live_waves(inside_scene):
    """Non-finite rays and bad intervals scattered through live waves give {0, 0} and disturb no neighbour."""
    import torch
    c = inside_scene
    sel = np.flatnonzero(c["keep"])[:200]
    rays = c["rays"][sel].copy()
    tmm = np.tile(np.array([-INF, INF], np.float32), (sel.size, 1))
    base = c["want_inf"][sel]
    assert (base[:, 0] > 0).sum() > 100
    dead = np.zeros(sel.size, bool)
    for j, (k, v) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf), (5, -np.inf))):
        rays[5 + 7 * j, k] = v
        dead[5 + 7 * j] = True
    for j, iv in enumerate(((np.nan, INF), (-INF, np.nan), (np.nan, np.nan), (1.0, 1.0), (2.0, 1.0), (INF, INF), (-INF, -INF),
                            (INF, -INF))):
        tmm[70 + 9 * j] = iv
        dead[70 + 9 * j] = True
    got = cross(torch, c["gs"], dev(torch, rays), dev(torch, tmm))
    assert (got[dead] == 0).all()
    np.testing.assert_array_equal(got[~dead], base[~dead])


# ------------------------------------------------------------------ 3. inside and signed distance
@pytest.fixture(scope="module")
def closed(request):
    cache, owned = {}, []

    def get(name):
        if name not in cache:
            tris = C.cube_tris() if name == "cube" else C.sphere_tris()
            v, t = S.mesh_of(tris)
            hs = rtm.HostScene.from_mesh(v, t, 45.0, np.eye(4, dtype=np.float32).reshape(16), grid_res=16)
            owned.append(hs)
            gs = rtm.GpuScene(hs, 0)
            owned.append(gs)
            pts, inside = C.closed_mesh_points(name, 4096, seed=21)
            ref = R.RefScene.from_host(hs)
            votes = {rule: C.inside_vote(ref, pts, rtm.INSIDE_DIRS, rule) for rule in ("winding", "parity")}
            cache[name] = dict(gs=gs, pts=pts, inside=inside, votes=votes, ref=ref)
        return cache[name]
    yield get
    for o in reversed(owned):
        o.close()


@pytest.mark.parametrize("rule", ("winding", "parity"))
@pytest.mark.parametrize("name", ("cube", "sphere"))
def test_inside_and_signed_distance(closed, name, rule):
    import torch
    c = closed(name)
    gs, pts = c["gs"], c["pts"]
    d_pts = dev(torch, pts)
    got = gs.inside(d_pts, rule=rule)
    assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == (4096,)
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got, c["votes"][rule], err_msg=f"{name} {rule}: the restatement's vote")
    np.testing.assert_array_equal(got, c["inside"], err_msg=f"{name} {rule}: the analytic inside")
    np.testing.assert_array_equal(gs.inside(pts, rule=rule), got, err_msg="numpy input")
    one = np.ascontiguousarray(rtm.INSIDE_DIRS[1:2])
    np.testing.assert_array_equal(gs.inside(d_pts, rule=rule, dirs=one).cpu().numpy(), C.inside_vote(c["ref"], pts, one, rule))
    plain = gs.distance(d_pts, closest=True)
    sd = gs.signed_distance(d_pts, closest=True, rule=rule)
    torch.cuda.synchronize()
    dist, sdist = plain.dist.cpu().numpy(), sd.dist.cpu().numpy()
    np.testing.assert_array_equal(np.abs(sdist).view(np.uint32), dist.view(np.uint32), err_msg="abs(signed) vs distance()")
    np.testing.assert_array_equal(np.signbit(sdist), got)
    assert torch.equal(sd.raw, plain.raw) and torch.equal(sd.closest, plain.closest) and torch.equal(sd.tri, plain.tri)
    h = gs.signed_distance(pts, rule=rule)
    np.testing.assert_array_equal(h.dist.view(np.uint32), sdist.view(np.uint32), err_msg="numpy input")
    assert h.closest is None
