"""rt_distance_points_device (GpuScene.distance) on the GPU: dist bits, tri and the closest-point identity against
tests/distance_ref.py (the oracle's DistancePointTri for every (point, triangle) pair, the reference's loop, the
lowest-index rule).  No point is excluded from any comparison.

Every call goes through the C ABI into buffers pre-filled with a sentinel that carry 64 records past n, which must
still hold the sentinel afterwards; every case runs the default arm, RT_DIST_SORT, RT_DIST_EXHAUSTIVE and both flags,
and all four must give the reference's bytes.
"""
import ctypes

import numpy as np
import pytest

import distance_ref as D
import synth_scenes as S
from conftest import load_package

pytestmark = pytest.mark.gpu
rtm = load_package()
NOTRI = D.NOTRI
FLT_MAX = D.FLT_MAX
TAIL = 64
SENT = 0x5A5A5A5A
ARMS = {"default": 0, "sort": rtm.RT_DIST_SORT, "exhaustive": rtm.RT_DIST_EXHAUSTIVE,
        "sort|exhaustive": rtm.RT_DIST_SORT | rtm.RT_DIST_EXHAUSTIVE}


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def raw_distance(torch, gs, d_pts, n=None, flags=0, closest=True, expect_rc=0, stream=None):
    """One rt_distance_points_device call into sentinel-filled buffers with a 64-record tail -> (records
    POINT_DIST_DTYPE [n], closest f32 [n, 3] or None); nothing may be written past n (nor at all by a rejected call)."""
    n = d_pts.shape[0] if n is None else n
    out = torch.full((n + TAIL, 2), SENT, dtype=torch.int32, device="cuda")
    cl = torch.full((n + TAIL, 3), SENT, dtype=torch.int32, device="cuda") if closest else None
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc = rtm.tracer_lib().rt_distance_points_device(gs._h, vp(d_pts), n, flags, vp(out), vp(cl), ctypes.c_void_p(st))
    assert rc == expect_rc, (rc, expect_rc)
    torch.cuda.synchronize()
    written = n if rc == 0 else 0
    h = out.cpu().numpy().view(np.uint32)
    assert (h[written:] == SENT).all(), "records written past n"
    q = None
    if closest:
        c = cl.cpu().numpy().view(np.uint32)
        assert (c[written:] == SENT).all(), "closest points written past n"
        q = c[:written].view(np.float32).copy()
    return h[:written].copy().view(rtm.POINT_DIST_DTYPE).reshape(written), q


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def check_against(pts, rec, q, want_dist, want_tri, what):
    bad = np.flatnonzero(rec["dist"].view(np.uint32) != want_dist.view(np.uint32))
    assert bad.size == 0, (what, "dist", bad[:8], pts[bad[:8]], rec["dist"][bad[:8]], want_dist[bad[:8]])
    bad = np.flatnonzero(rec["tri"] != want_tri)
    assert bad.size == 0, (what, "tri", bad[:8], pts[bad[:8]], rec["tri"][bad[:8]], want_tri[bad[:8]])
    none = rec["tri"] == NOTRI
    assert (rec["dist"][none] == FLT_MAX).all() and (q[none].view(np.uint32) == 0).all(), (what, "no triangle")
    ident = D.closest_identity(pts, q)
    bad = np.flatnonzero(~none & (ident.view(np.uint32) != rec["dist"].view(np.uint32)))
    assert bad.size == 0, (what, "closest", bad[:8], pts[bad[:8]], q[bad[:8]], ident[bad[:8]], rec["dist"][bad[:8]])


def check_all_arms(torch, oracle, gs, tris, pts, what):
    """The four arms against the reference; returns the reference's (dist, tri)."""
    pts = np.ascontiguousarray(pts, np.float32)
    want_dist, want_tri = D.reference(oracle, pts, tris)
    d_pts = dev(torch, pts)
    for arm, flags in ARMS.items():
        rec, q = raw_distance(torch, gs, d_pts, flags=flags)
        check_against(pts, rec, q, want_dist, want_tri, f"{what} [{arm}]")
    # without d_closest: the same records
    rec, _ = raw_distance(torch, gs, d_pts, closest=False)
    assert (rec["dist"].view(np.uint32) == want_dist.view(np.uint32)).all() and (rec["tri"] == want_tri).all()
    return want_dist, want_tri


@pytest.fixture(scope="module")
def scenes():
    """Per key: (HostScene, GpuScene, triangle corners f32 [nt, 3, 3]), made once.  A key is a shipped scene's number
    or a (name, mesh) pair built with HostScene.from_mesh on a coarse grid (the grid plays no part here)."""
    cache = {}

    def get(key, tris=None):
        if key not in cache:
            if tris is None:
                hs = rtm.HostScene.load(key)
            else:
                v, t = S.mesh_of(tris)
                hs = rtm.HostScene.from_mesh(v, t, 45.0, S.axis_cam(2, -1, (0.0, 0.0, 3.0)), grid_res=8)
            v, t = hs.mesh()
            cache[key] = (hs, rtm.GpuScene(hs, 0), D.triangles_of(v, t))
        return cache[key]
    yield get
    for hs, gs, _ in cache.values():
        gs.close()
        hs.close()


# ------------------------------------------------------------------ the shipped scenes
@pytest.mark.parametrize("sid", [1, 8])
def test_shipped_scenes_five_families(oracle, scenes, sid):
    """Scene 1 (two blocks, no upper level) and scene 8 (24,336 triangles, 761 blocks, two levels): 512 points, about
    100 of each family."""
    import torch
    hs, gs, tris = scenes(sid)
    assert tris.shape[0] == {1: 44, 8: 24336}[sid]
    pts = np.concatenate([D.families(tris, 102, 100 + sid), D.families(tris, 1, 200 + sid)[:2]])
    assert pts.shape == (512, 3)
    dist, tri = check_all_arms(torch, oracle, gs, tris, pts, f"scene{sid}")
    assert (tri != NOTRI).all()
    print(f"scene{sid}: {tris.shape[0]} triangles, dist {dist.min():.3g} .. {dist.max():.3g}")


# ------------------------------------------------------------------ the hierarchy's edges
@pytest.mark.parametrize("K", [3, 31, 32, 33, 64, 65, 1023, 1024, 1025, 32767, 32768, 32769])
def test_hierarchy_edges(oracle, scenes, K):
    """synth_scenes.sparse(seed, n = K - 2) has K triangles: one short of, at and one past 32^k at every level, and 64 /
    65, the last mesh whose default arm is the exhaustive kernel and the first that is culled."""
    import torch
    hs, gs, tris = scenes(("sparse", K), S.sparse(300 + K, n=K - 2))
    assert tris.shape[0] == K
    pts = np.concatenate([D.families(tris, 12, K), D.families(tris, 1, K + 1)[:4]])
    assert pts.shape == (64, 3)
    check_all_arms(torch, oracle, gs, tris, pts, f"sparse K = {K}")


# ------------------------------------------------------------------ a degenerate mesh
def test_degenerate_mesh_and_duplicate_pairs(oracle, scenes):
    """synth_scenes.degenerate(28): collinear triangles, point triangles (NaN distances) and exact duplicates.  Points
    on its vertices, on its edge midpoints, at the duplicated triangles' centroids and at random: tri is never the
    higher index of a duplicated pair."""
    import torch
    mesh = S.degenerate(28)
    hs, gs, tris = scenes(("degenerate", 28), mesh)
    np.testing.assert_array_equal(tris, mesh)
    dup_hi = np.array([40 + 3 * m + 2 for m in range(8)])
    dup_lo = np.array([3 * m for m in range(8)])
    np.testing.assert_array_equal(tris[dup_hi], tris[dup_lo])
    r = np.random.Generator(np.random.PCG64(5))
    mids = ((tris + np.roll(tris, 1, axis=1)) * np.float32(0.5)).reshape(-1, 3)
    cents = ((tris[dup_lo, 0] + tris[dup_lo, 1] + tris[dup_lo, 2]) / np.float32(3)).astype(np.float32)
    pts = np.concatenate([tris.reshape(-1, 3), mids, cents, r.uniform(-1.2, 1.2, (200, 3)).astype(np.float32)])
    dist, tri = check_all_arms(torch, oracle, gs, tris, pts, "degenerate")
    assert not np.isin(tri, dup_hi).any()
    assert np.isin(tri, dup_lo).sum() >= 8                 # the pairs are reached


# ------------------------------------------------------------------ non-finite and extreme points
@pytest.mark.parametrize("sid", [1, 8])
def test_non_finite_and_extreme_points(oracle, scenes, sid):
    import torch
    hs, gs, tris = scenes(sid)
    base = tris.reshape(-1, 3).mean(0).astype(np.float32)
    vals = [np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-40, -1e-40, 1.4e-45, 0.0, -0.0, 1e19, -2e19]
    pts = []
    for v in vals:
        for c in range(3):
            p = base.copy()
            p[c] = v
            pts.append(p)
        pts.append(np.full(3, v, np.float32))
    pts.append(np.array([np.nan, np.inf, -np.inf], np.float32))
    pts.append(np.array([3e38, -3e38, 1e-40], np.float32))
    pts = np.array(pts, np.float32)
    dist, tri = check_all_arms(torch, oracle, gs, tris, pts, f"scene{sid} extremes")
    assert not np.isnan(dist).any()
    nonfin = ~np.isfinite(pts).all(1)
    assert (dist[nonfin] == FLT_MAX).all() and (tri[nonfin] == NOTRI).all()


# ------------------------------------------------------------------ point counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_point_counts_and_canaries(oracle, scenes, n):
    import torch
    hs, gs, tris = scenes(("sparse", 1025), S.sparse(300 + 1025, n=1023))          # culled, two levels
    pts = D.families(tris, 820, 9)[np.random.Generator(np.random.PCG64(n)).permutation(4100)[:n]]
    if n == 0:
        d_pts = torch.zeros((1, 3), dtype=torch.float32, device="cuda")
        for flags in ARMS.values():
            rec, q = raw_distance(torch, gs, d_pts, n=0, flags=flags)
            assert rec.size == 0 and q.size == 0
        res = gs.distance(np.zeros((0, 3), np.float32), closest=True)
        assert res.dist.shape == (0,) and res.tri.shape == (0,) and res.closest.shape == (0, 3)
        return
    check_all_arms(torch, oracle, gs, tris, pts, f"n = {n}")


# ------------------------------------------------------------------ arguments and the Python layer
def test_c_abi_argument_errors_write_nothing(scenes):
    import torch
    hs, gs, tris = scenes(1)
    L = rtm.tracer_lib()
    d_pts = torch.zeros((8, 3), dtype=torch.float32, device="cuda")
    for flags in (4, 0x10, 0x80000000, 1 | 2 | 4):
        raw_distance(torch, gs, d_pts, flags=flags, expect_rc=1)
    out = torch.full((16, 2), SENT, dtype=torch.int32, device="cuda")
    cl = torch.full((16, 3), SENT, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, o, c = d_pts.data_ptr(), out.data_ptr(), cl.data_ptr()

    def call(scene, pp, n, oo, cc):
        return L.rt_distance_points_device(scene, ctypes.c_void_p(pp), n, 0, ctypes.c_void_p(oo), ctypes.c_void_p(cc), st)

    assert call(None, p, 8, o, c) == 1                         # a NULL scene, d_points, d_out
    assert call(gs._h, None, 8, o, c) == 1
    assert call(gs._h, p, 8, None, c) == 1
    assert call(gs._h, p + 2, 4, o, c) == 1                    # d_points, d_closest off 4 bytes; d_out off 8
    assert call(gs._h, p, 4, o, c + 1) == 1
    assert call(gs._h, p, 4, o + 4, c) == 1
    assert call(gs._h, p, 0x80000000, o, c) == 1               # n >= 2^31
    assert call(gs._h, p, 0, None, None) == 0                  # n == 0: RT_OK, nothing looked at
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENT).all() and (cl.cpu().numpy().view(np.uint32) == SENT).all()


def test_python_layer(oracle, scenes):
    """numpy in -> numpy out, torch in -> torch out (in place), the flags, and every refused input."""
    import torch
    hs, gs, tris = scenes(1)
    pts = D.families(tris, 8, 3)
    want_dist, want_tri = D.reference(oracle, pts, tris)
    for kw in ({}, {"sort": True}, {"exhaustive": True}, {"closest": True}, {"closest": True, "sort": True, "exhaustive": True}):
        res = gs.distance(pts, **kw)
        assert isinstance(res.dist, np.ndarray) and res.dist.dtype == np.float32 and res.tri.dtype == np.uint32
        assert res.raw.dtype == rtm.POINT_DIST_DTYPE
        assert (res.dist.view(np.uint32) == want_dist.view(np.uint32)).all() and (res.tri == want_tri).all()
        assert (res.closest is None) == (not kw.get("closest"))
        if res.closest is not None:
            assert (D.closest_identity(pts, res.closest).view(np.uint32) == want_dist.view(np.uint32)).all()
        d_pts = dev(torch, pts)
        res = gs.distance(d_pts, **kw)
        torch.cuda.synchronize()
        assert isinstance(res.dist, torch.Tensor) and res.dist.is_cuda and res.dist.dtype == torch.float32
        assert (res.dist.cpu().numpy().view(np.uint32) == want_dist.view(np.uint32)).all()
        assert (res.tri.cpu().numpy().view(np.uint32) == want_tri).all()
        assert tuple(res.raw.shape) == (pts.shape[0], 2)
        if kw.get("closest"):
            assert tuple(res.closest.shape) == (pts.shape[0], 3) and res.closest.dtype == torch.float32
    s = torch.cuda.Stream()
    d_pts = dev(torch, pts)
    torch.cuda.synchronize()
    res = gs.distance(d_pts, closest=True, stream=s.cuda_stream)
    s.synchronize()
    assert (res.dist.cpu().numpy().view(np.uint32) == want_dist.view(np.uint32)).all()
    good = torch.zeros((6, 3), dtype=torch.float32, device="cuda")
    for bad in (good.double(), good.half(), good.reshape(-1), good[:, :2], torch.zeros((6, 4), device="cuda"),
                torch.zeros((6, 6), device="cuda")[:, :3], good[::2], good.cpu(), good.cpu().numpy().astype(np.float64),
                good.cpu().numpy()[::2], good.cpu().numpy().reshape(-1), [[0.0, 0.0, 0.0]], None):
        with pytest.raises(ValueError):
            gs.distance(bad)


# ------------------------------------------------------------------ graph capture
def test_graph_capture_and_replay(oracle, scenes):
    """One warm-up call, the call (no RT_DIST_SORT) captured in a graph, two replays into cleared buffers: the same
    bytes each time."""
    import torch
    hs, gs, tris = scenes(8)
    pts = D.families(tris, 26, 77)
    want_dist, want_tri = D.reference(oracle, pts, tris)
    n = pts.shape[0]
    d_pts = dev(torch, pts)
    out = torch.full((n + TAIL, 2), SENT, dtype=torch.int32, device="cuda")
    cl = torch.full((n + TAIL, 3), SENT, dtype=torch.int32, device="cuda")
    L = rtm.tracer_lib()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert L.rt_distance_points_device(gs._h, vp(d_pts), n, 0, vp(out), vp(cl), ctypes.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    first = out.cpu().numpy().copy(), cl.cpu().numpy().copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assert L.rt_distance_points_device(gs._h, vp(d_pts), n, 0, vp(out), vp(cl), ctypes.c_void_p(s.cuda_stream)) == 0
    for _ in range(2):
        out.fill_(SENT)
        cl.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), first[0])
        np.testing.assert_array_equal(cl.cpu().numpy(), first[1])
    rec = first[0][:n].view(np.uint32).copy().view(rtm.POINT_DIST_DTYPE).reshape(n)
    check_against(pts, rec, first[1][:n].view(np.uint32).view(np.float32), want_dist, want_tri, "graph")


# ------------------------------------------------------------------ isolation
def test_frames_around_a_distance_call_are_identical(scenes):
    import torch
    hs, gs, tris = scenes(8)
    f = gs.frame(160, 90, 2)
    before = gs.render_frame(f).copy()
    pts = D.families(tris, 40, 1)
    for kw in ({}, {"sort": True}, {"exhaustive": True, "closest": True}):
        gs.distance(pts, **kw)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(gs.render_frame(f), before)
    fm = gs.frame(64, 36, 1)
    fm.intersector = rtm.RT_ISECT_RAY_MARCH
    march = gs.render_frame(fm).copy()
    gs.distance(pts, sort=True)
    np.testing.assert_array_equal(gs.render_frame(fm), march)
