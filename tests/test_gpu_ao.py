"""rt_render_ao_device (GpuScene.render_ao) on the GPU, held to the composition it fuses, with no tolerance:

    gs.primary_rays -> gs.trace_rays -> ao_ref.form (numpy) -> gs.occluded over (tmin, tmax) -> ao_ref.counts / pixels

The three library calls are pinned to the reference by tests/test_gpu_rays.py and tests/test_gpu_occlusion.py;
tests/ao_ref.py restates the few operations in between, one numpy operation per operation of the contract
(include/rt_tracer.h), and tests/test_ao_cpu.py checks its invariants, its known answers and that the views used here
are not vacuous.  d_counts is compared byte for byte and d_bgra word for word.  Both buffers are pre-filled with
0x5A and carry a tail, which must still hold 0x5A afterwards.
"""
import ctypes

import numpy as np
import pytest

import ao_ref as A
import occlusion_ref as R
import synth_scenes as S
from conftest import load_package

pytestmark = pytest.mark.gpu
rtm = load_package()
META = S.meta()
NOTRI = 0xFFFFFFFF
TAIL = 64
FILL = 0x5A
INF = np.float32(np.inf)
# (flat_front is the one view below the 2 % floor of occluded AO rays that tests/test_ao_cpu.py holds the others to,
# 1.89 %: flat_inplane, the same mesh seen along its plane, stands for it there; here it is rendered all the same)
VIEWS = ("inside", "stack1500", "stack2100", "degenerate", "zero_normals", "negative_octant", "scale_1500", "away",
         "flat_inplane")
EXTRA_VIEWS = ("flat_front",)
SCENE_VIEWS = {"scene1": (96, 54, 4), "scene8": (96, 54, 4)}


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ao_struct(K, tmin, tmax, dirs, rotate):
    d = np.ascontiguousarray(dirs, np.float32) if dirs is not None else None
    p = rtm.AoParams(K, float(tmin), float(tmax), d.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if d is not None else None,
                     rtm.RT_AO_ROTATE if rotate else 0)
    return p, d


def raw_ao(torch, gs, f, K, tmin, tmax, dirs=None, rotate=True, want_counts=True, stream=None, expect_rc=0, flags=None):
    """One rt_render_ao_device call into 0x5A-filled buffers with tails -> (pixels u32 [H, W], counts u8 [H, W, spp] or
    None); a rejected call: (None, None) after checking that nothing at all was written."""
    W, H, spp = f.width, f.height, max(1, f.spp)
    bgra = torch.full((W * H + TAIL,), S.SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((W * H * spp + TAIL,), FILL, dtype=torch.uint8, device="cuda") if want_counts else None
    p, keep = ao_struct(K, tmin, tmax, dirs, rotate)
    if flags is not None:
        p.flags = flags
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc = rtm.tracer_lib().rt_render_ao_device(gs._h, ctypes.byref(f), ctypes.byref(p), vp(bgra), vp(cnt), ctypes.c_void_p(st))
    assert rc == expect_rc, (rc, expect_rc)
    torch.cuda.synchronize()
    b = bgra.cpu().numpy().view(np.uint32)
    c = cnt.cpu().numpy() if want_counts else None
    if rc != 0:
        assert (b == S.SENTINEL).all() and (c is None or (c == FILL).all()), "a rejected call wrote"
        return None, None
    assert (b[W * H:] == S.SENTINEL).all(), "words written past the frame"
    if want_counts:
        assert (c[W * H * spp:] == FILL).all(), "bytes written past the counts"
        c = c[:W * H * spp].reshape(H, W, spp).copy()
    return b[:W * H].reshape(H, W).copy(), c


class AoScene:
    """One scene of these tests: .name, .hs (what rtm.GpuScene was made from: a HostScene, or a caller-built
    description), .gs, .sc (the RefScene over the same arrays); it unpacks as (hs, gs, sc).  traced(W, H, spp): the
    frame's camera rays and their closest hits from the library (host copies), computed once per frame shape."""

    def __init__(self, name, hs, gs, sc):
        self.name, self.hs, self.gs, self.sc = name, hs, gs, sc
        self._traced = {}

    def __iter__(self):
        return iter((self.hs, self.gs, self.sc))

    def __getitem__(self, i):
        return (self.hs, self.gs, self.sc)[i]

    def traced(self, W, H, spp):
        import torch
        key = (W, H, spp)
        if key not in self._traced:
            d_rays = self.gs.primary_rays(self.gs.frame(W, H, spp))
            res = self.gs.trace_rays(d_rays)
            torch.cuda.synchronize()
            h = res.hits.cpu().numpy().view(np.uint32)
            self._traced[key] = (d_rays.cpu().numpy(), h[:, 0].copy(), h[:, 1].view(np.float32).copy())
        return self._traced[key]


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """Per scene file: an AoScene (HostScene, GpuScene, RefScene), loaded once."""
    tmp = tmp_path_factory.mktemp("ao")
    cache = {}

    def get(name):
        if name not in cache:
            hs = rtm.HostScene.load(S.scene_file({"scene": name}, tmp))
            cache[name] = AoScene(name, hs, rtm.GpuScene(hs, 0), R.RefScene.from_host(hs))
        return cache[name]
    yield get
    for hs, gs, _ in cache.values():
        gs.close()
        hs.close()


def composed(torch, scene, W, H, spp, dirs, rotate, tmin, tmax):
    """The expected result on an AoScene: the composition of the three library calls and the restatement."""
    hs, gs, sc = scene
    rays, tri, t = scene.traced(W, H, spp)
    f = A.form(sc, rays, tri, t, dirs, rtm.ao_rotations() if rotate else None, W, H, spp)
    m = f["ao_rays"].shape[0]
    occ = np.zeros(0, np.uint8)
    if m:
        tmm = np.tile(np.array([tmin, tmax], np.float32), (m, 1))
        occ = gs.occluded(dev(torch, f["ao_rays"]), dev(torch, tmm))
        torch.cuda.synchronize()
        occ = occ.cpu().numpy()
    K = np.asarray(dirs).shape[0]
    cnt = A.counts(occ, f["hit"], K)
    return A.pixels(cnt, K, W, H, spp), cnt.reshape(H, W, spp), f, occ


def check(torch, scene, W, H, spp, K, rotate, tmin, tmax, dirs=None, what=""):
    hs, gs, sc = scene
    name = scene.name
    table = np.ascontiguousarray(dirs, np.float32) if dirs is not None else rtm.ao_table(K)
    want_pix, want_cnt, f, occ = composed(torch, scene, W, H, spp, table, rotate, tmin, tmax)
    got_pix, got_cnt = raw_ao(torch, gs, gs.frame(W, H, spp), table.shape[0], tmin, tmax, dirs=dirs, rotate=rotate)
    label = f"{name} {W}x{H}x{spp} K={table.shape[0]} rotate={rotate} ({float(tmin):g}, {float(tmax):g}) {what}"
    print(f"{label}: {int(f['hit'].sum())} hit samples, {int(occ.sum())} of {occ.size} AO rays occluded, "
          f"{np.unique(want_pix).size} distinct pixels")
    np.testing.assert_array_equal(got_cnt, want_cnt, err_msg=label + ": counts")
    np.testing.assert_array_equal(got_pix, want_pix, err_msg=label + ": pixels")
    # without d_counts: the same pixels
    only_pix, none = raw_ao(torch, gs, gs.frame(W, H, spp), table.shape[0], tmin, tmax, dirs=dirs, rotate=rotate,
                            want_counts=False)
    np.testing.assert_array_equal(only_pix, want_pix, err_msg=label + ": pixels without d_counts")
    return f, occ


# ------------------------------------------------------------------ 1. views
@pytest.mark.parametrize("name", VIEWS + EXTRA_VIEWS + tuple(SCENE_VIEWS))
def test_views(scenes, name):
    """Every view at K = 4, rotated, tmin = 1e-4 x the diagonal, tmax = 0.25 x the diagonal (the setting
    tests/test_ao_cpu.py shows to be non-vacuous), and at K = 5 unrotated over (0, +inf).  stack2100 walks the plain
    CSR ranges, the others the box runs; on the stacks the any-hit rays run lists of 1,500 and 2,100 records."""
    import torch
    W, H, spp = SCENE_VIEWS[name] if name in SCENE_VIEWS else (META["cases"][name][k] for k in ("W", "H", "spp"))
    hs, gs, sc = scenes(name)
    d = sc.diagonal()
    f, occ = check(torch, scenes(name), W, H, spp, 4, True, np.float32(1e-4) * d, np.float32(0.25) * d)
    if name == "away":
        assert occ.size == 0
    elif name not in EXTRA_VIEWS:
        assert 0.02 <= float(occ.mean()) <= 0.98
    check(torch, scenes(name), W, H, spp, 5, False, np.float32(0), INF)
    assert gs.info()["packed_cells"] == (0 if name == "stack2100" else 1)


# ------------------------------------------------------------------ 2. parameters
PARAMS = [  # K, spp, rotate, tmax / diagonal (None: +inf), tmin / diagonal
    (1, 1, True, 0.25, 1e-4), (1, 4, False, None, 0.0), (4, 1, False, 0.05, 0.0), (4, 16, True, None, 1e-4),
    (5, 4, True, 0.05, 1e-4), (5, 16, False, 0.25, 0.0), (16, 1, True, None, 1e-4), (16, 4, False, 0.25, 1e-4),
    (16, 16, True, 0.05, 0.0), (64, 1, False, 0.25, 1e-4), (64, 4, True, 0.05, 1e-4), (64, 16, True, None, 0.0),
]


@pytest.mark.parametrize("K,spp,rotate,tmax,tmin", PARAMS)
def test_parameters(scenes, K, spp, rotate, tmax, tmin):
    """K in {1, 4, 5, 16, 64} x spp in {1, 4, 16}, rotation on and off, tmax in {0.05, 0.25} x the diagonal and +inf,
    tmin in {0, 1e-4 x the diagonal}: `inside` at 33x21 (partial tiles; at spp 16 a tile is 64 waves)."""
    import torch
    d = scenes("inside")[2].diagonal()
    f, occ = check(torch, scenes("inside"), 33, 21, spp, K, rotate, np.float32(tmin) * d,
                   INF if tmax is None else np.float32(tmax) * d)
    assert 0 < int(occ.sum()) < occ.size


@pytest.mark.parametrize("name", ["inside", "scene1"])
def test_caller_directions_of_mixed_lengths(scenes, name):
    """A caller's table whose entries are the built-in directions scaled to lengths 0.5, 7.9 and 8.5 in turn (K = 6),
    used as passed: waves vote for the Newton reciprocal (|w|_inf <= 8) and for the division, some split.  t is in
    units of |w|, so the interval is what it is: no rescaling."""
    import torch
    d = scenes(name)[2].diagonal()
    dirs = (rtm.ao_table(6) * np.array([0.5, 7.9, 8.5, 8.5, 0.5, 7.9], np.float32)[:, None]).astype(np.float32)
    W, H, spp = (62, 46, 4) if name == "inside" else SCENE_VIEWS[name]
    for rotate in (True, False):
        f, occ = check(torch, scenes(name), W, H, spp, 6, rotate, np.float32(1e-4) * d, np.float32(0.25) * d, dirs=dirs,
                       what="caller dirs")
        wm = np.abs(f["w"]).max(2)
        assert (wm > 8).any() and (wm <= 8).any() and (wm[:, 2] > 8).any() and (wm[:, 3] <= 8).any()
        assert 0 < int(occ.sum()) < occ.size


# ------------------------------------------------------------------ 3. frame shapes
@pytest.mark.parametrize("W,H,spp", [(1, 1, 4), (15, 17, 4), (16, 16, 4), (17, 1, 4), (63, 47, 4), (130, 3, 4), (3, 3, 64),
                                     (17, 16, 1), (16, 17, 2), (5, 3, 32), (9, 2, 8)])
def test_frame_shapes(scenes, W, H, spp):
    """Partial tiles, one-wave launches, every power-of-two spp; at spp 64 one pixel fills a wave."""
    import torch
    d = scenes("inside")[2].diagonal()
    check(torch, scenes("inside"), W, H, spp, 4, True, np.float32(1e-4) * d, np.float32(0.25) * d)


# ------------------------------------------------------------------ 5. launch sequences
def test_ao_frame_between_render_frames_on_other_streams(scenes, golden):
    """render_frame_device, an AO frame and render_frame_device again, of one scene on three streams without a host
    wait (1920x1080x4 frames of scene 8, whose tables the 96x54x4 AO frame rewrites and the second frame rewrites
    back): both frames have the golden SHA, the AO frame the bytes of the composition."""
    import hashlib

    import torch
    name = "scene8"
    hs, gs, sc = scenes(name)
    W, H, spp = SCENE_VIEWS[name]
    d = sc.diagonal()
    tmin, tmax = np.float32(1e-4) * d, np.float32(0.25) * d
    want_pix, want_cnt, f, occ = composed(torch, scenes(name), W, H, spp, rtm.ao_table(4), True, tmin, tmax)
    big = gs.frame(1920, 1080, 4)
    outs = [torch.full((1920 * 1080,), S.SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2)]
    s0, s1, s2 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    bgra = torch.full((W * H + TAIL,), S.SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((W * H * spp + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    p, keep = ao_struct(4, tmin, tmax, None, True)
    fa = gs.frame(W, H, spp)
    torch.cuda.synchronize()
    gs.render_frame_device(big, outs[0].data_ptr(), s0.cuda_stream)
    assert rtm.tracer_lib().rt_render_ao_device(gs._h, ctypes.byref(fa), ctypes.byref(p), vp(bgra), vp(cnt),
                                                ctypes.c_void_p(s1.cuda_stream)) == 0
    gs.render_frame_device(big, outs[1].data_ptr(), s2.cuda_stream)
    torch.cuda.synchronize()
    for i in range(2):
        sha = hashlib.sha256(outs[i].cpu().numpy().view(np.uint32).tobytes()).hexdigest()
        assert sha == golden["frames_1080p4"]["8"]["bgra_sha256"], i
    b, c = bgra.cpu().numpy().view(np.uint32), cnt.cpu().numpy()
    assert (b[W * H:] == S.SENTINEL).all() and (c[W * H * spp:] == FILL).all()
    np.testing.assert_array_equal(c[:W * H * spp].reshape(H, W, spp), want_cnt)
    np.testing.assert_array_equal(b[:W * H].reshape(H, W), want_pix)


def test_graph_capture_and_replay(scenes):
    """One warm-up call of the frame, the call captured in a graph (torch.cuda.CUDAGraph), two replays into cleared
    buffers: the composition's bytes each time.  A caller's table is read during the captured call only."""
    import torch
    name = "scene1"
    hs, gs, sc = scenes(name)
    W, H, spp = SCENE_VIEWS[name]
    d = sc.diagonal()
    tmin, tmax = np.float32(1e-4) * d, np.float32(0.25) * d
    dirs = np.ascontiguousarray(rtm.ao_table(5)[::-1])
    want_pix, want_cnt, f, occ = composed(torch, scenes(name), W, H, spp, dirs, True, tmin, tmax)
    bgra = torch.full((W * H + TAIL,), S.SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((W * H * spp + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    p, keep = ao_struct(5, tmin, tmax, dirs.copy(), True)
    fa = gs.frame(W, H, spp)
    L = rtm.tracer_lib()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert L.rt_render_ao_device(gs._h, ctypes.byref(fa), ctypes.byref(p), vp(bgra), vp(cnt), ctypes.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assert L.rt_render_ao_device(gs._h, ctypes.byref(fa), ctypes.byref(p), vp(bgra), vp(cnt), ctypes.c_void_p(s.cuda_stream)) == 0
    keep[:] = np.nan                        # the library kept no pointer: the replays use the captured arguments
    for _ in range(2):
        bgra.fill_(S.SENTINEL)
        cnt.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        b, c = bgra.cpu().numpy().view(np.uint32), cnt.cpu().numpy()
        assert (b[W * H:] == S.SENTINEL).all() and (c[W * H * spp:] == FILL).all()
        np.testing.assert_array_equal(c[:W * H * spp].reshape(H, W, spp), want_cnt)
        np.testing.assert_array_equal(b[:W * H].reshape(H, W), want_pix)


def test_python_surface(scenes):
    """GpuScene.render_ao: a torch.uint32 [H, W] tensor (and uint8 [H, W, spp] counts), in place with out=, on another
    stream; the raw call's bytes."""
    import torch
    name = "inside"
    hs, gs, sc = scenes(name)
    W, H, spp = 62, 46, 4
    d = sc.diagonal()
    tmin, tmax = np.float32(1e-4) * d, np.float32(0.25) * d
    f = gs.frame(W, H, spp)
    want_pix, want_cnt = raw_ao(torch, gs, f, 4, tmin, tmax)
    pix, cnt = gs.render_ao(f, 4, tmin, tmax, counts=True)
    torch.cuda.synchronize()
    assert tuple(pix.shape) == (H, W) and pix.is_cuda and tuple(cnt.shape) == (H, W, spp) and cnt.dtype == torch.uint8
    assert pix.dtype == getattr(torch, "uint32", torch.int32)
    np.testing.assert_array_equal(pix.cpu().numpy().view(np.uint32), want_pix)
    np.testing.assert_array_equal(cnt.cpu().numpy(), want_cnt)
    out = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    back = gs.render_ao(f, tmin=tmin, tmax=tmax, out=out, stream=side.cuda_stream)
    side.synchronize()
    assert back is out
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want_pix)
    dirs = (rtm.ao_table(3) * np.float32(2)).astype(np.float32)
    a, _ = raw_ao(torch, gs, f, 3, tmin, tmax, dirs=dirs, rotate=False)
    b = gs.render_ao(f, tmin=tmin, tmax=tmax, dirs=dirs, rotate=False)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(b.cpu().numpy().view(np.uint32), a)
    with pytest.raises(ValueError):
        gs.render_ao(f, out=out[:, ::2])
    with pytest.raises(ValueError):
        gs.render_ao(f, out=torch.zeros((H, W + 1), dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------ 6. rejected calls
def test_rejected_calls_write_nothing(scenes):
    """Every rejection on a live scene: RT_E_INVALID, and every byte of both buffers still 0x5A (raw_ao checks)."""
    import torch
    hs, gs, sc = scenes("inside")
    good = rtm.ao_table(4)
    f = gs.frame(16, 16, 4)
    for K, tmin, tmax in ((0, 0.0, 1.0), (65, 0.0, 1.0), (4, np.nan, 1.0), (4, 0.0, np.nan), (4, 1.0, 1.0), (4, 2.0, 1.0),
                          (4, np.inf, np.inf)):
        raw_ao(torch, gs, f, K, tmin, tmax, expect_rc=1)
    for v in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[2, 1] = v
        raw_ao(torch, gs, f, 4, 0.0, 1.0, dirs=bad, expect_rc=1)
    for flags in (2, 3, 0x100):
        raw_ao(torch, gs, f, 4, 0.0, 1.0, flags=flags, expect_rc=1)
    for bad in (gs.frame(16, 16, 3), gs.frame(16, 16, 128), gs.frame(16, 16, 4, intersector=rtm.RT_ISECT_BRUTE_FORCE),
                gs.frame(16, 16, 4, intersector=rtm.RT_ISECT_RAY_MARCH), gs.frame(16, 16, 4, tri_test=rtm.RT_TRI_BARYCENTRIC),
                gs.frame(16, 16, 4, kernel=7)):
        raw_ao(torch, gs, bad, 4, 0.0, 1.0, expect_rc=1)
    L = rtm.tracer_lib()
    p, _ = ao_struct(4, 0.0, 1.0, None, True)
    buf = torch.full((16 * 16 + TAIL,), S.SENTINEL, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.rt_render_ao_device(None, ctypes.byref(f), ctypes.byref(p), vp(buf), None, st) == 1
    assert L.rt_render_ao_device(gs._h, None, ctypes.byref(p), vp(buf), None, st) == 1
    assert L.rt_render_ao_device(gs._h, ctypes.byref(f), None, vp(buf), None, st) == 1
    assert L.rt_render_ao_device(gs._h, ctypes.byref(f), ctypes.byref(p), None, vp(buf), st) == 1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint32) == S.SENTINEL).all()
    # ... and the scene still renders
    pix, cnt = raw_ao(torch, gs, f, 4, np.float32(1e-3), INF)
    assert (cnt != FILL).all()
