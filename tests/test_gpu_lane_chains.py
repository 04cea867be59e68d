"""The lean add chains of AUTO's per-lane box runs (csrc/rt_lane_run.h) on the device: frames and
hit IDs byte for byte those of RT_KERNEL_LANES (the plain per-lane walk, no box runs) from the same library and of
the CPU oracle.

* scenes 1, 8 and 5 at 192x108x4;
* a caller-built grid 512 cells long with one triangle at the far end, 64x64x4, the camera outside and inside it,
  so a ray crosses several of the longest boxes; and the same grid from a camera 2^24 scene diameters away, where
  every chain is stuck (a cell's step is far below an ulp of the crossing times);
* rt_trace_rays_device on 4,096 rays -- axis-parallel, near-axis (components down to the subnormals, whose cw / d
  overflows: the bounds are NaN and the wave takes the guarded loops) and long directions -- against the counting
  walk, which takes no box run;
* scene 8 dealt to 2 and 8 ranks (the wide section's walk included), and one overlapped pair on two streams.

Which chain form a case takes: the vote of rt_lane_run.h fails only for a NaN exit bound (a NaN or infinite crossing
or step, or f dt + x beyond FLT_MAX).  No camera reaches that -- a normalised direction times a camera matrix has
no component small enough -- so every FRAME here, the far camera's included, takes the lean chains: the far camera
pins the lean form on stuck chains, not the fall-back.  On the device the guarded fall-back is reached only by the
caller-supplied rays of kind 4 below with a subnormal component (1e-40, 1e-44: the step cw / d is above 1e38 or infinite);
that such steps give a NaN bound is shown on the CPU (tests/test_lane_chains_lean.py::test_subnormal_components_fail_the_vote;
its `naninf` and `onefail` families run the fall-back against the reference loops) -- the device cannot report which
form a wave took.  The AO walks and
the wide section keep the guarded loops alone.

Small frames: every case runs in a second or two.
"""
import numpy as np
import pytest

from conftest import load_package
from synth_scenes import OracleScene, mesh_of

rtm = load_package()
pytestmark = pytest.mark.gpu
W, H, SPP = 192, 108, 4
SENTINEL = 0x5A5A5A5A
# sample 0 on the pixel corner: pixel (32, 32) of a 64x64 frame looks exactly down the camera axis
OFFSETS = np.array([0.0, 0.0, 0.25, 0.5, 0.5, 0.25, 0.75, 0.75], np.float32)


def words(t):
    return t.cpu().numpy().view(np.uint32)


def frame_and_hits(gs, frame, rank=0, nranks=1):
    import torch
    n = frame.width * frame.height
    out = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    hits = torch.full((n * frame.spp,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gs.render_hits_device(frame, rank, nranks, out.data_ptr(), hits.data_ptr(), 0)
    torch.cuda.synchronize()
    return words(out).reshape(frame.height, frame.width), words(hits)


def check_auto_against_plain(gs, w, h, spp, exp=None, exp_hits=None, **kw):
    """AUTO's frame and hit IDs == RT_KERNEL_LANES' (== the oracle's, when given).  Returns the frame."""
    a_img, a_hits = frame_and_hits(gs, gs.frame(w, h, spp, **kw))
    l_img, l_hits = frame_and_hits(gs, gs.frame(w, h, spp, kernel=rtm.RT_KERNEL_LANES, **kw))
    assert a_img.tobytes() == l_img.tobytes(), f"{int((a_img != l_img).sum())} pixels differ from RT_KERNEL_LANES"
    assert a_hits.tobytes() == l_hits.tobytes(), f"{int((a_hits != l_hits).sum())} hit IDs differ from RT_KERNEL_LANES"
    if exp is not None:
        assert a_img.tobytes() == exp.tobytes(), f"{int((a_img != exp).sum())} pixels differ from the oracle"
        assert a_hits.tobytes() == exp_hits.tobytes(), f"{int((a_hits != exp_hits).sum())} hit IDs differ from the oracle"
    return a_img, a_hits


@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(sid):
        if sid not in cache:
            hs = rtm.HostScene.load(sid)
            cache[sid] = (hs, rtm.GpuScene(hs, 0))
        return cache[sid]
    yield get
    for hs, gs in cache.values():
        gs.close()
        hs.close()


@pytest.fixture(scope="module")
def expected(oracle):
    cache = {}

    def get(sid):
        if sid not in cache:
            img, hits, _ = oracle.render(sid, W, H, SPP, hits=True)
            cache[sid] = (img, hits)
        return cache[sid]
    return get


@pytest.mark.parametrize("sid", [1, 8, 5])
def test_scene_frames(scenes, expected, sid):
    hs, gs = scenes(sid)
    exp, exp_hits = expected(sid)
    img, hits = check_auto_against_plain(gs, W, H, SPP, exp, exp_hits)
    assert (hits != 0xFFFFFFFF).any()


# ---- the long grid ---------------------------------------------------------------------------------------------
LONG = 64.0        # the grid's extent along x; 1 along y and z: 512 x 9 x 9 cells of 1/8
FOV = 3.0          # degrees: the far triangle covers a few hundred samples from the near end


def long_tris():
    far = [[LONG - 0.05, 0.1, 0.1], [LONG - 0.02, 0.9, 0.2], [LONG - 0.04, 0.3, 0.9]]
    near = [[0.0, 0.0, 0.0], [0.02, 0.0, 0.01], [0.01, 0.02, 0.0]]
    top = [[LONG, 1.0, 1.0], [LONG - 0.02, 1.0, 0.99], [LONG - 0.01, 0.98, 1.0]]
    return [far, near, top]


CAMERAS = {"outside": ((-20.0, 0.45, 0.4), (LONG, 0.45, 0.4)),
           "outside_oblique": ((-6.0, -0.8, 2.2), (LONG, 0.5, 0.4)),
           "inside": ((0.6, 0.5, 0.5), (LONG, 0.45, 0.4)),
           "far": ((-LONG * 16777216.0, 0.5, 0.5), (LONG, 0.5, 0.5))}


@pytest.mark.parametrize("view", list(CAMERAS))
def test_long_grid(oracle, tmp_path, view):
    eye, at = CAMERAS[view]
    v, t = mesh_of(long_tris())
    hs = rtm.HostScene.from_mesh(v, t, FOV, rtm.look_at(eye, at), grid_res=512)
    gs = rtm.GpuScene(hs, 0)
    try:
        assert hs.grid()[0]["dims"][0] == 512 and max(hs.grid()[0]["dims"][1:]) <= 9
        path = str(tmp_path / "long.rtscene")
        hs.save(path)
        orc = OracleScene(oracle, path)
        try:
            exp, exp_hits = orc.render(64, 64, 4)
        finally:
            orc.close()
        img, hits = check_auto_against_plain(gs, 64, 64, 4, exp, exp_hits)
        # sample 0 on the pixel corner: the centre pixel's ray runs exactly along the grid (two still axes)
        img2, hits2 = check_auto_against_plain(gs, 64, 64, 4, sample_offsets=OFFSETS)
        if view in ("outside", "inside"):
            assert (hits == 0).any(), "no sample reaches the far triangle"
        print(view, "hits of the far triangle:", int((hits == 0).sum()), "and", int((hits2 == 0).sum()))
    finally:
        gs.close()
        hs.close()


# ---- caller-supplied rays --------------------------------------------------------------------------------------
def query_rays(lo, hi):
    r = np.random.Generator(np.random.PCG64(97))
    ctr, ext = (lo + hi) * np.float32(0.5), (hi - lo)
    n = 4096
    org = (ctr + 0.9 * ext * r.uniform(-1, 1, (n, 3))).astype(np.float32)
    d = r.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    k = np.arange(n)
    ax = r.integers(0, 3, n)
    sign = r.choice(np.array([-1.0, 1.0], np.float32), n)
    kind = (k // 64) % 8                    # whole waves of a kind, then (kind 7) every ray a kind of its own
    kind = np.where(kind == 7, k % 7, kind)
    for i in range(n):
        a, b = ax[i], (ax[i] + 1) % 3
        if kind[i] == 1:                    # axis-parallel
            d[i] = 0.0
            d[i, a] = sign[i]
        elif kind[i] == 2:                  # one still axis
            d[i, a] = 0.0
        elif kind[i] == 3:                  # near-axis: a component of 1e-30
            d[i, a] = sign[i] * np.float32(1e-30)
        elif kind[i] == 4:                  # a component near and in the subnormals: cw / d overflows
            d[i, a] = sign[i] * np.float32([1e-37, 1e-38, 1e-40, 1e-44][i % 4])
            d[i, b] = np.float32(1e-3) * d[i, b]
        elif kind[i] == 5:                  # long directions
            d[i] *= np.float32([2.0 ** 20, 2.0 ** 60, 2.0 ** 100, 2.0 ** -60][i % 4])
        elif kind[i] == 6:                  # two tiny components
            d[i, a] = sign[i] * np.float32(1e-30)
            d[i, b] = np.float32(1e-36)
    return np.ascontiguousarray(np.concatenate([org, d.astype(np.float32)], axis=1), np.float32)


@pytest.mark.parametrize("sid", [1, 8])
def test_caller_rays_against_the_counting_walk(scenes, oracle, sid):
    hs, gs = scenes(sid)
    info = oracle.info(sid)
    rays = query_rays(np.array(list(info.aabb_min), np.float32), np.array(list(info.aabb_max), np.float32))
    fast = gs.trace_rays(rays.copy())
    slow = gs.trace_rays(rays.copy(), count=True)
    nhit = int((slow.tri != 0xFFFFFFFF).sum())
    print(f"scene {sid}: {rays.shape[0]} rays, {nhit} hits by the counting walk")
    # (the comparison must not be vacuous on either side: a twentieth of the set each)
    assert nhit >= 200 and rays.shape[0] - nhit >= 200
    np.testing.assert_array_equal(fast.hits.view(np.uint32), slow.hits.view(np.uint32))
    srt = gs.trace_rays(rays.copy(), sort=True)
    np.testing.assert_array_equal(srt.hits.view(np.uint32), slow.hits.view(np.uint32))


# ---- ranks and streams -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 8])
def test_scene8_dealt_to_ranks(scenes, expected, nranks):
    import torch
    hs, gs = scenes(8)
    exp, _ = expected(8)
    e = rtm.shard_elems(W, H, nranks)
    for kernel in (rtm.RT_KERNEL_AUTO, rtm.RT_KERNEL_AUTO | rtm.RT_KERNEL_FLAG_WIDE_HEAVY):
        for rep in range(3):
            gathered = torch.full((nranks * e,), SENTINEL, dtype=torch.int32, device="cuda")
            out = torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            for rank in range(nranks):
                gs.render_shard_device(gs.frame(W, H, SPP, kernel=kernel), rank, nranks, gathered.data_ptr() + 4 * rank * e, 0)
            rtm.unshard_device(W, H, nranks, gathered.data_ptr(), out.data_ptr(), 0)
            torch.cuda.synchronize()
            got = words(out).reshape(H, W)
            assert got.tobytes() == exp.tobytes(), (nranks, kernel, rep, int((got != exp).sum()))


def test_overlapped_pair_on_two_streams(scenes, expected):
    import torch
    hs, gs = scenes(1)
    exp, _ = expected(1)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for k in range(2):
        gs.render_frame_device(gs.frame(W, H, SPP, kernel=rtm.RT_KERNEL_AUTO | rtm.RT_KERNEL_FLAG_OVERLAP),
                               outs[k].data_ptr(), streams[k].cuda_stream)
    torch.cuda.synchronize()
    for k in range(2):
        got = words(outs[k]).reshape(H, W)
        assert got.tobytes() == exp.tobytes(), (k, int((got != exp).sum()))
