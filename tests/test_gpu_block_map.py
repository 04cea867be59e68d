"""The lane kernels' prologue on the device: the block map without divisions, the plan mark, the
miss-mask word and the camera-space table entries loaded as one group -- at the smallest frames where the map's
cases differ.

  shape (W x H x spp)   tiles     what it exercises
  16x16x4               one       every block in the tail past the whole rounds (and below 8 blocks: no front)
  48x112x4              3 x 7     fewer blocks than one round of 8 turns (nb < 8 chunk)
  48x128x1              3 x 8     exactly one round, one workgroup per tile
  112x144x4             7 x 9     a round and a tail
  112x272x4             7 x 17    two rounds and a tail
  40x130x16             ragged    tiles overhanging the region on both axes (the clamped table loads)

RT_HF_MIN_BLOCKS=8 and RT_WG64_MIN_BLOCKS=8 (read at scene creation) put these frames on the heavy-first front and on
k_render_lanes_w64; RT_HF_FLOOR=1 besides, because the plan lists a block only above max(hf_floor, ...) shader cycles
and the default floor (100,000) is above every wave of frames this small: without it the front exists but stays
empty, and neither the list nor a matching mark is ever read.  Each scene runs once more with none of them set.

Per shape the same AUTO frame is rendered 40 times (plans are measured at frames 0, 1, 16, 32 and adopted after), and
frames 0, 1, 2, 17, 18, 33 and 39 must equal the RT_KERNEL_LANES frame of that shape byte for byte (and the CPU
restatement's for scene 1, and tests/golden's where it holds that shape); rt_render_hits_device must agree with its
RT_KERNEL_LANES launch.  One shape each also runs overlapped on two streams, dealt to 2 and 8 ranks, and as a batch
of the two scenes.  The forced runs must have seen, in at least one shape, a front with listed blocks in use, a miss
mask with flagged items in use, and a launch of the one-wave kernel (rt_debug_heavy_first, rt_debug_miss_mask,
rt_debug_lane_launches: rt_scene_info's layout is pinned by tests/test_abi.py, so the launch counter has its own
debug call).
"""
import gzip
import os

import numpy as np
import pytest

import synth_scenes as sy
from conftest import GOLD, load_package

pytestmark = pytest.mark.gpu
rtm = load_package()
SHAPES = ((16, 16, 4), (48, 112, 4), (48, 128, 1), (112, 144, 4), (112, 272, 4), (40, 130, 16))
CHECKED = (0, 1, 2, 17, 18, 33, 39)
FRAMES = 40
OVERLAP_SHAPE, SHARD_SHAPE, BATCH_SHAPE = (112, 272, 4), (112, 144, 4), (48, 112, 4)
FORCED = {"RT_HF_MIN_BLOCKS": "8", "RT_WG64_MIN_BLOCKS": "8", "RT_HF_FLOOR": "1", "RT_MISS_SKIP": "1"}
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def hosts():
    hs = {"scene1": rtm.HostScene.load(1), "axis_z": sy.build_host(sy.cases()["axis_z"])}
    yield hs
    for h in hs.values():
        h.close()


def gpu_scene(hs, forced):
    """A device scene created with the tunables of FORCED in the environment (they are read once, at creation)."""
    old = {k: os.environ.get(k) for k in FORCED}
    try:
        for k, v in FORCED.items():
            if forced:
                os.environ[k] = v
            else:
                os.environ.pop(k, None)
        return rtm.GpuScene(hs, 0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def words(t):
    return t.cpu().numpy().view(np.uint32)


class Seen:
    """What the launches of a run went through (debug calls between frames)."""

    def __init__(self, gs):
        self.gs, self.front, self.flagged, self.one_wave = gs, 0, 0, 0
        self.launches = gs.lane_launches()

    def before(self):
        front, listed, epoch = self.gs.heavy_first()
        # a shape's first two frames run in the natural order whatever is listed
        return front > 0 and listed > 0 and epoch >= 3

    def after(self, planned):
        front, listed, _ = self.gs.heavy_first()
        self.front += planned and front > 0 and listed > 0
        self.flagged += self.gs.miss_mask()[0] > 0
        now = self.gs.lane_launches()
        self.one_wave += now[1] > self.launches[1]
        self.launches = now


def render_device(gs, frame, stream=0):
    import torch
    out = torch.full((frame.width * frame.height,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gs.render_frame_device(frame, out.data_ptr(), stream)
    torch.cuda.synchronize()
    return words(out).reshape(frame.height, frame.width)


def hits_of(gs, W, H, spp, kernel):
    import torch
    out = torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda")
    hits = torch.full((W * H * spp,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gs.render_hits_device(gs.frame(W, H, spp, kernel=kernel), 0, 1, out.data_ptr(), hits.data_ptr(), 0)
    torch.cuda.synchronize()
    return words(out).reshape(H, W), words(hits)


def golden_frame(name, W, H, spp):
    path = os.path.join(GOLD, "frames", f"{name}_{W}x{H}x{spp}.bgra.gz")
    if not os.path.exists(path):
        return None
    with gzip.open(path, "rb") as f:
        return np.frombuffer(f.read(), "<u4").reshape(H, W)


def overlapped(gs, W, H, spp, ref, seen):
    """FRAMES frames alternating between two streams with RT_KERNEL_FLAG_OVERLAP, each pair checked.  The debug reads
    of Seen synchronise the device (rt_debug_heavy_first, rt_debug_miss_mask), so they are taken once per PAIR: before
    its stream-0 launch and after the pair's own synchronisation.  Nothing between the two launches of a pair waits
    for the device, so both frames are in flight together -- one reading the current plan's marks, list and counts
    while the other, or its k_hf_plan, runs on the other stream."""
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.zeros(W * H, dtype=torch.int32, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    planned = False
    for i in range(FRAMES):
        k = i % 2
        if k == 0:
            planned = seen.before()
        with torch.cuda.stream(streams[k]):
            outs[k].fill_(SENTINEL)
        gs.render_frame_device(gs.frame(W, H, spp, kernel=rtm.RT_KERNEL_AUTO | rtm.RT_KERNEL_FLAG_OVERLAP),
                               outs[k].data_ptr(), streams[k].cuda_stream)
        if k:
            torch.cuda.synchronize()
            for o in outs:
                assert np.array_equal(words(o).reshape(H, W), ref), ("overlap", i)
            seen.after(planned)
    torch.cuda.synchronize()


def sharded(gs, W, H, spp, ref, seen, nranks, reps=20):
    """The frame dealt to nranks ranks `reps` times (every rank's launch shape measures and adopts its own plan),
    un-sharded and compared with the whole frame each time."""
    import torch
    e = rtm.shard_elems(W, H, nranks)
    for rep in range(reps):
        gathered = torch.full((nranks * e,), SENTINEL, dtype=torch.int32, device="cuda")
        out = torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for rank in range(nranks):
            planned = seen.before()
            gs.render_shard_device(gs.frame(W, H, spp), rank, nranks, gathered.data_ptr() + 4 * rank * e, 0)
            seen.after(planned)
        rtm.unshard_device(W, H, nranks, gathered.data_ptr(), out.data_ptr(), 0)
        torch.cuda.synchronize()
        assert np.array_equal(words(out).reshape(H, W), ref), ("shards", nranks, rep)


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "defaults"])
@pytest.mark.parametrize("name", ["scene1", "axis_z"])
def test_small_frames(oracle, hosts, name, forced):
    gs = gpu_scene(hosts[name], forced)
    seen = Seen(gs)
    try:
        if forced:
            assert gs.info()["hf_min_blocks"] == 8
        for W, H, spp in SHAPES:
            ref = gs.render_frame(gs.frame(W, H, spp, kernel=rtm.RT_KERNEL_LANES))
            if name == "scene1":
                assert np.array_equal(ref, oracle.render(1, W, H, spp)[0]), (W, H, spp)
            gold = golden_frame(name, W, H, spp)
            assert gold is None or np.array_equal(ref, gold), (W, H, spp)
            for i in range(FRAMES):
                planned = seen.before()
                got = render_device(gs, gs.frame(W, H, spp))
                seen.after(planned)
                if i in CHECKED:
                    assert np.array_equal(got, ref), (name, (W, H, spp), i, int((got != ref).sum()))
            a_out, a_hits = hits_of(gs, W, H, spp, rtm.RT_KERNEL_AUTO)
            l_out, l_hits = hits_of(gs, W, H, spp, rtm.RT_KERNEL_LANES)
            assert np.array_equal(a_out, ref) and np.array_equal(l_out, ref), (name, (W, H, spp), "hits frame")
            assert np.array_equal(a_hits, l_hits), (name, (W, H, spp), "hit IDs")
            if (W, H, spp) == OVERLAP_SHAPE:
                overlapped(gs, W, H, spp, ref, seen)
            if (W, H, spp) == SHARD_SHAPE:
                for nranks in (2, 8):
                    sharded(gs, W, H, spp, ref, seen, nranks)
        print(name, "forced" if forced else "defaults", "front in use", seen.front, "mask in use", seen.flagged,
              "one-wave launches", seen.one_wave, "of", seen.launches)
        if forced:
            assert seen.front > 0, "no frame ran under a front with listed blocks"
            assert seen.one_wave > 0, "no launch of the one-wave kernel"
            if name == "scene1":        # (its own camera leaves rows of the frame outside the grid box)
                assert seen.flagged > 0, "no frame ran with flagged items in its miss mask"
    finally:
        gs.close()


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "defaults"])
def test_batch_of_the_two_scenes(hosts, forced):
    """Both scenes' frames in one rt_render_batch_device launch, 20 times: each equals its own RT_KERNEL_LANES frame."""
    import torch
    W, H, spp = BATCH_SHAPE
    gss = [gpu_scene(hosts[n], forced) for n in ("scene1", "axis_z")]
    seen = Seen(gss[0])
    try:
        refs = [g.render_frame(g.frame(W, H, spp, kernel=rtm.RT_KERNEL_LANES)) for g in gss]
        before = gss[0].info()
        for rep in range(20):
            outs = [torch.full((W * H,), SENTINEL, dtype=torch.int32, device="cuda") for _ in gss]
            torch.cuda.synchronize()
            planned = seen.before()
            rtm.render_batch_device(gss, [g.frame(W, H, spp) for g in gss], [o.data_ptr() for o in outs], stream=0)
            torch.cuda.synchronize()
            seen.after(planned)
            for k, o in enumerate(outs):
                assert np.array_equal(words(o).reshape(H, W), refs[k]), (rep, k)
        after = gss[0].info()
        assert after["batch_launches"] == before["batch_launches"] + 20, (before, after)
        assert after["batch_fallbacks"] == before["batch_fallbacks"], (before, after)
        print("batch", "forced" if forced else "defaults", "front in use", seen.front, "one-wave launches", seen.one_wave)
        assert seen.one_wave > 0        # (a batched launch takes one-wave workgroups at any size)
        if forced:
            assert seen.front > 0, "no batch ran under a front with listed blocks"
    finally:
        for g in gss:
            g.close()
