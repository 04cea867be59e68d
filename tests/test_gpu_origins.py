"""One scene at SEVERAL camera origins, in one batch and from launch to launch: the host side that picks
which of a scene's two per-origin record buffers a frame reads, recomputes it (k_origin_pre) and orders
that recompute after the launches that still read it (csrc/rt_fref_slots.h, order_all / order_overlap,
launch_batch).  tests/test_fref_slots.py checks the policy exhaustively on the CPU; here
real launch sequences run on the device and EVERY output of EVERY step is compared bit for bit.

Scenes 1 and 8 at 256x144x4 from five origins: the four reference views of tests/test_gpu_views.py
(golden["views"], the reference's own renders: frame, per-sample hit IDs, record columns) and the scene's
own camera (the oracle's restatement, which tests/test_oracle_golden.py pins to the reference).  Fresh
scenes per test: the order of launches on a scene is the point."""
import contextlib
import hashlib

import numpy as np
import pytest

from conftest import load_package
from test_gpu_views import expect, host, product_records, shas, view_frame

pytestmark = pytest.mark.gpu
rtm = load_package()
W, H, SPP = 256, 144, 4
X, Y, Z, V = "inside_down_z", "inside_down_x", "orbit37", "corner"     # the four views (V: the issue's W)
OWN = "own"
SENT = 0x5A5A5A5A


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sha_dev(t):
    return sha(t.cpu().numpy())


@pytest.fixture(scope="module")
def expected(golden, oracle):
    """(scene, origin name) -> the fixture dict (bgra_sha256, hits_sha256; record columns for the views).
    Computed once, never modified."""
    exp = {}
    for sid in (1, 8):
        for n in (X, Y, Z, V):
            v = golden["views"][f"scene{sid}_{n}"]
            assert (v["W"], v["H"], v["spp"], v["scene"]) == (W, H, SPP, sid)
            exp[(sid, n)] = v
        img, hid, _ = oracle.render(sid, W, H, SPP, hits=True)
        exp[(sid, OWN)] = {"bgra_sha256": sha(img), "hits_sha256": sha(hid)}
    return exp


@pytest.fixture(scope="module")
def hosts():
    hs = {sid: rtm.HostScene.load(sid) for sid in (1, 8)}
    yield hs
    for h in hs.values():
        h.close()


@contextlib.contextmanager
def fresh(hosts, *sids):
    """New GpuScenes (no per-origin records computed, no launch yet), closed whatever happens."""
    import torch
    gss = []
    try:
        for sid in sids:
            gss.append(rtm.GpuScene(hosts[sid], 0))
        yield gss
    finally:
        torch.cuda.synchronize()
        for g in gss:
            g.close()


def frame_of(gs, expected, sid, name, kernel=rtm.RT_KERNEL_AUTO):
    if name == OWN:
        return gs.frame(W, H, SPP, kernel=kernel)
    return view_frame(gs, expected[(sid, name)], kernel=kernel)


def origin_bits(f):
    return tuple(np.array([f.cam[12], f.cam[13], f.cam[14]], np.float32).view(np.uint32).tolist())


def buffers(torch, n, elems=W * H):
    outs = [torch.full((elems,), SENT, dtype=torch.int32, device="cuda") for _ in range(n)]
    hits = [torch.full((W * H * SPP,), SENT, dtype=torch.int32, device="cuda") for _ in range(n)]
    return outs, hits


def batch(torch, expected, items, label=""):
    """items: [(gs, sid, origin name)] rendered by ONE rt_render_batch_device call with d_hits into
    sentinel-filled buffers; every frame and its hit IDs compared."""
    outs, hits = buffers(torch, len(items))
    fs = [frame_of(g, expected, sid, n) for g, sid, n in items]
    rtm.render_batch_device([g for g, _, _ in items], fs, [o.data_ptr() for o in outs],
                            d_hits=[h.data_ptr() for h in hits], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for i, ((_, sid, n), o, h) in enumerate(zip(items, outs, hits)):
        assert sha_dev(o) == expected[(sid, n)]["bgra_sha256"], (label, i, sid, n)
        assert sha_dev(h) == expected[(sid, n)]["hits_sha256"], (label, i, sid, n)


def single(torch, expected, gs, sid, name, label="", with_hits=False):
    outs, hits = buffers(torch, 1)
    f = frame_of(gs, expected, sid, name)
    st = torch.cuda.current_stream().cuda_stream
    if with_hits:
        gs.render_hits_device(f, 0, 1, outs[0].data_ptr(), hits[0].data_ptr(), st)
    else:
        gs.render_frame_device(f, outs[0].data_ptr(), st)
    torch.cuda.synchronize()
    assert sha_dev(outs[0]) == expected[(sid, name)]["bgra_sha256"], (label, sid, name)
    if with_hits:
        assert sha_dev(hits[0]) == expected[(sid, name)]["hits_sha256"], (label, sid, name)


def counters(gs):
    i = gs.info()
    return i["batch_launches"], i["batch_fallbacks"]


@pytest.mark.parametrize("sid", [1, 8])
def test_five_distinct_origins(hosts, expected, sid):
    """The premise of every case below: the four views and the scene's own camera are five origins."""
    with fresh(hosts, sid) as (gs,):
        assert len({origin_bits(frame_of(gs, expected, sid, n)) for n in (X, Y, Z, V, OWN)}) == 5


@pytest.mark.parametrize("sid", [1, 8])
def test_rendered_once_then_two_new_origins(hosts, expected, sid):
    """A scene that has rendered one frame takes a batch at two NEW origins as one launch (the ordered
    batch may recompute the buffer the frame before it read)."""
    import torch
    with fresh(hosts, sid) as (gs,):
        single(torch, expected, gs, sid, OWN, "own", with_hits=True)
        before = counters(gs)
        batch(torch, expected, [(gs, sid, Z), (gs, sid, V)], "batch")
        after = counters(gs)
        assert (after[0] - before[0], after[1] - before[1]) == (1, 0)


@pytest.mark.parametrize("sid", [1, 8])
def test_two_origin_batches_then_single_then_batch(hosts, expected, sid):
    """[X, Y], [Z, V], one frame at the own camera, [X, Y] again: both buffers are the last launch's after
    each batch, and every later launch still finds one."""
    import torch
    with fresh(hosts, sid) as (gs,):
        before = counters(gs)
        batch(torch, expected, [(gs, sid, X), (gs, sid, Y)], "step 0")
        batch(torch, expected, [(gs, sid, Z), (gs, sid, V)], "step 1")
        single(torch, expected, gs, sid, OWN, "step 2")
        batch(torch, expected, [(gs, sid, X), (gs, sid, Y)], "step 3")
        after = counters(gs)
        assert (after[0] - before[0], after[1] - before[1]) == (3, 0)


@pytest.mark.parametrize("nlaunch", [1, 2])
@pytest.mark.parametrize("sid", [1, 8])
def test_host_tiled_after_two_origin_batch(hosts, expected, sid, nlaunch):
    """rt_render_frame_host_tiled at a third origin after a two-origin batch (its full wait frees both
    buffers), in one and in two row-band launches: the tile buffers reassemble to the view's frame."""
    import torch
    with fresh(hosts, sid) as (gs,):
        batch(torch, expected, [(gs, sid, X), (gs, sid, Y)], "batch")
        pf = rtm.PinnedFrame(W, H)
        try:
            flat = pf.array.reshape(-1)
            flat[:] = 0xDEADBEEF
            gs.render_frame_host_tiled(frame_of(gs, expected, sid, Z), pf, 12, 9, nlaunch)
            gs.wait_rows(H)
            img = np.zeros((H, W), np.uint32)
            for (x0, y0, x1, y1), t in zip(rtm.framebuffer_tiles(W, H), rtm.tile_views(flat, W, H)):
                img[y0:y1, x0:x1] = t
            assert sha(img) == expected[(sid, Z)]["bgra_sha256"]
        finally:
            pf.close()
        batch(torch, expected, [(gs, sid, V), (gs, sid, X)], "after")


@pytest.mark.parametrize("order", [(X, X, Y), (X, Y, X)], ids=["XXY", "XYX"])
@pytest.mark.parametrize("sid", [1, 8])
def test_repeat_within_a_batch(hosts, expected, sid, order):
    """Three frames of one scene at TWO origins: no error, every frame right, and each call is exactly one
    of a batched launch or a documented fallback."""
    import torch
    with fresh(hosts, sid) as (gs,):
        for rep in range(2):
            before = counters(gs)
            batch(torch, expected, [(gs, sid, n) for n in order], rep)
            after = counters(gs)
            assert (after[0] - before[0]) + (after[1] - before[1]) == 1, (before, after)


@pytest.mark.parametrize("sid", [1, 8])
def test_three_origins_in_one_batch_fall_back(hosts, expected, sid):
    """Three origins of one scene cannot share a launch (two buffers): the call falls back to a launch per
    frame, as rt_render_batch_device documents, and the scene batches again right after."""
    import torch
    with fresh(hosts, sid) as (gs,):
        before = counters(gs)
        batch(torch, expected, [(gs, sid, X), (gs, sid, Y), (gs, sid, Z)], "three")
        mid = counters(gs)
        assert (mid[0] - before[0], mid[1] - before[1]) == (0, 1)
        batch(torch, expected, [(gs, sid, V), (gs, sid, X)], "two")
        after = counters(gs)
        assert (after[0] - mid[0], after[1] - mid[1]) == (1, 0)


def test_another_scene_in_between(hosts, expected):
    """[A@X, B@X, A@Y] then [B@Z, A@Z, B@V] (A: killeroo, B: Cornell box): a scene's frames are not
    neighbours in the batch, and each scene is the repeated one once."""
    import torch
    with fresh(hosts, 8, 1) as (a, b):
        before = counters(a), counters(b)
        batch(torch, expected, [(a, 8, X), (b, 1, X), (a, 8, Y)], "step 0")
        batch(torch, expected, [(b, 1, Z), (a, 8, Z), (b, 1, V)], "step 1")
        after = counters(a), counters(b)
        # each chunk is led by (and counted on) its first frame's scene
        assert [(x[0] - y[0], x[1] - y[1]) for x, y in zip(after, before)] == [(1, 0), (1, 0)]


@pytest.mark.parametrize("sid", [1, 8])
def test_records_of_two_origin_batches(hosts, expected, sid):
    """rt_render_records_device with [X, Y] and then [Z, V], full-frame rectangles: every sample's record
    columns and the frames equal the views'."""
    import torch
    with fresh(hosts, sid) as (gs,):
        for pair in ((X, Y), (Z, V)):
            fs = [frame_of(gs, expected, sid, n) for n in pair]
            outs, recs = product_records(torch, [gs, gs], fs, [(0, 0, W, H)] * 2)
            torch.cuda.synchronize()
            for n, o, r in zip(pair, outs, recs):
                expect(expected[(sid, n)], shas(host(r)))
                assert sha_dev(o) == expected[(sid, n)]["bgra_sha256"], n


def test_sharded_ranks_of_8(hosts, expected):
    """[X, Y], [Z, V] and a single own-camera frame of killeroo as 8 ranks' shard launches (the wide section
    leads each batch), every rank rendered and unsharded: frames and hit IDs equal the fixtures'."""
    import torch
    sid, N = 8, 8
    e = rtm.shard_elems(W, H, N)
    st = torch.cuda.current_stream().cuda_stream
    full = torch.zeros(W * H, dtype=torch.int32, device="cuda")

    def check(names, outs, hits, label):
        torch.cuda.synchronize()
        for n, o, h in zip(names, outs, hits):
            full.fill_(SENT)
            rtm.unshard_device(W, H, N, o.data_ptr(), full.data_ptr(), st)
            torch.cuda.synchronize()
            assert sha_dev(full) == expected[(sid, n)]["bgra_sha256"], (label, n)
            assert sha_dev(h) == expected[(sid, n)]["hits_sha256"], (label, n)

    with fresh(hosts, sid) as (gs,):
        for step, pair in enumerate(((X, Y), (Z, V))):
            outs, hits = buffers(torch, 2, N * e)
            fs = [frame_of(gs, expected, sid, n) for n in pair]
            for r in range(N):
                rtm.render_batch_device([gs, gs], fs, [o.data_ptr() + 4 * r * e for o in outs], rank=r, nranks=N,
                                        d_hits=[h.data_ptr() for h in hits], stream=st)
            check(pair, outs, hits, step)
        outs, hits = buffers(torch, 1, N * e)
        f = frame_of(gs, expected, sid, OWN)
        for r in range(N):
            gs.render_hits_device(f, r, N, outs[0].data_ptr() + 4 * r * e, hits[0].data_ptr(), st)
        check((OWN,), outs, hits, 2)


def test_two_streams_rotating_origin_pairs(hosts, expected):
    """Ten batched steps of killeroo, each a pair of the five origins that recomputes at least one buffer,
    every frame asking to overlap (RT_KERNEL_FLAG_OVERLAP), the steps alternating over two streams with no
    synchronisation between them.  A two-origin batch owns both buffers, so the library must refuse the
    overlap and order each step after the one before it on the OTHER stream: a recompute that did not wait
    for that step's reader shows up as a wrong frame.  Every step's frames and hit IDs are compared."""
    import torch
    sid = 8
    steps = [(X, Y), (Z, V), (OWN, X), (X, Z), (V, OWN), (Y, V), (Z, X), (OWN, Y), (Y, Z), (V, X)]
    held = set()
    for pair in steps:                  # (the premise: an origin that neither buffer holds is recomputed)
        assert len(set(pair)) == 2 and not set(pair) <= held
        held = set(pair)
    with fresh(hosts, sid) as (gs,):
        flag = rtm.RT_KERNEL_AUTO | rtm.RT_KERNEL_FLAG_OVERLAP
        fs = {n: frame_of(gs, expected, sid, n, kernel=flag) for n in (X, Y, Z, V, OWN)}
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        bufs = [buffers(torch, 2) for _ in steps]
        torch.cuda.synchronize()        # (the fills run on torch's stream, not on these)
        before = counters(gs)
        for j, pair in enumerate(steps):
            outs, hits = bufs[j]
            rtm.render_batch_device([gs, gs], [fs[n] for n in pair], [o.data_ptr() for o in outs],
                                    d_hits=[h.data_ptr() for h in hits], stream=streams[j % 2].cuda_stream)
        torch.cuda.synchronize()
        after = counters(gs)
        assert (after[0] - before[0], after[1] - before[1]) == (len(steps), 0)
        for j, pair in enumerate(steps):
            for n, o, h in zip(pair, *bufs[j]):
                assert sha_dev(o) == expected[(sid, n)]["bgra_sha256"], (j, n)
                assert sha_dev(h) == expected[(sid, n)]["hits_sha256"], (j, n)
