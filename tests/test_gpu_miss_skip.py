"""The lane kernels' miss skip on the device (csrc/rt_miss_mask.h, k_miss_mask, process_item).

A work item whose 64 samples provably miss the grid box stores its row's all-miss word without tracing.  Every
synthetic frame below is rendered four ways and must be byte-equal: AUTO with the skip, AUTO on a scene created
with RT_MISS_SKIP=0 (no masks), RT_KERNEL_LANES (never skipped) -- and the oracle (the CPU restatement on the saved
scene file, tests/synth_scenes.py OracleScene), which shares no code with the device.  The synthetic scenes are a
one-cell grid and a 64-cell grid whose box outline crosses work items, tiles and the frame's edge; Cornell and
killeroo at the bench's spp are held against the oracle and the golden SHAs.  A key gets its mask at its second
request (a camera that moves every frame never pays for one), so a frame is rendered until its mask is in use
(`settled`); the debug count (rt_debug_miss_mask) must then equal what the CPU checker
(tests/miss_mask_check.cpp) flags -- a mask that silently stayed null would pass every comparison of pixels.
"""
import hashlib
import os

import numpy as np
import pytest

import camera_matrices as cm
import synth_scenes as ss
from conftest import ROOT, load_package
from miss_skip_cases import SETTLE, build_checker, cam16, cpu_mask, frame, gpu_scene, settled

pytestmark = pytest.mark.gpu
rtm = load_package()
SIZES = ((64, 48), (96, 54))
FOV = 45.0
CAM_A = ((1.8, 1.2, 5.0), (1.1, 0.6, 0.0))       # the box [-1, 1]^3 across the frame's left and lower edges
CAM_B = ((-2.5, 0.4, 4.0), (-0.6, -0.8, 0.0))
CAM_IN = ((0.2, 0.1, 0.3), (0.0, 0.0, -1.0))     # inside the box


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("missmask"))


@pytest.fixture(scope="module")
def synth(oracle, tmp_path_factory):
    """{name: (host scene, GpuScene with the skip, GpuScene without, OracleScene, scene file)}"""
    meshes = {"cell1": (np.concatenate([cm.facing_stack([0.1 * i for i in range(5)]), ss.anchors()]), 1),
              "grid64": (ss.sparse(20261020, n=40), 64)}
    tmp = tmp_path_factory.mktemp("missskip")
    out = {}
    for name, (tris, res) in meshes.items():
        hs = cm.host_scene(tris, rtm.look_at(*CAM_A), fov=FOV, grid_res=res)
        path = str(tmp / f"{name}.rtscene")
        hs.save(path)
        out[name] = (hs, gpu_scene(hs, True), gpu_scene(hs, False), ss.OracleScene(oracle, path), path)
    yield out
    for hs, a, b, o, _ in out.values():
        o.close()
        a.close()
        b.close()
        hs.close()


def four_ways(sc, W, H, spp, cam):
    """The frame with the skip (settled), without, by RT_KERNEL_LANES and by the oracle: (image, flagged)."""
    _, skip, plain, osc, _ = sc
    (a,), flagged = settled(lambda: [skip.render_frame(frame(skip, W, H, spp, cam))], skip)
    b = plain.render_frame(frame(plain, W, H, spp, cam))
    assert plain.miss_mask() == (0, 0)
    c = skip.render_frame(frame(skip, W, H, spp, cam, kernel=rtm.RT_KERNEL_LANES))
    assert skip.miss_mask()[0] == 0          # the LANES arm takes no mask
    exp, _ = osc.render(W, H, spp, cam=cam16(cam), fov=FOV)
    assert np.array_equal(a, b), "RT_MISS_SKIP=0"
    assert np.array_equal(a, c), "RT_KERNEL_LANES"
    assert np.array_equal(a, exp), "oracle"
    return a, flagged


@pytest.mark.parametrize("spp", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("name", ["cell1", "grid64"])
def test_frames_equal_the_unskipped_arms_and_the_oracle(synth, checker, name, spp):
    for W, H in SIZES:
        for cam in (CAM_A, CAM_B):
            a, flagged = four_ways(synth[name], W, H, spp, cam)
            cpu = cpu_mask(checker, synth[name][4], W, H, spp, cam=cam16(cam))
            print(name, W, H, spp, "flagged", flagged, "cpu", cpu)
            assert flagged == cpu["flagged"] > 0, (W, H, cam)
            assert (a != a[:, :1]).any()     # ... and the box is in the frame: not every pixel is its row's miss word


def test_camera_inside_the_box_takes_no_mask(synth):
    a, flagged = four_ways(synth["grid64"], 96, 54, 4, CAM_IN)
    assert flagged == 0 and synth["grid64"][1].miss_mask()[1] >= 0


@pytest.mark.parametrize("name", ["cell1", "grid64"])
def test_unaligned_regions(synth, checker, name):
    _, skip, plain, osc, path = synth[name]
    rects = [(5, 3, 61, 47), (17, 9, 64, 48), (0, 0, 33, 17), (31, 30, 96, 54)]
    for W, H in SIZES:
        exp, _ = osc.render(W, H, 4)
        for r in [r for r in rects if r[2] <= W and r[3] <= H]:
            (a,), flagged = settled(lambda: skip.render_tiles(frame(skip, W, H, 4), [r]), skip)
            b = plain.render_tiles(frame(plain, W, H, 4), [r])[0]
            c = skip.render_tiles(frame(skip, W, H, 4, kernel=rtm.RT_KERNEL_LANES), [r])[0]
            assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, exp[r[1]:r[3], r[0]:r[2]]), r
            assert flagged == cpu_mask(checker, path, W, H, 4, rect=r)["flagged"], r


@pytest.mark.parametrize("nranks", [2, 3, 8])
def test_shards(synth, nranks):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    for name in ("cell1", "grid64"):
        _, skip, plain, osc, _ = synth[name]
        W, H = 96, 54
        e = rtm.shard_elems(W, H, nranks)
        total = 0
        gathered = []
        for rank in range(nranks):
            def shard(gs):
                o = torch.full((e,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                gs.render_shard_device(frame(gs, W, H, 4), rank, nranks, o.data_ptr(), st)
                torch.cuda.synchronize()
                return [o.cpu().numpy()]
            (a,), flagged = settled(lambda: shard(skip), skip)
            total += flagged
            assert np.array_equal(a, shard(plain)[0]), (name, rank)
            gathered.append(a)
        assert total > 0
        # the ranks' shards, put together, are the oracle's frame
        g = torch.from_numpy(np.concatenate(gathered)).cuda()
        out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        rtm.unshard_device(W, H, nranks, g.data_ptr(), out.data_ptr(), st)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(H, W), osc.render(W, H, 4)[0]), name


def test_tiled_host_frame(synth):
    """rt_render_frame_host_tiled in one launch and in three row bands (three keys for two buffers: two bands
    settle on masks, the third stays unmasked -- no mask is recomputed per frame)."""
    _, skip, plain, osc, _ = synth["grid64"]
    W, H = 96, 54
    exp, _ = osc.render(W, H, 4)
    pf = rtm.PinnedFrame(W, H)
    try:
        flat = pf.array.reshape(-1)

        def tiled(gs, nl):
            flat[:] = 0xDEADBEEF
            gs.render_frame_host_tiled(frame(gs, W, H, 4), pf, 12, 9, nl)
            gs.wait_rows(H)
            img = np.zeros((H, W), np.uint32)
            for (x0, y0, x1, y1), t in zip(rtm.framebuffer_tiles(W, H), rtm.tile_views(flat, W, H)):
                img[y0:y1, x0:x1] = t
            return [img]
        assert np.array_equal(tiled(plain, 3)[0], exp)
        (a,), flagged = settled(lambda: tiled(skip, 1), skip)
        assert np.array_equal(a, exp) and flagged > 0
        before = skip.miss_mask()[1]
        for _ in range(SETTLE):
            assert np.array_equal(tiled(skip, 3)[0], exp)
        mid = skip.miss_mask()[1]
        for _ in range(6):
            assert np.array_equal(tiled(skip, 3)[0], exp)
        assert before < mid == skip.miss_mask()[1]       # bands got masks, and then none was computed again
    finally:
        pf.close()


def test_batches_of_two_cameras_and_two_scenes(synth):
    import torch
    W, H = 96, 54
    st = torch.cuda.current_stream().cuda_stream
    c1, c2 = synth["cell1"], synth["grid64"]
    cases = {"two cameras": ([c2, c2], [CAM_A, CAM_B]), "two scenes": ([c1, c2], [CAM_A, CAM_A])}
    for what, (scs, cams) in cases.items():
        def batch(gss):
            outs = [torch.full((W * H,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in gss]
            rtm.render_batch_device(gss, [frame(g, W, H, 4, c) for g, c in zip(gss, cams)], [o.data_ptr() for o in outs],
                                    stream=st)
            torch.cuda.synchronize()
            return [o.cpu().numpy().view(np.uint32).reshape(H, W) for o in outs]
        skips = [sc[1] for sc in scs]
        got, flagged = settled(lambda: batch(skips), skips[-1])
        assert flagged > 0, what
        for a, b, sc, c in zip(got, batch([sc[2] for sc in scs]), scs, cams):
            assert np.array_equal(a, b), what
            assert np.array_equal(a, sc[3].render(W, H, 4, cam=cam16(c), fov=FOV)[0]), what


@pytest.mark.parametrize("overlap", [False, True])
def test_camera_sequences_never_read_a_stale_mask(synth, overlap):
    """Cameras that stay for a few frames (masks are computed, kept, evicted: A, B, A, then C long enough to take a
    buffer), then a new camera every frame -- plain on one stream; overlapped on two streams, where a new mask may
    not go into the buffer the launch in flight reads.  A stale mask shows as wrong pixels."""
    import torch
    hs, _, plain, osc, _ = synth["grid64"]
    skip = gpu_scene(hs, True)           # (its own scene: the masks computed below are counted)
    W, H = 96, 54
    cam_c = ((0.5, 2.5, 4.5), (0.2, 1.0, 0.0))
    moving = [((1.8 - 0.4 * i, 1.2, 5.0 - 0.1 * i), (1.1 - 0.2 * i, 0.6, 0.0)) for i in range(1, 7)]
    eyes = [CAM_A] * 3 + [CAM_B] * 3 + [CAM_A] * 3 + [cam_c] * 14 + moving + [CAM_A, cam_c, cam_c]
    want = {}
    for c in eyes:
        if c not in want:
            want[c] = osc.render(W, H, 4, cam=cam16(c), fov=FOV)[0]
            assert np.array_equal(plain.render_frame(frame(plain, W, H, 4, c)), want[c])
    flag = rtm.RT_KERNEL_FLAG_OVERLAP if overlap else 0
    streams = [torch.cuda.Stream() for _ in range(2 if overlap else 1)]
    # (two rounds: the second finds the launch shape's plan context, so its frames do overlap)
    for rnd in range(2):
        outs = [torch.full((W * H,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in eyes]
        torch.cuda.synchronize()
        for i, c in enumerate(eyes):
            skip.render_frame_device(frame(skip, W, H, 4, c, kernel=rtm.RT_KERNEL_AUTO | flag), outs[i].data_ptr(),
                                     streams[i % len(streams)].cuda_stream)
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            assert np.array_equal(o.cpu().numpy().view(np.uint32).reshape(H, W), want[eyes[i]]), (rnd, i)
        flagged, computed = skip.miss_mask()
        assert flagged > 0                               # the last frame (camera C again) ran with its mask
    skip.close()
    assert 3 <= computed <= 6, computed                  # A, B, C in the first round, little after: not one per frame


def test_hit_ids_and_records_on_a_frame_with_flagged_items(synth):
    import torch
    _, skip, plain, osc, _ = synth["grid64"]
    W, H, spp = 96, 54, 4
    st = torch.cuda.current_stream().cuda_stream
    _, flagged = settled(lambda: [skip.render_frame(frame(skip, W, H, spp))], skip)
    assert flagged > 0                               # the plain frame of this camera does skip items
    res = []
    for gs in (skip, plain):
        out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        hits = torch.full((W * H * spp,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        gs.render_hits_device(frame(gs, W, H, spp), 0, 1, out.data_ptr(), hits.data_ptr(), st)
        torch.cuda.synchronize()
        assert gs.miss_mask()[0] == 0                # a frame that asks for hit IDs takes no mask
        out2 = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        recs = torch.full((W * H * spp * 12,), -1, dtype=torch.int32, device="cuda")
        rtm.render_records_device([gs], [frame(gs, W, H, spp)], [out2.data_ptr()], [(0, 0, W, H)], [recs.data_ptr()], stream=st)
        torch.cuda.synchronize()
        res.append([t.cpu().numpy() for t in (out, hits, out2, recs)])
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    exp, exp_hits = osc.render(W, H, spp)
    assert np.array_equal(res[0][0].view(np.uint32).reshape(H, W), exp)
    assert np.array_equal(res[0][1].view(np.uint32), exp_hits)
    assert (exp_hits == 0xFFFFFFFF).any() and (exp_hits != 0xFFFFFFFF).any()


@pytest.mark.parametrize("sid", [1, 8])
def test_bench_scenes_against_golden_and_the_cpu_count(golden, oracle, checker, sid):
    """The bench pair: 256x144x4 against the oracle, 1920x1080x4 against the reference's golden SHA; the frames of
    a shape share one mask, computed at the shape's second frame, and the device flags exactly the items the CPU
    checker does (killeroo: none, and its mask is dropped once its count is known)."""
    hs = rtm.HostScene.load(sid)
    gs = gpu_scene(hs, True)
    path = os.path.join(ROOT, "data", "scenes", f"scene{sid}.rtscene")
    try:
        for n, (W, H, spp) in enumerate(((256, 144, 4), (1920, 1080, 4))):
            cpu = cpu_mask(checker, path, W, H, spp)
            for rep in range(4):
                img = gs.render_frame(gs.frame(W, H, spp))
                flagged, computed = gs.miss_mask()
                print(sid, (W, H), rep, "gpu flagged", flagged, "computed", computed, "cpu", cpu)
                if H == 144:
                    assert np.array_equal(img, oracle.render(sid, W, H, spp)[0])
                else:
                    assert hashlib.sha256(img.tobytes()).hexdigest() == golden["frames_1080p4"][str(sid)]["bgra_sha256"]
                assert computed == n + (rep >= 1)               # one mask per frame shape, at its second frame
                assert flagged == (cpu["flagged"] if rep >= 1 else 0)
    finally:
        gs.close()
        hs.close()
