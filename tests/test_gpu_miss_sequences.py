"""The miss skip's host logic across SEQUENCES of frames (ensure_miss_mask / miss_launched, csrc/rt_launch.hip;
DESIGN.md §4.32; harness: tests/miss_skip_cases.py).

A mask is keyed by the camera, the frame's shape and the version of the camera-space tables (tab_epoch: the field of
view and the sample table are not in the key themselves).  These tests change exactly what only tab_epoch keeps out
of a key match -- the field of view, the sample table -- call the entry points that rewrite the tables between two
masked frames, run a masked launch under the heavy-first block order and in the ten-frame batched launch, and deal
a scene with dense cells to 2 and 8 ranks.  Every frame is held to the CPU restatement (or the reference's golden
SHA-256 at 1920x1080x4), and wherever a mask is in use its flagged count must be the CPU checker's for that very
frame: a stale mask shows as wrong pixels or as another frame's count.
"""
import hashlib

import numpy as np
import pytest

import camera_matrices as cm
import miss_skip_cases as mk
from conftest import load_package

pytestmark = pytest.mark.gpu
rtm = load_package()
FOV = 45.0
CAM_A = ((1.8, 1.2, 5.0), (1.1, 0.6, 0.0))       # tests/test_gpu_miss_skip.py's
W, H = 96, 54
FOVS = (45, 45, 45, 30, 30, 30, 45, 45, 60, 60, 60)
RUN_ENDS = (2, 5, 10)                            # the last frame of each run of three
SHIPPED_FLAGGING = {0: 725, 1: 630, 4: 560, 6: 204}      # flagged at 256x144x4 (tests/test_gpu_miss_reach.py's table)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return mk.build_checker(tmp_path_factory.mktemp("missseq"))


@pytest.fixture(scope="module")
def grid64(oracle, tmp_path_factory):
    """(host scene, scene file, OracleScene, directory) of tests/test_gpu_miss_skip.py's 64-cell mesh"""
    tmp = tmp_path_factory.mktemp("missseq64")
    tris, res = mk.synth_meshes()["grid64"]
    hs = cm.host_scene(tris, rtm.look_at(*CAM_A), fov=FOV, grid_res=res)
    path = str(tmp / "grid64.rtscene")
    hs.save(path)
    osc = mk.oracle_scene(oracle, path)
    yield hs, path, osc, tmp
    osc.close()
    hs.close()


def tables():
    r = np.random.Generator(np.random.PCG64(20261022))
    return [r.uniform(-0.5, 0.5, (4, 2)).astype(np.float32),
            np.array([[-1.5, 0.75], [1.25, -2.0], [0.0, 0.0], [2.5, 1.5]], np.float32)]


# Flagged items (CPU checker before any GPU run), grid64, 96x54, CAM_A (336 items with a valid lane at spp 4, 672 at 8):
#   fov 45: 169 (spp 4), 351 (spp 8)   fov 30: 156, 312   fov 60: 191, 382
#   the seeded table: 169 / 156 / 194 (fov 45 / 30 / 60)   the table outside [-0.5, 0.5]: 152 / 121 / 168
RUNS = (0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3)          # the run each frame of FOVS belongs to
RUN_ALT = (0, 1, 1, 0)                           # which spp / table a run takes: the two 45-degree runs differ
PER_RUN = ("fov", "fov_spp", "fov_tables")       # one spp / table per run: the last frame of a run of three is masked
PER_FRAME = ("spp_per_frame", "tables_per_frame")


@pytest.mark.parametrize("mode", PER_RUN + PER_FRAME)
def test_fov_sequences(oracle, checker, grid64, mode):
    """One camera and shape, the field of view 45, 45, 45, 30, 30, 30, 45, 45, 60, 60, 60:

      fov          spp 4, the Hammersley table throughout
      fov_spp      spp 4, 8, 8, 4 for the four runs (8 after 4: the larger mask takes over a freed buffer and
                   reallocates it, ensure_miss_mask's `need > m.cap`)
      fov_tables   two caller-supplied sample tables, A, B, B, A for the four runs: nothing but tab_epoch tells the two
                   45-degree runs -- the same camera, shape and spp under different tables -- apart in a mask's key

    Every frame equals the oracle's; a frame that runs with a mask flags exactly what the checker flags for ITS field
    of view, spp and table; and the last frame of each run of three runs with its mask, flagged == the checker's > 0.

      spp_per_frame, tables_per_frame   the same alternations frame by frame.  Every frame changes the tables there,
                   so no key is requested twice and no frame gets a mask (the design's price); kept as a stale-mask
                   check: a key match that ignores the tables shows as another frame's count or as wrong pixels."""
    hs, path, osc, tmp = grid64
    skip = mk.gpu_scene(hs, True)
    cam = mk.cam16(CAM_A)
    tbls = tables()
    files = [mk.samples_file(tmp, f"seq{i}", t) for i, t in enumerate(tbls)]
    want, cpu = {}, {}
    try:
        seen, keys = [], []
        for i, fov in enumerate(FOVS):
            alt = RUN_ALT[RUNS[i]] if mode in PER_RUN else i % 2
            spp = (4, 8)[alt] if "spp" in mode else 4
            ti = alt if "tables" in mode else None
            key = (fov, spp, ti)
            if key not in want:
                tbl = None if ti is None else tbls[ti]
                want[key] = mk.oracle_frame(oracle, osc.h, W, H, spp, cam, fov, tbl)[0]
                cpu[key] = mk.cpu_mask(checker, path, W, H, spp, cam=cam, fov=fov,
                                       samples=None if ti is None else files[ti])["flagged"]
                assert cpu[key] > 0
            f = mk.frame(skip, W, H, spp, cam, fov=fov, offsets=None if ti is None else tbls[ti])
            got = skip.render_frame(f)
            flagged = skip.miss_mask()[0]
            seen.append(flagged)
            keys.append(key)
            print(mode, i, key, "flagged", flagged, "cpu", cpu[key])
            assert np.array_equal(got, want[key]), (mode, i, key)
            assert flagged in (0, cpu[key]), (mode, i, key, flagged, cpu[key])
        if mode in PER_RUN:
            assert all(seen[i] == cpu[keys[i]] > 0 for i in RUN_ENDS), seen
            assert len(set(cpu.values())) >= 3            # (the runs do flag different counts)
    finally:
        skip.close()


def test_other_entry_points_between_two_masked_frames(oracle, checker, grid64):
    """A masked frame F; then, at another shape and field of view, rt_primary_rays_device, rt_render_ao_device, a
    hit-ID frame, an RT_KERNEL_LANES frame and an RT_ISECT_RAY_MARCH frame -- each rewrites the camera-space tables
    F's mask was computed from --; F again gives the same bytes, and again after one more repetition, and settles
    on the same count."""
    import torch
    hs, path, osc, _ = grid64
    skip = mk.gpu_scene(hs, True)
    cam, spp = mk.cam16(CAM_A), 4
    try:
        exp = mk.oracle_frame(oracle, osc.h, W, H, spp, cam, FOV)[0]
        cpu = mk.cpu_mask(checker, path, W, H, spp, cam=cam)

        def render_f():
            return [skip.render_frame(mk.frame(skip, W, H, spp, cam))]
        (a,), flagged, used = mk.settle(render_f, skip)
        assert used >= 2 and flagged == cpu["flagged"] > 0
        assert np.array_equal(a, exp)
        w2, h2, fov2 = 64, 48, 30.0
        st = torch.cuda.current_stream().cuda_stream
        exp2, hid2 = mk.oracle_frame(oracle, osc.h, w2, h2, spp, cam, fov2)
        for what in ("primary_rays", "render_ao", "hits", "lanes", "march"):
            if what == "primary_rays":
                rays = skip.primary_rays(mk.frame(skip, w2, h2, spp, cam, fov=fov2))
                torch.cuda.synchronize()
                assert np.array_equal(rays.cpu().numpy().view(np.uint32),
                                      cm.generate_rays(cam, fov2, w2, h2, rtm.sample_table(spp)).view(np.uint32))
            elif what == "render_ao":
                skip.render_ao(mk.frame(skip, w2, h2, spp, cam, fov=fov2))
                torch.cuda.synchronize()
            elif what == "hits":
                out = torch.zeros(w2 * h2, dtype=torch.int32, device="cuda")
                hits = torch.zeros(w2 * h2 * spp, dtype=torch.int32, device="cuda")
                skip.render_hits_device(mk.frame(skip, w2, h2, spp, cam, fov=fov2), 0, 1, out.data_ptr(), hits.data_ptr(), st)
                torch.cuda.synchronize()
                assert np.array_equal(hits.cpu().numpy().view(np.uint32), hid2)
                assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(h2, w2), exp2)
            elif what == "lanes":
                assert np.array_equal(skip.render_frame(mk.frame(skip, w2, h2, spp, cam, rtm.RT_KERNEL_LANES, fov=fov2)), exp2)
            else:
                f = mk.frame(skip, w2, h2, spp, cam, fov=fov2)
                f.intersector = rtm.RT_ISECT_RAY_MARCH
                skip.render_frame(f)
            if what in ("hits", "lanes", "march"):       # (a render launch: rt_debug_miss_mask speaks of it)
                assert skip.miss_mask()[0] == 0, what
            for rep in range(2):
                assert np.array_equal(render_f()[0], exp), (what, rep)
                assert skip.miss_mask()[0] in (0, cpu["flagged"]), (what, rep)
        (a,), flagged, used = mk.settle(render_f, skip)
        assert np.array_equal(a, exp) and used >= 2 and flagged == cpu["flagged"]
    finally:
        skip.close()


# ------------------------------------------------------------------ the shipped scenes: plan order, batch of ten, shards
@pytest.fixture(scope="module")
def shipped():
    hss = [rtm.HostScene.load(sid) for sid in range(10)]
    gss = [mk.gpu_scene(hs, True) for hs in hss]
    yield hss, gss
    for g in gss:
        g.close()
    for h in hss:
        h.close()


@pytest.mark.parametrize("overlap", [False, True])
def test_heavy_first_order_with_a_mask_in_use(golden, checker, overlap):
    """Scene 4 (dense cells, 34,701 flagged items of 129,600) at 1920x1080x4: the same key rendered until a launch
    runs BOTH under a heavy-first block order with listed blocks (rt_debug_heavy_first: a front section, and a plan
    that lists blocks) and with its mask in use -- the front section renders the plan's heavy blocks first and the
    others skip them, while the mask is indexed by the launch's natural item order.  Every frame is the reference's
    (golden SHA-256); on one stream, and with RT_KERNEL_FLAG_OVERLAP on two."""
    import torch
    sid, Wd, Ht, spp = 4, 1920, 1080, 4
    hs = rtm.HostScene.load(sid)
    skip = mk.gpu_scene(hs, True)
    try:
        want = golden["frames_1080p4"][str(sid)]["bgra_sha256"]
        cpu = mk.cpu_mask(checker, rtm.scene_path(sid), Wd, Ht, spp)
        flag = rtm.RT_KERNEL_FLAG_OVERLAP if overlap else 0
        streams = [torch.cuda.Stream() for _ in range(2 if overlap else 1)]
        out = [torch.zeros(Wd * Ht, dtype=torch.int32, device="cuda") for _ in streams]
        both = 0
        for i in range(40):
            k = i % len(streams)
            # the plan this launch adopts was written by earlier frames; a shape's first two frames run in the natural
            # order whatever is listed, so only launches from the fourth on are counted
            front, listed, epoch = skip.heavy_first()
            if epoch < 3:
                listed = 0
            skip.render_frame_device(skip.frame(Wd, Ht, spp, kernel=rtm.RT_KERNEL_AUTO | flag), out[k].data_ptr(),
                                     streams[k].cuda_stream)
            if not overlap or i % 2:
                torch.cuda.synchronize()
                for o in out:
                    assert hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest() == want, i
                flagged = skip.miss_mask()[0]
                front1, listed1, _ = skip.heavy_first()
                assert flagged in (0, cpu["flagged"])
                both += flagged > 0 and front > 0 and listed > 0 and front1 > 0 and listed1 > 0
                if both >= 2:
                    break
        print("frames", i + 1, "heavy-first", skip.heavy_first(), "flagged", flagged)
        assert both >= 2, (skip.heavy_first(), flagged)
    finally:
        skip.close()
        hs.close()


@pytest.mark.parametrize("odd_camera", [False, True])
def test_batch_of_ten(oracle, checker, shipped, odd_camera):
    """All ten shipped scenes at 256x144x4 through rt_render_batch_device, repeated until every scene that can flag
    (0, 1, 4, 6) runs with its mask for a second batch; each frame equals the oracle's and each count the
    checker's.  odd_camera: scene 1's camera with its 3x3 times 1024 -- that frame loses the gate and kVarFastRcp,
    so the batch takes the per-frame fall-back (rt_scene_info.batch_fallbacks), masks included."""
    import torch
    hss, gss = shipped
    Wd, Ht, spp = 256, 144, 4
    st = torch.cuda.current_stream().cuda_stream
    cams = [np.asarray(hs.cam, np.float32).copy() for hs in hss]
    expect = dict(SHIPPED_FLAGGING)
    if odd_camera:
        cams[1] = cm.apply_factor(cams[1], np.eye(3) * 1024.0)
        expect[1] = mk.cpu_mask(checker, rtm.scene_path(1), Wd, Ht, spp, cam=cams[1])["flagged"]
        assert expect[1] == SHIPPED_FLAGGING[1]          # (a uniform scale moves no ray)
    want = [oracle.render_cam(sid, Wd, Ht, spp, cams[sid], hss[sid].fov)[0] for sid in range(10)]
    before = gss[0].info()["batch_fallbacks"]
    used = {sid: 0 for sid in expect}
    for rep in range(mk.SETTLE):
        outs = [torch.full((Wd * Ht,), cm.SENTINEL, dtype=torch.int32, device="cuda") for _ in gss]
        rtm.render_batch_device(gss, [mk.frame(g, Wd, Ht, spp, c) for g, c in zip(gss, cams)], [o.data_ptr() for o in outs],
                                stream=st)
        torch.cuda.synchronize()
        for sid, o in enumerate(outs):
            assert np.array_equal(o.cpu().numpy().view(np.uint32).reshape(Ht, Wd), want[sid]), (rep, sid)
            flagged = gss[sid].miss_mask()[0]
            assert flagged in (0, expect.get(sid, 0)), (rep, sid, flagged)
            if sid in used:
                used[sid] += flagged > 0
        if all(v >= 2 for v in used.values()):
            break
    print("batches", rep + 1, used)
    assert all(v >= 2 for v in used.values()), used
    fell_back = gss[0].info()["batch_fallbacks"] - before
    assert (fell_back == rep + 1) if odd_camera else (fell_back == 0), fell_back


@pytest.mark.parametrize("nranks", [2, 8])
def test_shards_of_a_scene_with_dense_cells(oracle, checker, shipped, nranks):
    """Scene 4 at 256x144x4 dealt to 2 and 8 ranks (AUTO takes the wide section for a shard of a scene with dense
    cells): each rank's shard settled on its mask, its count the checker's for that rank; the gathered frame is the
    oracle's."""
    import torch
    sid, Wd, Ht, spp = 4, 256, 144, 4
    skip = shipped[1][sid]
    st = torch.cuda.current_stream().cuda_stream
    e = rtm.shard_elems(Wd, Ht, nranks)
    gathered, total = [], 0
    for rank in range(nranks):
        def shard():
            o = torch.full((e,), cm.SENTINEL, dtype=torch.int32, device="cuda")
            skip.render_shard_device(skip.frame(Wd, Ht, spp), rank, nranks, o.data_ptr(), st)
            torch.cuda.synchronize()
            return [o.cpu().numpy()]
        cpu = mk.cpu_mask(checker, rtm.scene_path(sid), Wd, Ht, spp, rank=rank, nranks=nranks)
        (a,), flagged, used = mk.settle(shard, skip)
        print("rank", rank, "of", nranks, "flagged", flagged, "cpu", cpu)
        assert flagged == cpu["flagged"] and (used >= 2 or cpu["flagged"] == 0), (rank, flagged, cpu, used)
        total += flagged
        gathered.append(a)
    assert total == SHIPPED_FLAGGING[sid]            # the ranks' items are the frame's, each once
    g = torch.from_numpy(np.concatenate(gathered)).cuda()
    out = torch.zeros(Wd * Ht, dtype=torch.int32, device="cuda")
    rtm.unshard_device(Wd, Ht, nranks, g.data_ptr(), out.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(Ht, Wd), oracle.render(sid, Wd, Ht, spp)[0])
