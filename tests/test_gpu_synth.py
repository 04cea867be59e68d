"""Every render kernel against the REFERENCE's own code on scenes that are none of the ten shipped ones.

Fixtures: tests/golden/synth and synth.json (oracle/gen_golden_synth.py, from oracle/_ref/refdriver*; the
scenes are described in tests/synth_scenes.py).  What the shipped scenes never reach and these do: a cell of
1,500 references (>= wg64_max_refs and wh_auto_refs, still packable) and one of 2,100 (not packable: AUTO
falls back to kVarAutoCore | kVarFastRcp over the plain CSR walk, COMPACT to its distance-skip arm), rays
with one and with two exactly-zero direction components through long empty runs, eyes exactly on a grid face
and on an interior cell plane, grids one cell thick on one or two axes, a mesh wholly in negative coordinates,
coordinates scaled by 1500 and by 0.02, degenerate triangles and NaN colours.

Bar: bit-exact, for frames, per-sample hit IDs and every record column.  Floats that may be NaN
(zero_normals) compare NaN == NaN whatever the payload (conftest.nan_equal_bits explains why).
Every output buffer is pre-filled with 0x5A5A5A5A, which no fixture contains, so a word the kernels leave
unwritten fails the comparison.  62x46x4 and 63x47x4 frames: each case takes well under a second.
"""
import hashlib

import numpy as np
import pytest

import synth_scenes as S
from conftest import ALT_REC_DTYPE, ISECT, load_package

pytestmark = pytest.mark.gpu
rtm = load_package()
META = S.meta()
CASES = sorted(META["cases"])
KERNELS = {"auto": rtm.RT_KERNEL_AUTO, "lanes": rtm.RT_KERNEL_LANES, "pixel_loop": rtm.RT_KERNEL_PIXEL_LOOP,
           "compact": rtm.RT_KERNEL_COMPACT, "auto_wide": rtm.RT_KERNEL_AUTO | rtm.RT_KERNEL_FLAG_WIDE_HEAVY}


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("synth")
    cache = {}

    def get(entry):
        key = entry["scene"]
        if key not in cache:
            hs = rtm.HostScene.load(S.scene_file(entry, tmp))
            cache[key] = (hs, rtm.GpuScene(hs, 0))
        return cache[key]
    yield get
    for hs, gs in cache.values():
        gs.close()
        hs.close()


def sentinel(torch, n):
    return torch.full((n,), S.SENTINEL, dtype=torch.int32, device="cuda")


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def frames_of(e):
    return [e] + ([e["axis_frame"]] if "axis_frame" in e else [])


def expect_frame(got, e, what):
    """got: u32 [W H]; against the stored frame (a mismatch is printed per pixel) and its SHA."""
    ref = S.read_synth(e["bgra"], "<u4")
    assert not (ref == S.SENTINEL).any()
    np.testing.assert_array_equal(got.reshape(-1), ref, err_msg=f"{e['name']} {what}")
    assert hashlib.sha256(got.tobytes()).hexdigest() == e["bgra_sha256"]


def product_records(torch, gs, f, rank=0, nranks=1, out=None, rec=None):
    """rt_render_records_device over the whole frame: (frame or shard tensor, records tensor).  A rank of N
    writes its own tiles' records, frame-absolute, into rec."""
    Wd, Ht, spp = f.width, f.height, f.spp
    if out is None:
        out = sentinel(torch, Wd * Ht if nranks == 1 else rtm.shard_elems(Wd, Ht, nranks))
    if rec is None:
        rec = sentinel(torch, Wd * Ht * spp * S.REC_WORDS)
    rtm.render_records_device([gs], [f], [out.data_ptr()], [(0, 0, Wd, Ht)], [rec.data_ptr()], rank, nranks,
                              stream=torch.cuda.current_stream().cuda_stream)
    return out, rec


def expect_product_records(rec_t, e, what):
    rec = host_u32(rec_t).reshape(-1, S.REC_WORDS)
    assert not (rec[:, :3] == S.SENTINEL).any() and not (rec[:, 5:11] == S.SENTINEL).any(), f"{what}: unwritten records"
    assert (rec[:, 3] == 0xFFFFFFFF).all() and (rec[:, 4] == 0xFFFFFFFF).all()       # not counted by the product walks
    S.check_rec11(S.to_rec11(rec), e, cols=S.PRODUCT_COLS, what=what)


@pytest.mark.parametrize("name", CASES)
def test_frames_every_kernel(scenes, name):
    """The frame from RT_KERNEL_AUTO, LANES, PIXEL_LOOP, COMPACT and AUTO | WIDE_HEAVY, each twice (the second
    launch finds the per-origin records and the launch shape in place), through rt_render_frame_device."""
    import torch
    for e in frames_of(META["cases"][name]):
        hs, gs = scenes(e)
        for kname, k in KERNELS.items():
            f = gs.frame(e["W"], e["H"], e["spp"], kernel=k)
            for rep in range(2):
                out = sentinel(torch, e["W"] * e["H"])
                gs.render_frame_device(f, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                expect_frame(host_u32(out), e, f"{kname} launch {rep}")


@pytest.mark.parametrize("name", CASES)
def test_hit_ids(scenes, name):
    """rt_render_hits_device: the frame and the per-sample hit triangle (0xFFFFFFFF on a miss)."""
    import torch
    for e in frames_of(META["cases"][name]):
        hs, gs = scenes(e)
        n = e["W"] * e["H"]
        out, hits = sentinel(torch, n), sentinel(torch, n * e["spp"])
        gs.render_hits_device(gs.frame(e["W"], e["H"], e["spp"]), 0, 1, out.data_ptr(), hits.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        expect_frame(host_u32(out), e, "hits launch")
        assert hashlib.sha256(host_u32(hits).tobytes()).hexdigest() == e["hits_sha256"], e["name"]


@pytest.mark.parametrize("name", CASES)
def test_debug_records(scenes, name):
    """rt_trace_samples (the plain cell-by-cell walk, which counts): all 11 columns, DDA steps and
    ray/triangle tests included."""
    for e in frames_of(META["cases"][name]):
        hs, gs = scenes(e)
        rec = gs.trace_samples(gs.frame(e["W"], e["H"], e["spp"]), 0, 0, e["W"], e["H"])
        S.check_rec11(S.to_rec11(rec), e, what="rt_trace_samples")


@pytest.mark.parametrize("nranks", [1, 2, 8])
@pytest.mark.parametrize("name", CASES)
def test_product_records(scenes, name, nranks):
    """rt_render_records_device (the benchmarked launch path) at 1, 2 and 8 ranks, every rank: words hit,
    tri, voxel, t, u, v, r, g, b of every sample; the ranks' shards unsharded give the frame."""
    import torch
    for e in frames_of(META["cases"][name]):
        hs, gs = scenes(e)
        Wd, Ht = e["W"], e["H"]
        f = gs.frame(Wd, Ht, e["spp"])
        rec = None
        shards = []
        for r in range(nranks):
            out, rec = product_records(torch, gs, f, r, nranks, rec=rec)
            shards.append(out)
        torch.cuda.synchronize()
        expect_product_records(rec, e, f"rank of {nranks}")
        if nranks == 1:
            expect_frame(host_u32(shards[0]), e, "records launch")
        else:
            full = sentinel(torch, Wd * Ht)
            gathered = torch.cat(shards)
            rtm.unshard_device(Wd, Ht, nranks, gathered.data_ptr(), full.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            expect_frame(host_u32(full), e, f"unsharded rank of {nranks}")


@pytest.mark.parametrize("name", S.BARY_ALT)
def test_bary_brute_march(scenes, name):
    """The second ray/triangle test (IntersectRayTriBarycentric) through the lane, pixel-loop and compaction
    kernels and the debug records; brute force and the ray march on their windows."""
    import torch
    b = dict(META["bary_alt"][name]["bary"], scene=name)
    hs, gs = scenes(b)
    n = S.W * S.H
    out, hits = sentinel(torch, n), sentinel(torch, n * S.SPP)
    fb = gs.frame(S.W, S.H, S.SPP, tri_test=rtm.RT_TRI_BARYCENTRIC)
    gs.render_hits_device(fb, 0, 1, out.data_ptr(), hits.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert hashlib.sha256(host_u32(out).tobytes()).hexdigest() == b["bgra_sha256"]
    assert hashlib.sha256(host_u32(hits).tobytes()).hexdigest() == b["hits_sha256"]
    for k in (rtm.RT_KERNEL_LANES, rtm.RT_KERNEL_PIXEL_LOOP, rtm.RT_KERNEL_COMPACT):
        img = gs.render_frame(gs.frame(S.W, S.H, S.SPP, tri_test=rtm.RT_TRI_BARYCENTRIC, kernel=k))
        assert hashlib.sha256(img.tobytes()).hexdigest() == b["bgra_sha256"], k
    S.check_rec11(S.to_rec11(gs.trace_samples(fb, 0, 0, S.W, S.H)), b, what="bary rt_trace_samples")
    for mode in ("brute", "march"):
        a = META["bary_alt"][name][mode]
        f = gs.frame(S.W, S.H, S.SPP, intersector=ISECT[mode])
        got = gs.trace_samples(f, a["x0"], a["y0"], a["w"], a["h"])
        S.check_alt(got, S.read_synth(a["rec"], ALT_REC_DTYPE), mode, f"{name} {mode}")


@pytest.mark.parametrize("name", S.BIG)
def test_big_frames(scenes, name):
    """1920x1080x2 (16,200 workgroups, above wg64_min_blocks and hf_min_blocks): three frames through
    rt_render_frame_device (the first in natural block order, then heavy-first; one-wave workgroups for
    `inside`, 256-lane ones for stack1500, whose cell of 1,500 is >= wg64_max_refs), the hit IDs, and eight
    frames with RT_KERNEL_FLAG_OVERLAP on two alternating streams (one-wave workgroups for both)."""
    import torch
    b = META["big"][name]
    hs, gs = scenes({"scene": name})
    Wd, Ht, spp = b["W"], b["H"], b["spp"]
    f = gs.frame(Wd, Ht, spp)
    st = torch.cuda.current_stream().cuda_stream
    for i in range(3):
        out = sentinel(torch, Wd * Ht)
        gs.render_frame_device(f, out.data_ptr(), st)
        torch.cuda.synchronize()
        assert hashlib.sha256(host_u32(out).tobytes()).hexdigest() == b["bgra_sha256"], (name, i)
    out, hits = sentinel(torch, Wd * Ht), sentinel(torch, Wd * Ht * spp)
    gs.render_hits_device(f, 0, 1, out.data_ptr(), hits.data_ptr(), st)
    torch.cuda.synchronize()
    assert hashlib.sha256(host_u32(out).tobytes()).hexdigest() == b["bgra_sha256"]
    assert hashlib.sha256(host_u32(hits).tobytes()).hexdigest() == b["hits_sha256"]
    fo = gs.frame(Wd, Ht, spp, kernel=rtm.RT_KERNEL_AUTO | rtm.RT_KERNEL_FLAG_OVERLAP)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [sentinel(torch, Wd * Ht) for _ in range(8)]
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        gs.render_frame_device(fo, o.data_ptr(), streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert hashlib.sha256(host_u32(o).tobytes()).hexdigest() == b["bgra_sha256"], (name, "overlap", i)


@pytest.mark.parametrize("nranks", [2, 8])
def test_wide_section_on_a_cell_of_1500(nranks, monkeypatch, tmp_path):
    """stack1500 at a rank of 2 and of 8: max_cell_refs 1500 >= wh_auto_refs, so AUTO's shard launches take
    the wide section by themselves.  Frames are rendered (every rank; the records of every sample compared
    with the reference's for every frame) until gs.wide_tiers() reports items in the G-lane tier at a rank of
    2, in the LDS tier at a rank of 8, and three more frames have run with them; 20 frames at the most, else
    the test fails.

    Which knobs: the frame is 256x144x4 (2,304 work items; the 62x46 one has 16 or 32 per rank of 8), and the
    thresholds are set with RT_WH_FLOOR / RT_WH_ALPHA16 / RT_WH_BETA16, which are read once at scene creation
    (hence a scene of this test's own).  k_hf_plan lists an item in the G-lane tier above
    max(floor, sum of item costs * alpha16 / (16 * 8192)) cycles and in the LDS tier between that and
    max(floor, the same with beta16): alpha16 = 16 * 8192 / (items per rank) puts the first threshold at the
    MEAN item cost, beta16 = 0 and floor = 1 the second at one cycle.  The frame's items are a few heavy
    ones (the cell of 1,500) among many cheap ones, so whatever the cycle counts are, the heavy ones are
    above the mean and the cheap ones between the thresholds."""
    import torch
    e = META["wide"]
    Wd, Ht, spp = S.WIDE_FRAME
    # work items: a 16x16 tile at spp 4 is 4 workgroups of 4 waves, each wave an item
    items = ((Wd + 15) // 16) * ((Ht + 15) // 16) * spp * 4 // nranks
    monkeypatch.setenv("RT_WH_ALPHA16", str(16 * 8192 // items))
    monkeypatch.setenv("RT_WH_BETA16", "0")
    monkeypatch.setenv("RT_WH_FLOOR", "1")
    hs = rtm.HostScene.load(S.gunzip_scene("stack1500", tmp_path))
    gs = rtm.GpuScene(hs, 0)
    try:
        info = gs.info()
        assert info["max_cell_refs"] == 1500 and info["max_cell_refs"] >= info["wh_auto_refs"], info
        assert info["packed_cells"] == 1 and info["box_words"] == 1 and info["rcp_safe"] == 1, info
        f = gs.frame(Wd, Ht, spp)
        listed = lds = with_tier = 0
        rec = None
        for frame in range(20):
            for r in range(nranks):
                _, rec = product_records(torch, gs, f, r, nranks, rec=rec)
            torch.cuda.synchronize()
            expect_product_records(rec, e, f"rank of {nranks} frame {frame}")
            rec.fill_(S.SENTINEL)
            if (listed if nranks == 2 else lds):
                with_tier += 1              # (this frame ran with the tier filled, and compared equal)
                if with_tier == 3:
                    break
            listed, lds = gs.wide_tiers()
        print(f"rank of {nranks}: wide_tiers (G-lane, LDS) = {(listed, lds)} after {frame + 1} frames")
        if nranks == 8:
            assert lds > 0, "the LDS tier never filled"
        else:
            assert listed > 0, "the G-lane tier never filled"
    finally:
        gs.close()
        hs.close()


@pytest.mark.parametrize("scene", S.CAM_SCENES)
def test_seeded_cameras(scenes, oracle, scene, tmp_path):
    """Sixteen seeded cameras per scene (the six exact axis directions, two eyes inside the grid, two on a
    grid face, one looking away, five random) at 96x54x4: AUTO's frame and hit IDs against the reference's
    SHAs, and first against the live CPU restatement so that a mismatch is printed per pixel."""
    import torch
    hs, gs = scenes({"scene": scene})
    osc = S.OracleScene(oracle, S.scene_file({"scene": scene}, tmp_path))
    try:
        for v in [v for v in META["cameras"].values() if v["scene"] == scene]:
            cam, fov = S.bits_f32(v["cam_bits"]), float(S.bits_f32([v["fov_bits"]])[0])
            f = gs.frame(v["W"], v["H"], v["spp"])
            for k in range(16):
                f.cam[k] = float(cam[k])
            f.fov = fov
            n = v["W"] * v["H"]
            out, hits = sentinel(torch, n), sentinel(torch, n * v["spp"])
            gs.render_hits_device(f, 0, 1, out.data_ptr(), hits.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            img, hid = osc.render(v["W"], v["H"], v["spp"], cam=cam, fov=fov)
            np.testing.assert_array_equal(host_u32(out).reshape(v["H"], v["W"]), img, err_msg=f"{scene} {v['view']}")
            np.testing.assert_array_equal(host_u32(hits), hid, err_msg=f"{scene} {v['view']} hit ids")
            assert hashlib.sha256(host_u32(out).tobytes()).hexdigest() == v["bgra_sha256"], v["view"]
            assert hashlib.sha256(host_u32(hits).tobytes()).hexdigest() == v["hits_sha256"], v["view"]
    finally:
        osc.close()
