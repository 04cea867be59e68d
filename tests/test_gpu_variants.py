"""Every scene-dependent kernel choice, reached on purpose.

rt_scene_create derives four properties from the scene and the launcher picks its kernels from them
(render_device, rt_launch.hip; lanes_kernel, rt_kernels.hip):

  property (rt_scene_info)            false when                                  what changes
  packed_cells                        a cell of >= 2,048 references, or           no cell words at all: the plain CSR walk
                                      num_refs >= 2^21                            (cell_range, rt_walk.h) inside AUTO
  box_words (needs packed_cells)      num_refs >= 2^20 or > 16 M cells            no box runs: the distance-skip walk
  pack_ok                             a grid axis of more than 512 cells          RT_DDA_ADVANCE_ADD in the walk
  octant_words (needs packed_cells)   more than 2^23 cells                        L-inf words, oct_stride == 0
  rcp_safe                            |e1|_1 |e2|_1 >= 2^120 for a reference       the exact reciprocal

  AUTO instantiation                                      scenes
  kVarAuto (Core | FastRcp | PackedRem | SkipRun)         all four true: the ten shipped scenes
  kVarAutoCore | kVarFastRcp                              rcp_safe, but box_words or pack_ok false  (B1-B4)
  kVarAutoCore | kVarPackedRem | kVarSkipRun              box_words and pack_ok, not rcp_safe       (B5)
  kVarAutoCore                                            neither                                   (B5 on stack2100)
  COMPACT: kVarCompactBox when all hold, else kVarWaveGate | kVarDistSkip | kVarOriginPre (B1-B5)

Each case first asserts with gs.info() that the intended property holds -- otherwise it would quietly test
kVarAuto once more -- and then compares AUTO and COMPACT with RT_KERNEL_LANES and RT_KERNEL_PIXEL_LOOP (the plain
walks, pinned to the reference by test_gpu_parity.py and test_gpu_synth.py) exactly as
test_gpu_uniform_lists.check_against_plain_walk does: frames, the product kernel's records, rt_trace_samples.
Where the grid is the reference's (resolution 64), the live CPU restatement is compared as well.
64x64x4 frames with test_gpu_uniform_lists.OFFSETS: pixel (32, 32) sample 0 looks exactly down the camera axis.
One test per case, so that a fault can be attributed to one case.
"""
import os

import numpy as np
import pytest

import synth_scenes as S
from conftest import load_package, nan_equal_bits
from ray_variant_scenes import CallerBuilt
from test_gpu_uniform_lists import H, OFFSETS, REC_WORDS, SHARED_WORDS, SPP, W, check_against_plain_walk

pytestmark = pytest.mark.gpu
rtm = load_package()
FLOAT_WORDS = (5, 6, 7, 8, 9, 10)            # t, u, v, r, g, b of rt_sample_rec


class VScene:
    """A host scene (built here, or handed in) and its device copy; .look() moves the camera."""

    def __init__(self, tris=None, cam=None, grid_res=64, fov=45.0, host=None):
        if host is None:
            v, t = S.mesh_of(tris)
            host = rtm.HostScene.from_mesh(v, t, fov, cam, grid_res=grid_res)
        self.hs = host
        self.gs = rtm.GpuScene(host, 0)

    def look(self, cam):
        self.hs.cam = np.ascontiguousarray(cam, np.float32).reshape(16)

    def close(self):
        self.gs.close()
        if hasattr(self.hs, "close"):
            self.hs.close()


def expect_info(gs, **want):
    info = gs.info()
    got = {k: info[k] for k in want}
    print("info:", {k: info[k] for k in ("rcp_safe", "pack_ok", "box_words", "packed_cells", "octant_words",
                                         "max_cell_refs")})
    assert got == want, info
    return info


def render(gs, f):
    """rt_render_frame_device into a sentinel-filled buffer -> u32 [H, W]."""
    import torch
    out = torch.full((f.width * f.height,), S.SENTINEL, dtype=torch.int32, device="cuda")
    gs.render_frame_device(f, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(f.height, f.width)


def check_kernels(sc, nan_ok=False):
    """AUTO and COMPACT against LANES and PIXEL_LOOP: frames byte for byte (twice: the second AUTO launch finds
    its per-origin records in place), AUTO's product records and rt_trace_samples word for word
    (check_against_plain_walk; with nan_ok the float words compare NaN == NaN).  Returns AUTO's records."""
    import torch
    gs = sc.gs
    img = {}
    for name, k in (("lanes", rtm.RT_KERNEL_LANES), ("pixel_loop", rtm.RT_KERNEL_PIXEL_LOOP),
                    ("auto", rtm.RT_KERNEL_AUTO), ("compact", rtm.RT_KERNEL_COMPACT), ("auto again", rtm.RT_KERNEL_AUTO)):
        img[name] = render(gs, gs.frame(W, H, SPP, kernel=k, sample_offsets=OFFSETS))
        assert not (img[name] == S.SENTINEL).any(), f"{name}: pixels left unwritten"
    np.testing.assert_array_equal(img["pixel_loop"], img["lanes"], err_msg="PIXEL_LOOP vs LANES")
    for name in ("auto", "compact", "auto again"):
        np.testing.assert_array_equal(img[name], img["lanes"], err_msg=f"{name} vs LANES")
    if not nan_ok:
        return check_against_plain_walk(sc)
    f_auto = gs.frame(W, H, SPP, sample_offsets=OFFSETS)
    out = torch.full((W * H,), S.SENTINEL, dtype=torch.int32, device="cuda")
    rec = torch.full((W * H * SPP * REC_WORDS,), -1, dtype=torch.int32, device="cuda")
    rtm.render_records_device([gs], [f_auto], [out.data_ptr()], [(0, 0, W, H)], [rec.data_ptr()],
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32).reshape(H, W), img["lanes"])
    got = rec.cpu().numpy().view(np.uint32).reshape(-1, REC_WORDS)
    ref = gs.trace_samples(gs.frame(W, H, SPP, kernel=rtm.RT_KERNEL_LANES, sample_offsets=OFFSETS), 0, 0, W, H)
    ref = ref.view(np.uint32).reshape(-1, REC_WORDS)
    for w in SHARED_WORDS:
        if w in FLOAT_WORDS:
            assert nan_equal_bits(got[:, w].view(np.float32), ref[:, w].view(np.float32)), f"record word {w}"
        else:
            np.testing.assert_array_equal(got[:, w], ref[:, w], err_msg=f"record word {w}")
    assert (got[:, 3] == 0xFFFFFFFF).all() and (got[:, 4] == 0xFFFFFFFF).all()
    return got


def check_live_oracle(sc, oracle, tmp_path, name):
    """Resolution-64 grids: AUTO's and COMPACT's frames, AUTO's product records and rt_trace_samples (all
    columns) against the CPU restatement on the same scene file (Hammersley samples: the oracle takes no
    sample table)."""
    import torch
    path = os.path.join(str(tmp_path), name + ".rtscene")
    sc.hs.save(path)
    osc = S.OracleScene(oracle, path)
    try:
        img, _ = osc.render(W, H, SPP)
        exp = osc.records(W, H, SPP).view(np.uint32).reshape(-1, REC_WORDS)
    finally:
        osc.close()
    gs = sc.gs
    for k in (rtm.RT_KERNEL_AUTO, rtm.RT_KERNEL_COMPACT):
        np.testing.assert_array_equal(render(gs, gs.frame(W, H, SPP, kernel=k)), img, err_msg=f"kernel {k} vs oracle")
    f = gs.frame(W, H, SPP)
    out = torch.full((W * H,), S.SENTINEL, dtype=torch.int32, device="cuda")
    rec = torch.full((W * H * SPP * REC_WORDS,), -1, dtype=torch.int32, device="cuda")
    rtm.render_records_device([gs], [f], [out.data_ptr()], [(0, 0, W, H)], [rec.data_ptr()],
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = rec.cpu().numpy().view(np.uint32).reshape(-1, REC_WORDS)
    dbg = gs.trace_samples(f, 0, 0, W, H).view(np.uint32).reshape(-1, REC_WORDS)
    for w in SHARED_WORDS:
        np.testing.assert_array_equal(got[:, w], exp[:, w], err_msg=f"product record word {w} vs oracle")
    for w in range(11):
        np.testing.assert_array_equal(dbg[:, w], exp[:, w], err_msg=f"rt_trace_samples word {w} vs oracle")


def hits_and_misses(rec):
    assert (rec[:, 0] == 1).sum() >= 100 and (rec[:, 0] == 0).sum() >= 100, \
        ((rec[:, 0] == 1).sum(), (rec[:, 0] == 0).sum())


MID = 0.5 * (S.STACK_LO + S.STACK_HI)
STACK_CAM = S.axis_cam(2, -1, (MID, MID, 1.5))


# ------------------------------------------------------------------ B1
def test_b1_unpackable_stack2100(oracle, tmp_path):
    """A cell of 2,100 references: no cell words (packed_cells == 0, box_words == 0), so AUTO runs
    kVarAutoCore | kVarFastRcp over the plain CSR walk with cellw == nullptr."""
    sc = VScene(host=rtm.HostScene.load(S.gunzip_scene("stack2100", tmp_path)))
    try:
        expect_info(sc.gs, packed_cells=0, box_words=0, octant_words=0, rcp_safe=1, pack_ok=1, max_cell_refs=2100)
        hits_and_misses(check_kernels(sc))
        check_live_oracle(sc, oracle, tmp_path, "b1")
        sc.look(S.look((0.9, 0.7, 1.4), (MID, MID, MID)))          # oblique: the lists' cell is entered sideways
        check_kernels(sc)
    finally:
        sc.close()


@pytest.mark.parametrize("n", [2047, 2048])
def test_b1_packable_boundary(oracle, tmp_path, n):
    """A cell of exactly 2,047 references is the largest an 11-bit count holds (packable: this is the packable
    side of the pair, kVarAuto); one of exactly 2,048 is not."""
    sc = VScene(S.stack(n, 13), STACK_CAM, fov=2.0)
    try:
        assert sc.hs.stats["max_refs_per_cell"] == n
        p = int(n < 2048)
        expect_info(sc.gs, packed_cells=p, box_words=p, octant_words=p, rcp_safe=1, pack_ok=1, max_cell_refs=n)
        rec = check_kernels(sc)
        hits_and_misses(rec)
        assert (rec[rec[:, 0] == 1, 1] >= n - 64).any()            # the nearest triangles are the list's last
        check_live_oracle(sc, oracle, tmp_path, f"b1_{n}")
    finally:
        sc.close()


# ------------------------------------------------------------------ B2
def test_b2_packable_without_box_words():
    """num_refs in [2^20, 2^21): the cell words still pack (every cell under 2,048) but the box-run words,
    whose start field has 20 bits, are not built: the distance-skip walk with octant words and packed counts.
    (No triangle can overlap every cell of a grid, as the issue's sketch had it: 7,000 tilted sheets of
    about 150 cells each on a 16^3 grid give 1,067,456 references, at most 507 per cell.)"""
    sc = VScene(S.sheets(7000, 41), S.look((2.5, 1.8, 3.0), (0.0, 0.0, 0.0)), grid_res=16)
    try:
        nrefs = sc.hs.stats["num_refs"]
        assert (1 << 20) <= nrefs < (1 << 21) and sc.hs.stats["max_refs_per_cell"] < 2048, sc.hs.stats
        expect_info(sc.gs, packed_cells=1, box_words=0, octant_words=1, rcp_safe=1, pack_ok=1)
        hits_and_misses(check_kernels(sc))
        sc.look(S.axis_cam(0, -1, (3.0, 0.05, 0.03)))              # in the sheets' plane: long lists, late hits
        check_kernels(sc)
    finally:
        sc.close()


# ------------------------------------------------------------------ B3
@pytest.mark.parametrize("res", [512, 513])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_b3_pack_ok_boundary(axis, res):
    """A ribbon along one axis: res x 3 x 3 cells.  512 is the largest count the 11-bit fields of the packed
    remainders hold (pack_ok == 1: the packable side of the pair; the z count field of a box word has 9
    bits, rt_box_words.h); at 513 pack_ok == 0, so AUTO drops the box runs and RT_DDA_ADVANCE_ADD runs inside
    the distance-skip walk.  One view travels the whole long axis, the other crosses it."""
    thin = [k for k in range(3) if k != axis]
    eye = np.full(3, 0.005, np.float32)
    eye[axis] = 1.5
    sc = VScene(S.ribbon(axis, 50 + axis), S.axis_cam(axis, -1, eye), grid_res=res, fov=2.0)
    try:
        dims = sc.hs.grid()[0]["dims"]
        assert dims[axis] == res and dims[thin[0]] == 3 and dims[thin[1]] == 3, dims
        ok = int(res <= 512)
        expect_info(sc.gs, pack_ok=ok, packed_cells=1, octant_words=1, rcp_safe=1)
        rec = check_kernels(sc)
        assert (rec[:, 0] == 1).any() and (rec[:, 0] == 0).any()
        eye = np.full(3, 0.005, np.float32)
        eye[axis] = 0.3
        eye[thin[0]] = 0.12
        at = eye.copy()
        at[thin[0]] = 0.0
        at[axis] = 0.25
        sc.hs.fov = 45.0
        sc.look(S.look(eye, at))
        rec = check_kernels(sc)
        assert (rec[:, 0] == 1).any() and (rec[:, 0] == 0).any()
    finally:
        sc.close()


# ------------------------------------------------------------------ B4
def test_b4_no_octant_words():
    """512 x 129 x 128 = 8,454,144 cells, just over 2^23 with every axis <= 512: the 8 octant copies would
    pass their 256 MiB cap, so the walk reads the L-inf words with oct_stride == 0 (and no box words: their
    24 copies pass their cap as well).  The host grid is 34 MB of offsets; rt_scene_create's BFS over the
    cells is the slow part."""
    import time
    t0 = time.time()
    sc = VScene(S.big_grid_mesh(60), S.look((2.2, 1.4, 1.9), (0.0, 0.25, 0.25)), grid_res=512)
    print(f"B4 scene creation {time.time() - t0:.1f} s")
    try:
        dims = sc.hs.grid()[0]["dims"]
        assert dims == [512, 129, 128], dims
        expect_info(sc.gs, octant_words=0, packed_cells=1, box_words=0, pack_ok=1, rcp_safe=1)
        rec = check_kernels(sc)
        assert (rec[:, 0] == 1).any() and (rec[:, 0] == 0).any()
        sc.look(S.axis_cam(0, 1, (-1.5, 0.2, 0.21)))               # along the 512-cell axis
        check_kernels(sc)
    finally:
        sc.close()


# ------------------------------------------------------------------ B5
def test_b5_not_rcp_safe():
    """The sparse scene plus a triangle with |e1|_1 |e2|_1 = 1.5 * 2^124: rcp_safe == 0 with box words and
    pack_ok, i.e. kVarAutoCore | kVarPackedRem | kVarSkipRun (the exact reciprocal inside the box-run walk)."""
    hs = S.build_host(S.cases()["axis_z"])
    try:
        cb = CallerBuilt(hs)
    finally:
        hs.close()
    sc = VScene(host=cb)
    try:
        expect_info(sc.gs, rcp_safe=0, packed_cells=1, box_words=1, pack_ok=1, octant_words=1)
        rec = check_kernels(sc, nan_ok=True)
        assert (rec[:, 1] == cb.t.shape[0] - 1).any(), "no sample reached the appended triangle"
        sc.look(S.look((0.8, 0.6, 2.6), (0.0, 0.0, -0.36)))
        check_kernels(sc, nan_ok=True)
    finally:
        sc.close()


def test_b5_not_rcp_safe_unpackable(tmp_path):
    """The same on stack2100: neither rcp_safe nor cell words, i.e. kVarAutoCore alone."""
    hs = rtm.HostScene.load(S.gunzip_scene("stack2100", tmp_path))
    try:
        cb = CallerBuilt(hs)
    finally:
        hs.close()
    sc = VScene(host=cb)
    try:
        expect_info(sc.gs, rcp_safe=0, packed_cells=0, box_words=0, pack_ok=1, max_cell_refs=2100)
        rec = check_kernels(sc, nan_ok=True)
        assert (rec[:, 1] == cb.t.shape[0] - 1).any(), "no sample reached the appended triangle"
        assert ((rec[:, 0] == 1) & (rec[:, 1] < 2100)).any()
    finally:
        sc.close()


# ------------------------------------------------------------------ B6
def test_b6_batch_falls_back_for_a_non_auto_scene(oracle, tmp_path):
    """rt_render_batch_device refuses scenes that are not kVarAuto (launch_batch) and renders one launch per
    frame instead: [stack2100, scene 1] gives both correct frames and batch_fallbacks goes up."""
    import torch
    e = S.meta()["cases"]["stack2100"]
    hss = [rtm.HostScene.load(S.gunzip_scene("stack2100", tmp_path)), rtm.HostScene.load(1)]
    gss = [rtm.GpuScene(h, 0) for h in hss]
    try:
        expect_info(gss[0], packed_cells=0)
        before = gss[0].info()
        fs = [g.frame(S.W, S.H, S.SPP) for g in gss]
        outs = [torch.full((S.W * S.H,), S.SENTINEL, dtype=torch.int32, device="cuda") for _ in gss]
        hits = [torch.full((S.W * S.H * S.SPP,), S.SENTINEL, dtype=torch.int32, device="cuda") for _ in gss]
        rtm.render_batch_device(gss, fs, [o.data_ptr() for o in outs], d_hits=[h.data_ptr() for h in hits],
                                stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        after = gss[0].info()
        assert after["batch_fallbacks"] == before["batch_fallbacks"] + 1, (before, after)
        assert after["batch_launches"] == before["batch_launches"]
        np.testing.assert_array_equal(outs[0].cpu().numpy().view(np.uint32), S.read_synth(e["bgra"], "<u4"))
        exp, hid, _ = oracle.render(1, S.W, S.H, S.SPP, hits=True)
        np.testing.assert_array_equal(outs[1].cpu().numpy().view(np.uint32).reshape(S.H, S.W), exp)
        np.testing.assert_array_equal(hits[1].cpu().numpy().view(np.uint32), hid)
        import hashlib
        assert hashlib.sha256(hits[0].cpu().numpy().tobytes()).hexdigest() == e["hits_sha256"]
    finally:
        for g in gss:
            g.close()
        for h in hss:
            h.close()
