"""AUTO's wave-uniform record loop (test_cell, rt_walk.h) on synthetic scenes that sit on its edges.

The loop walks a cell's list two records per trip with the NEXT record always in flight, so the
last trip loads one record past the list; for the last cell of the CSR that record lies in the zero
pad behind the per-origin record buffers (kFrefPad, rt_kparams.h).  What the loop must keep: the
same records tested in the same order, so every frame is byte-equal to RT_KERNEL_LANES (the plain
per-lane walk, pinned to the reference by test_gpu_parity.py) and every per-sample record of the
product kernel (rt_render_records_device, obtained as in test_gpu_records.py) is bit-equal to the
plain walk's record of the same sample (rt_trace_samples).

The product kernels do not count DDA steps or tests (their records hold 0xFFFFFFFF there, see
store_record), so `steps` and `tests` cannot be compared word for word; the walk itself is pinned
through the voxel word instead: the cell a hit was accepted in, or the last cell walked on a miss,
which differs as soon as a walk takes another step sequence.

64x64x4 frames, a few triangles: every case takes well under a second.
"""
import numpy as np
import pytest

from conftest import load_package

rtm = load_package()
W, H, SPP = 64, 64, 4
REC_WORDS = 12
# rt_sample_rec words both kernels fill: hit, tri, voxel, t, u, v, r, g, b
SHARED_WORDS = (0, 1, 2, 5, 6, 7, 8, 9, 10)
# sample 0 sits on the pixel corner: pixel (32, 32) then looks exactly down the camera axis, so an
# axis-aligned camera gives that ray two zero direction components
OFFSETS = np.array([0.0, 0.0, 0.25, 0.5, 0.5, 0.25, 0.75, 0.75], np.float32)


def mesh_of(tris):
    """tris: [nt, 3, 3] points -> (vertices [3 nt, 6], triangles [nt, 6]) as HostScene.from_mesh takes them."""
    p = np.asarray(tris, np.float32)
    nt = p.shape[0]
    v = np.zeros((nt * 3, 6), np.float32)
    v[:, :3] = p.reshape(-1, 3)
    v[:, 4] = 1.0
    t = np.zeros((nt, 6), np.uint32)
    t[:, :3] = np.arange(nt * 3, dtype=np.uint32).reshape(nt, 3)
    t[:, 4] = np.float32(1.0).view(np.uint32)
    return v, t


def facing_stack(zs):
    """One big triangle per z, all overlapping around the z axis (slightly different shapes, so
    their u, v differ), facing a camera on the z axis."""
    out = []
    for i, z in enumerate(zs):
        s = 1.0 + 0.03 * (i % 5)
        out.append([[-s, -0.9, z], [s, -0.8, z], [0.05 * (i % 3), s, z]])
    return out


class Scene:
    def __init__(self, tris, eye, at, grid_res):
        v, t = mesh_of(tris)
        self.hs = rtm.HostScene.from_mesh(v, t, 45.0, rtm.look_at(eye, at), grid_res=grid_res)
        self.gs = rtm.GpuScene(self.hs, 0)

    def look(self, eye, at):
        self.hs.cam = rtm.look_at(eye, at)

    def close(self):
        self.gs.close()
        self.hs.close()


def check_against_plain_walk(sc):
    """AUTO's frame and product records vs RT_KERNEL_LANES' frame and the plain walk's records.
    Returns AUTO's records (u32 [W H SPP, 12])."""
    import torch
    gs = sc.gs
    f_auto = gs.frame(W, H, SPP, sample_offsets=OFFSETS)
    f_lanes = gs.frame(W, H, SPP, kernel=rtm.RT_KERNEL_LANES, sample_offsets=OFFSETS)
    plain = gs.render_frame(f_lanes)
    auto = gs.render_frame(f_auto)
    assert auto.tobytes() == plain.tobytes(), f"{(auto != plain).sum()} pixels differ from RT_KERNEL_LANES"
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    rec = torch.full((W * H * SPP * REC_WORDS,), -1, dtype=torch.int32, device="cuda")
    rtm.render_records_device([gs], [f_auto], [out.data_ptr()], [(0, 0, W, H)], [rec.data_ptr()],
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert out.cpu().numpy().view(np.uint32).reshape(H, W).tobytes() == plain.tobytes()
    got = rec.cpu().numpy().view(np.uint32).reshape(-1, REC_WORDS)
    ref = gs.trace_samples(f_lanes, 0, 0, W, H).view(np.uint32).reshape(-1, REC_WORDS)
    for w in SHARED_WORDS:
        np.testing.assert_array_equal(got[:, w], ref[:, w], err_msg=f"record word {w}")
    assert (got[:, 3] == 0xFFFFFFFF).all() and (got[:, 4] == 0xFFFFFFFF).all()
    return got


def centre_record(rec):
    return rec[((H // 2) * W + W // 2) * SPP]          # pixel (32, 32), sample 0: the camera axis


EYE, AT = (0.0, 0.0, 4.0), (0.0, 0.0, 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [1, 2, 3, 4, 5, 8, 9, 16, 17])
@pytest.mark.parametrize("nearest", ["last", "first"])
def test_single_cell_list_lengths(nt, nearest):
    """grid_res=1: one cell holds every triangle, and it is the CSR's first and last cell, so the
    loop's final look-ahead load lands in the pad.  nt covers both register sets, odd and even
    tails and the lone record.  The camera looks down -z from z = 4, so the nearest triangle is the
    one with the largest z: at the last list position ('last': a hit accepted in the final record
    of the odd tail or of the second set) or at the first."""
    zs = [0.1 * i for i in range(nt)]                     # ascending z: the last triangle is nearest
    if nearest == "first":
        zs = zs[::-1]
    sc = Scene(facing_stack(zs), EYE, AT, grid_res=1)
    try:
        assert sc.hs.grid()[0]["dims"] == [1, 1, 1]
        rec = check_against_plain_walk(sc)
        c = centre_record(rec)
        assert c[0] == 1 and c[1] == (nt - 1 if nearest == "last" else 0)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [2, 5, 8])
def test_tie_in_the_last_records_keeps_the_first(nt):
    """The two nearest triangles are the same triangle twice, at the last two list positions: the
    strict '<' of grid.cpp:258-260 keeps the first of equal t."""
    zs = [0.1 * i for i in range(nt - 1)]
    tris = facing_stack(zs)
    tris.append([list(p) for p in tris[-1]])              # coplanar, identical
    sc = Scene(tris, EYE, AT, grid_res=1)
    try:
        rec = check_against_plain_walk(sc)
        c = centre_record(rec)
        assert c[0] == 1 and c[1] == nt - 2
        hits = rec[rec[:, 0] == 1]
        assert not (hits[:, 1] == nt - 1).any()           # the duplicate never wins anywhere
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [1, 4])
def test_pad_stays_zero_across_origins(nt):
    """Origins A, B, C, A: both per-origin buffers are filled again (k_origin_pre writes nrefs
    records only), and every frame still equals the plain walk's -- the look-ahead record behind the
    last list is read in each of them."""
    sc = Scene(facing_stack([0.1 * i for i in range(nt)]), EYE, AT, grid_res=1)
    try:
        for eye in (EYE, (0.7, -0.4, 3.5), (-1.1, 0.6, 5.0), EYE):
            sc.look(eye, AT)
            check_against_plain_walk(sc)
    finally:
        sc.close()


def corner_scene(eye, at):
    """An 8^3 grid that is empty but for one small triangle in the far corner cell and one in the
    near corner cell (which spans the grid): rays cross long empty box runs of different lengths."""
    far = [[0.90, 0.90, 0.90], [0.98, 0.90, 0.92], [0.92, 0.98, 0.96]]
    near = [[-0.98, -0.98, -0.98], [-0.92, -0.98, -0.97], [-0.97, -0.92, -0.98]]
    return Scene([far, near], eye, at, grid_res=8)


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["diagonal", "axis"])
def test_box_runs_of_different_lengths(view):
    """The camera looks down the grid's diagonal at the far corner triangle (lanes of one wave take
    runs of different lengths along all three axes), or straight along an axis (pixel (32, 32)
    sample 0 has two zero direction components, its neighbours tiny ones).  The voxel word (the
    accepted cell, or the last cell walked on a miss) must be the plain walk's for every sample."""
    if view == "diagonal":
        sc = corner_scene((-3.0, -2.6, -2.8), (0.94, 0.93, 0.93))
    else:
        sc = corner_scene((0.93, 0.93, -4.0), (0.93, 0.93, 0.0))
    try:
        assert sc.hs.grid()[0]["dims"] == [8, 8, 8]
        rec = check_against_plain_walk(sc)
        assert (rec[:, 0] == 1).any() and (rec[:, 0] == 0).any()
    finally:
        sc.close()


@pytest.mark.gpu
def test_device_bytes_counts_both_padded_buffers():
    sc = Scene(facing_stack([0.0, 0.1, 0.2]), EYE, AT, grid_res=1)
    try:
        nrefs = sc.hs.stats["num_refs"]
        assert nrefs == 3
        # refs (48 B each) + two padded per-origin buffers are part of the total
        assert sc.gs.device_bytes() >= 48 * nrefs + 2 * rtm.fref_buffer_bytes(nrefs)
    finally:
        sc.close()


def test_fref_buffer_bytes_includes_the_pad():
    """CPU only: one per-origin buffer = 64 B per reference (at least one) + 2 * (256 / 64) pad records."""
    pad = 2 * (256 // 64)
    for n in (0, 1, 2, 7, 1000, (1 << 20) - 1):
        assert rtm.fref_buffer_bytes(n) == (max(n, 1) + pad) * 64
