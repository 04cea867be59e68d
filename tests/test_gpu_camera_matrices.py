"""The render kernels under cameras whose 3x3 is not orthonormal (tests/camera_matrices.py).

rt_frame.cam is the caller's matrix; GenerateRay normalises the direction BEFORE the 3x3, so a scaled matrix gives
long (or short) directions.  Two proofs of the benchmarked path assume unit ones: the record gate's bound E
(csrc/rt_record_gate.h, |D_i| <= 1.0001) and kVarFastRcp in the render kernels (csrc/rt_ray_common.h,
|d|_inf <= 8).  The library bounds |D_i| per frame from the matrix (csrc/rt_cam_bound.h) and launches that frame
without gate records / without kVarFastRcp when the bound is exceeded.  Without that guard AUTO skips records a
lane passes: the frozen sliver scene (a triangle whose u = 0 edge lies in the plane of one pixel column's rays)
shows it at S = 2^10 and 2^20.

Expected values are the reference's own (tests/golden/cameras.json, oracle/gen_golden_cameras.py): frame and hit-ID
SHA-256 from `refdriver render --view` for the 64-cell scenes, hit-ID SHA-256 from `refdriver rays <file> 1` for the
single-cell scenes (a grid the reference's renderer cannot build; there the frames of every kernel are held to the
plain per-lane walk's, RT_KERNEL_LANES, and its records to the reference's hit IDs).  Each comparison goes first
against the live CPU restatement, so that a mismatch is printed per sample.

Per (scene, factor): frames from AUTO, LANES, PIXEL_LOOP, COMPACT and AUTO | WIDE_HEAVY, each twice, on the scene
and on one created with RT_REC_GATE=0; rt_render_hits_device; rt_render_records_device at 1, 2 and 8 ranks against
rt_trace_samples word for word; rt_trace_rays_device of the frame's primary rays.  Every output buffer is
pre-filled with 0x5A5A5A5A.  64x64x4 and 96x54x4 frames: a case takes well under a second.
"""
import hashlib

import numpy as np
import pytest

import camera_matrices as C
import occlusion_ref as R
import synth_scenes as S
from conftest import load_package
from ray_variant_scenes import CallerBuilt
from test_gpu_record_gate import gate_env

pytestmark = pytest.mark.gpu
rtm = load_package()
FX = C.fixture()
CASES = sorted(FX["cases"])
KERNELS = {"auto": rtm.RT_KERNEL_AUTO, "lanes": rtm.RT_KERNEL_LANES, "pixel_loop": rtm.RT_KERNEL_PIXEL_LOOP,
           "compact": rtm.RT_KERNEL_COMPACT, "auto_wide": rtm.RT_KERNEL_AUTO | rtm.RT_KERNEL_FLAG_WIDE_HEAVY}
REC_WORDS = 12
SHARED_WORDS = (0, 1, 2, 5, 6, 7, 8, 9, 10)         # hit, tri, voxel, t, u, v, r, g, b (test_gpu_uniform_lists.py)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sentinel(torch, n):
    return torch.full((n,), C.SENTINEL, dtype=torch.int32, device="cuda")


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


class Sc:
    """One scene on the device, twice (with and without gate records), and its CPU restatement."""

    def __init__(self, name, tmp, oracle):
        self.name, self.cell = name, name not in C.GRID_SCENES
        if self.cell:
            tris, cam = C.cell_scenes(FX)[name]
            self.hs = C.host_scene(tris, cam)
            assert self.hs.grid()[0]["dims"] == [1, 1, 1]
            self.osc = None
            self.frame_shape, self.offsets = (C.W, C.H, C.SPP), C.OFFSETS
        else:
            path = S.scene_file({"scene": name}, tmp)
            self.hs = rtm.HostScene.load(path)
            self.osc = S.OracleScene(oracle, path)
            self.frame_shape, self.offsets = C.CAM_FRAME, None
        self.ref = R.RefScene.from_host(self.hs)
        with gate_env(None):
            self.gs = rtm.GpuScene(self.hs, 0)
        with gate_env("0"):
            self.gs0 = rtm.GpuScene(self.hs, 0)
        self.smp = C.OFFSETS.reshape(-1, 2) if self.cell else rtm.sample_table(self.frame_shape[2])
        self.expected = {}

    def cam_of(self, factor):
        e = FX["cases"][f"{self.name}|{factor}"]
        cam = C.from_bits(FX["cams"][e["cam"]][factor])
        fov = float(C.from_bits([FX["cams"][e["cam"]]["fov_bits"]])[0]) if not self.cell else 45.0
        return cam, fov

    def frame(self, factor, kernel=rtm.RT_KERNEL_AUTO, gs=None):
        cam, fov = self.cam_of(factor)
        Wd, Ht, spp = self.frame_shape
        f = (gs or self.gs).frame(Wd, Ht, spp, kernel=kernel, sample_offsets=self.offsets)
        for k in range(16):
            f.cam[k] = float(cam[k])
        f.fov = fov
        return f

    def expect(self, factor):
        """(frame u32 [H, W] or None, hit ids u32 [W H spp], rays f32 [n, 6]) of the live CPU restatement, held to
        the fixture's SHAs: computed once per (scene, factor).  None: a single-cell scene has no reference frame."""
        if factor not in self.expected:
            e = FX["cases"][f"{self.name}|{factor}"]
            cam, fov = self.cam_of(factor)
            Wd, Ht, spp = self.frame_shape
            rays = C.generate_rays(cam, fov, Wd, Ht, self.smp)
            if self.cell:
                res = R.walk(self.ref, rays)
                img, hid = None, np.where(res["hit"], res["tri"], np.uint32(C.NOTRI)).astype(np.uint32)
            else:
                img, hid = self.osc.render(Wd, Ht, spp, cam=cam, fov=fov)
                assert sha(img) == e["bgra_sha256"], "the CPU restatement differs from the reference"
            assert sha(hid) == e["hits_sha256"], "the CPU restatement differs from the reference"
            self.expected[factor] = (img, hid, rays)
        return self.expected[factor]

    def close(self):
        self.gs.close()
        self.gs0.close()
        if self.osc:
            self.osc.close()
        self.hs.close()


@pytest.fixture(scope="module")
def scenes(tmp_path_factory, oracle):
    tmp = tmp_path_factory.mktemp("cameras")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Sc(name, tmp, oracle)
        return cache[name]
    yield get
    import torch
    torch.cuda.synchronize()
    for sc in cache.values():
        sc.close()


def render(torch, gs, f, what, st=None):
    out = sentinel(torch, f.width * f.height)
    gs.render_frame_device(f, out.data_ptr(), st if st is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = host_u32(out).reshape(f.height, f.width)
    assert not (got == C.SENTINEL).any(), f"{what}: unwritten pixels"
    return got


def check_case(sc, factor):
    import torch
    e = FX["cases"][f"{sc.name}|{factor}"]
    img, hid, rays = sc.expect(factor)
    Wd, Ht, spp = sc.frame_shape
    st = torch.cuda.current_stream().cuda_stream
    what = f"{sc.name} {factor}"
    # the plain per-lane walk first: its counting records against the reference's hit IDs, its frame is the
    # expectation where the reference has none
    f_lanes = sc.frame(factor, rtm.RT_KERNEL_LANES)
    plain = sc.gs.trace_samples(f_lanes, 0, 0, Wd, Ht).view(np.uint32).reshape(-1, REC_WORDS)
    pid = np.where(plain[:, 0] == 1, plain[:, 1], np.uint32(C.NOTRI))
    np.testing.assert_array_equal(pid, hid, err_msg=f"{what}: rt_trace_samples hit ids")
    if img is None:
        img = render(torch, sc.gs, f_lanes, what + " lanes")
    # every kernel, twice, with and without gate records
    for gname, gs in (("gate", sc.gs), ("RT_REC_GATE=0", sc.gs0)):
        for kname, k in KERNELS.items():
            f = sc.frame(factor, k, gs)
            for rep in range(2):
                got = render(torch, gs, f, f"{what} {kname} {gname}")
                np.testing.assert_array_equal(got, img, err_msg=f"{what}: {kname} ({gname}) launch {rep}")
    if "bgra_sha256" in e:
        assert sha(img) == e["bgra_sha256"]
    # hit ids
    n = Wd * Ht
    f = sc.frame(factor)
    out, hits = sentinel(torch, n), sentinel(torch, n * spp)
    sc.gs.render_hits_device(f, 0, 1, out.data_ptr(), hits.data_ptr(), st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host_u32(hits), hid, err_msg=f"{what}: rt_render_hits_device hit ids")
    np.testing.assert_array_equal(host_u32(out).reshape(Ht, Wd), img, err_msg=f"{what}: rt_render_hits_device frame")
    assert sha(host_u32(hits)) == e["hits_sha256"] and int((hid != C.NOTRI).sum()) == e["hit_samples"]
    # the benchmarked launch path's records at 1, 2 and 8 ranks, word for word against the plain walk's
    for nranks in (1, 2, 8):
        rec = sentinel(torch, n * spp * REC_WORDS)
        shards = []
        for r in range(nranks):
            o = sentinel(torch, n if nranks == 1 else rtm.shard_elems(Wd, Ht, nranks))
            rtm.render_records_device([sc.gs], [f], [o.data_ptr()], [(0, 0, Wd, Ht)], [rec.data_ptr()], r, nranks, stream=st)
            shards.append(o)
        torch.cuda.synchronize()
        got = host_u32(rec).reshape(-1, REC_WORDS)
        for w in SHARED_WORDS:
            a, b = got[:, w], plain[:, w]
            if w >= 5:
                a, b = S.nan_canonical(a), S.nan_canonical(b)
            np.testing.assert_array_equal(a, b, err_msg=f"{what}: rank of {nranks}, record word {w}")
        assert (got[:, 3] == 0xFFFFFFFF).all() and (got[:, 4] == 0xFFFFFFFF).all()
        if nranks == 1:
            full = shards[0]
        else:
            full = sentinel(torch, n)
            rtm.unshard_device(Wd, Ht, nranks, torch.cat(shards).data_ptr(), full.data_ptr(), st)
            torch.cuda.synchronize()
        np.testing.assert_array_equal(host_u32(full).reshape(Ht, Wd), img, err_msg=f"{what}: rank of {nranks} frame")
    # the frame's primary rays: GenerateRay bit for bit, and rt_trace_rays_device finds the same triangles
    d_rays = sc.gs.primary_rays(f)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_rays.cpu().numpy().view(np.uint32), rays.view(np.uint32), err_msg=f"{what}: primary rays")
    th = sc.gs.trace_rays(d_rays)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host_u32(th.hits[:, 0].contiguous()), hid, err_msg=f"{what}: rt_trace_rays_device")


@pytest.mark.parametrize("case", CASES)
def test_every_kernel_against_the_reference(scenes, case):
    scene, factor = case.split("|")
    check_case(scenes(scene), factor)


# ------------------------------------------------------------------ state and batching
STATE_SCENES = ("sliver9_4", "scene8")
SEQ = ("identity", C.S1024, "identity")


def expected_frame(torch, sc, factor):
    img, hid, _ = sc.expect(factor)
    if img is None:
        img = render(torch, sc.gs, sc.frame(factor, rtm.RT_KERNEL_LANES), f"{sc.name} {factor} lanes")
    return img, hid


@pytest.mark.parametrize("scene", STATE_SCENES)
def test_camera_changes_between_frames(scenes, scene):
    """orthonormal -> S = 1024 -> orthonormal at one origin, twice over: the per-origin records and gate arrays
    stay, what the launch may use of them changes with the frame's matrix."""
    import torch
    sc = scenes(scene)
    want = {f: expected_frame(torch, sc, f)[0] for f in set(SEQ)}
    for rnd in range(2):
        for i, factor in enumerate(SEQ):
            got = render(torch, sc.gs, sc.frame(factor), f"{scene} {factor}")
            np.testing.assert_array_equal(got, want[factor], err_msg=f"{scene}: round {rnd} frame {i} ({factor})")


@pytest.mark.parametrize("scene", STATE_SCENES)
def test_camera_changes_between_overlapped_frames(scenes, scene):
    """The same sequence with RT_KERNEL_FLAG_OVERLAP on two alternating streams, nothing waited for in between."""
    import torch
    sc = scenes(scene)
    want = {f: expected_frame(torch, sc, f)[0] for f in set(SEQ)}
    Wd, Ht, _ = sc.frame_shape
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    seq = SEQ * 3
    outs = [sentinel(torch, Wd * Ht) for _ in seq]
    torch.cuda.synchronize()
    for i, factor in enumerate(seq):
        f = sc.frame(factor, rtm.RT_KERNEL_AUTO | rtm.RT_KERNEL_FLAG_OVERLAP)
        sc.gs.render_frame_device(f, outs[i].data_ptr(), streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for i, factor in enumerate(seq):
        np.testing.assert_array_equal(host_u32(outs[i]).reshape(Ht, Wd), want[factor], err_msg=f"{scene}: frame {i} ({factor})")


@pytest.mark.parametrize("nranks", [1, 8])
@pytest.mark.parametrize("order", [("identity", C.S1024), (C.S1024, "identity"), ("identity", "scale_1+2^-13")])
@pytest.mark.parametrize("scene", STATE_SCENES)
def test_batch_of_two_cameras(scenes, scene, order, nranks):
    """rt_render_batch_device of [orthonormal, S = 1024] and the reverse: the camera is per FRAME, so a guard taken
    from frame 0 alone gives the other frame the wrong loop.  [orthonormal, 1 + 2^-13]: both keep the fast
    reciprocal (the same kernel variant) and only the second loses the gate.  Every frame and its hit IDs must equal
    its own expectation; frames whose choices differ do not share a launch (rt_scene_info.batch_fallbacks counts it)."""
    import torch
    sc = scenes(scene)
    Wd, Ht, spp = sc.frame_shape
    n = Wd * Ht
    want = [expected_frame(torch, sc, f) for f in order]
    fs = [sc.frame(f) for f in order]
    e = n if nranks == 1 else rtm.shard_elems(Wd, Ht, nranks)
    st = torch.cuda.current_stream().cuda_stream
    before = sc.gs.info()["batch_fallbacks"]
    for rep in range(2):
        bufs = [sentinel(torch, nranks * e) for _ in order]
        hits = [sentinel(torch, n * spp) for _ in order]
        for r in range(nranks):
            rtm.render_batch_device([sc.gs, sc.gs], fs, [b.data_ptr() + 4 * r * e for b in bufs], rank=r, nranks=nranks,
                                    d_hits=[h.data_ptr() for h in hits], stream=st)
        torch.cuda.synchronize()
        for i, factor in enumerate(order):
            full = bufs[i]
            if nranks > 1:
                full = sentinel(torch, n)
                rtm.unshard_device(Wd, Ht, nranks, bufs[i].data_ptr(), full.data_ptr(), st)
                torch.cuda.synchronize()
            np.testing.assert_array_equal(host_u32(full).reshape(Ht, Wd), want[i][0],
                                          err_msg=f"{scene} {order} rank of {nranks}: frame {i} ({factor}), launch {rep}")
            np.testing.assert_array_equal(host_u32(hits[i]), want[i][1],
                                          err_msg=f"{scene} {order} rank of {nranks}: hit ids {i} ({factor}), launch {rep}")
    assert sc.gs.info()["batch_fallbacks"] == before + 2 * nranks


# ------------------------------------------------------------------ ray generation
def test_generate_ray_bit_for_bit():
    """rt_debug_primitives kind 2 (GenerateRay) on every matrix of the fixture, every fifth pixel (12 x 12 x 4 samples) of a
    64 x 64 frame each, against the numpy float32 restatement: one rounding per operation, no FMA."""
    smp = C.OFFSETS.reshape(-1, 2)
    for base, cams in FX["cams"].items():
        fov = float(C.from_bits([cams["fov_bits"]])[0]) if "fov_bits" in cams else 45.0
        for factor in C.FACTOR_NAMES:
            if factor not in cams:
                continue
            cam = C.from_bits(cams[factor])
            rays = C.generate_rays(cam, fov, C.W, C.H, smp).reshape(C.H, C.W, C.SPP, 6)[4::5, 4::5]
            y, x, s = [a.reshape(-1) for a in np.meshgrid(np.arange(4, C.H, 5), np.arange(4, C.W, 5), np.arange(C.SPP),
                                                          indexing="ij")]
            rin = np.zeros((x.size, 23), np.float32)
            rin[:, :16] = cam
            b = rin.view(np.uint32)
            b[:, 16], b[:, 17], b[:, 18], b[:, 19] = x, y, C.W, C.H
            rin[:, 20], rin[:, 21], rin[:, 22] = smp[s, 0], smp[s, 1], np.float32(fov)
            got = rtm.debug_primitives(2, rin)
            np.testing.assert_array_equal(got.view(np.uint32), rays.reshape(-1, 6).view(np.uint32),
                                          err_msg=f"GenerateRay {base} {factor}")


# ------------------------------------------------------------------ the reciprocal
RCP_SCALES = {"2^0": 0, "2^4": 4, "2^8": 8, "2^10": 10, "2^20": 20}      # uniform scales of the camera's 3x3


@pytest.fixture(scope="module")
def big_scene():
    """axis_z (synth_scenes) with one appended triangle of edges 2^59.5 and 2^59 * (1, 2): |e1|_1 |e2|_1 =
    0.75 * 2^120, just under the bound below which rt_scene_info.rcp_safe holds, so AUTO's kVarFastRcp
    instantiation runs -- whose reciprocal is exact only for |det| < 2^126, that is for |d|_inf <= 8."""
    hs = S.build_host(S.cases()["axis_z"])
    cb = CallerBuilt(hs, big=2.0 ** 58.5)
    hs.close()
    gs = rtm.GpuScene(cb, 0)
    ref = R.RefScene(cb.g, cb.offs, cb.refs, cb.v, cb.t)
    yield cb, gs, ref
    gs.close()


@pytest.mark.parametrize("factor", list(RCP_SCALES))
def test_fast_reciprocal_only_inside_its_proof(big_scene, factor):
    """|det| of the appended triangle is 2^119 |d_z|: inside rcp_nr's exact range for a unit direction, above it --
    up to overflow -- at 2^8, 2^10 and 2^20.  Expected: tests/occlusion_ref.py's closest-hit walk on the frame's
    own primary rays (the reference cannot build this grid); the frames of AUTO, COMPACT and AUTO | WIDE_HEAVY
    against the plain per-lane walk's."""
    import torch
    cb, gs, ref = big_scene
    info = gs.info()
    assert info["rcp_safe"] == 1 and info["box_words"] == 1 and info["pack_ok"] == 1, info
    cam = C.apply_factor(cb.cam, np.eye(3) * 2.0 ** RCP_SCALES[factor])
    Wd, Ht, spp = C.CAM_FRAME

    def frame(k):
        f = gs.frame(Wd, Ht, spp, kernel=k)
        for i in range(16):
            f.cam[i] = float(cam[i])
        return f
    d_rays = gs.primary_rays(frame(rtm.RT_KERNEL_AUTO))
    torch.cuda.synchronize()
    rays = d_rays.cpu().numpy()
    np.testing.assert_array_equal(rays.view(np.uint32),
                                  C.generate_rays(cam, cb.fov, Wd, Ht, rtm.sample_table(spp)).view(np.uint32))
    res = R.walk(ref, rays)
    hid = np.where(res["hit"], res["tri"], np.uint32(C.NOTRI)).astype(np.uint32)
    big = cb.t.shape[0] - 1
    print(f"{factor}: {int((hid == big).sum())} samples end on the appended triangle, {int(res['hit'].sum())} hits")
    assert (hid == big).sum() >= 100          # (a det that overflowed gives 1 / inf = 0: u = v = t = 0, a hit)
    n = Wd * Ht
    out, hits = sentinel(torch, n), sentinel(torch, n * spp)
    gs.render_hits_device(frame(rtm.RT_KERNEL_AUTO), 0, 1, out.data_ptr(), hits.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host_u32(hits), hid, err_msg=f"{factor}: hit ids")
    want = render(torch, gs, frame(rtm.RT_KERNEL_LANES), "lanes")
    np.testing.assert_array_equal(host_u32(out).reshape(Ht, Wd), want, err_msg=f"{factor}: hits launch frame")
    for kname, k in KERNELS.items():
        for rep in range(2):
            got = render(torch, gs, frame(k), kname)
            np.testing.assert_array_equal(got, want, err_msg=f"{factor}: {kname} launch {rep}")
