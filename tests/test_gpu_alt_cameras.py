"""RT_ISECT_BRUTE_FORCE and RT_ISECT_RAY_MARCH (brute_intersect and ray_march of csrc/rt_frame_isect.h) under cameras whose
3x3 is not orthonormal, from eyes on and around the mesh and on meshes with NaN-distance triangles
(tests/alt_cameras.py): everything the grid walk is pinned on, for the two other per-sample intersectors.

Expected values are the reference's own (tests/golden/alt_cameras.json, oracle/gen_golden_alt_cameras.py).  Every
comparison goes first against the live CPU restatement (column by column, so that a mismatch is printed per sample),
then against the fixture's SHA-256s.  Per case: rt_trace_samples records of the window (hit, steps, t, colour; brute
also tri, u, v and tests == the mesh's triangle count); frames from RT_KERNEL_LANES and RT_KERNEL_PIXEL_LOOP, each
twice; rt_render_hits_device's frame; for the march all of that once more with RT_KERNEL_FLAG_EXHAUSTIVE -- both arms
against the reference, not against each other -- and GpuScene.march of the window's primary rays in both arms.  Every
output buffer is pre-filled with 0x5A5A5A5A.  No sample is left out.
"""
import ctypes

import numpy as np
import pytest

import alt_cameras as A
import camera_matrices as C
import synth_scenes as S
from conftest import ISECT, load_package

pytestmark = pytest.mark.gpu
rtm = load_package()
CASES, _ = A.fixture()
KERNELS = {"lanes": rtm.RT_KERNEL_LANES, "pixel_loop": rtm.RT_KERNEL_PIXEL_LOOP}
REC_WORDS = 12


def sentinel(torch, n):
    return torch.full((n,), A.SENTINEL, dtype=torch.int32, device="cuda")


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


class Sc:
    def __init__(self, name, tmp):
        self.hs = rtm.HostScene.load(A.scene_file(name, tmp))
        self.gs = rtm.GpuScene(self.hs, 0)
        self.ntris = len(self.hs.mesh()[1])

    def close(self):
        self.gs.close()
        self.hs.close()


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("alt_cameras_gpu")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Sc(name, tmp)
        return cache[name]
    yield get
    import torch
    torch.cuda.synchronize()
    for sc in cache.values():
        sc.close()


@pytest.fixture(scope="module")
def live(oracle, tmp_path_factory):
    lv = A.Live(oracle, tmp_path_factory.mktemp("alt_cameras_live"))
    yield lv
    lv.close()


def frame_of(gs, c, shape, kernel, intersector=None):
    f = gs.frame(*shape, kernel=kernel, intersector=ISECT[c["mode"]] if intersector is None else intersector)
    for k in range(16):
        f.cam[k] = float(c["cam"][k])
    f.fov = float(c["fov"])
    return f


def render(torch, gs, f, what):
    out = sentinel(torch, f.width * f.height)
    gs.render_frame_device(f, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = host_u32(out).reshape(f.height, f.width)
    assert not (got == A.SENTINEL).any(), f"{what}: unwritten pixels"
    return got


def trace(gs, f, x0, y0, w, h):
    """rt_trace_samples into a pre-filled buffer."""
    out = np.full(w * h * max(1, f.spp) * REC_WORDS, A.SENTINEL, np.uint32)
    L = rtm.tracer_lib()
    rtm._check(L.rt_trace_samples(gs._h, ctypes.byref(f), x0, y0, w, h, rtm._ptr(out)), L, "rt_trace_samples")
    assert not (out.reshape(-1, REC_WORDS)[:, :11] == A.SENTINEL).any(), "unwritten record words"
    return out.view(rtm.SAMPLE_REC_DTYPE)


def check_case(sc, c, live):
    import torch
    key, mode, gs = c["key"], c["mode"], sc.gs
    cols, img = live.expect(c)
    A.check_entry(cols, img, c["exp"], key + " (restatement)")
    Wd, Ht, spp, x0, y0, w, h = c["window"]
    arms = {"default": 0, "exhaustive": rtm.RT_KERNEL_FLAG_EXHAUSTIVE} if mode == "march" else {"default": 0}
    for aname, flag in arms.items():
        what = f"{key} [{aname}]"
        # records
        rec = trace(gs, frame_of(gs, c, (Wd, Ht, spp), rtm.RT_KERNEL_AUTO | flag), x0, y0, w, h)
        got = A.columns(rec, mode)
        A.check_columns(got, cols, what + " rt_trace_samples")
        if mode == "brute":
            assert (rec["tests"] == sc.ntris).all(), what
        A.check_entry(got, None, {k: v for k, v in c["exp"].items() if k != "frame_sha"}, what)
        # frames
        if c["frame"]:
            pow2 = c["frame"][2] & (c["frame"][2] - 1) == 0          # (RT_KERNEL_LANES: spp a power of two; else AUTO)
            for kname, k in KERNELS.items():
                f = frame_of(gs, c, c["frame"], (k if pow2 or kname != "lanes" else rtm.RT_KERNEL_AUTO) | flag)
                for rep in range(2):
                    np.testing.assert_array_equal(render(torch, gs, f, what), img, err_msg=f"{what}: {kname} launch {rep}")
            f = frame_of(gs, c, c["frame"], rtm.RT_KERNEL_AUTO | flag)
            fw, fh, fs = c["frame"]
            out, hits = sentinel(torch, fw * fh), sentinel(torch, fw * fh * fs)
            gs.render_hits_device(f, 0, 1, out.data_ptr(), hits.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(host_u32(out).reshape(fh, fw), img, err_msg=f"{what}: rt_render_hits_device frame")
            assert A.sha(host_u32(out)) == c["exp"]["frame_sha"], what
            if mode == "brute" and (x0, y0, w, h) == (0, 0, fw, fh) and (Wd, Ht, spp) == c["frame"]:
                np.testing.assert_array_equal(host_u32(hits), cols["tri"], err_msg=f"{what}: rt_render_hits_device hit ids")
    if mode == "march":
        # the march query on the window's primary rays: the frame records' hit, t and steps (a frame miss reports
        # 128 steps, a query miss 0)
        rays = gs.primary_rays(frame_of(gs, c, (Wd, Ht, spp), rtm.RT_KERNEL_AUTO))
        win = rays.reshape(Ht, Wd, spp, 6)[y0:y0 + h, x0:x0 + w].reshape(-1, 6).contiguous()
        for ex in (False, True):
            mh = gs.march(win, exhaustive=ex)
            torch.cuda.synchronize()
            raw = mh.raw.cpu().numpy().view(np.uint32)
            steps = raw[:, 3]
            what = f"{key} GpuScene.march exhaustive={ex}"
            np.testing.assert_array_equal((steps != 0).astype(np.uint32), cols["hit"], err_msg=what)
            np.testing.assert_array_equal(np.where(steps != 0, steps, A.MARCH_STEPS), cols["steps"], err_msg=what)
            np.testing.assert_array_equal(S.nan_canonical(raw[:, 0]), cols["t"], err_msg=what)


@pytest.mark.parametrize("key", sorted(CASES))
def test_alt_intersectors_against_the_reference(scenes, live, key):
    c = CASES[key]
    check_case(scenes(c["scene"]), c, live)


def test_nan_triangles_are_first_on_the_device(scenes):
    """The premise of the nan_* cases: the march's first seed (sorted record 0) is a NaN-distance triangle
    (alt_cameras.morton_order; tests/test_alt_cameras_cpu.py holds it to dist_tree_build's own order).  The
    device's distance query on a point next to it reports the lowest mesh triangle at the minimum, never one of them."""
    meshes = A.meshes()
    for name, lead in A.NAN_FIRST.items():
        order = A.morton_order(meshes[name])
        assert sorted(order[:lead]) == list(range(lead)), name
        if lead == meshes[name].shape[0]:
            continue
        pts = np.ascontiguousarray(meshes[name][0, :1] + np.float32(1e-3))
        d = scenes(name).gs.distance(pts)
        assert np.isfinite(d.dist).all() and (d.tri >= lead).all(), name


SHARD_SCENES = ("scene1", "inside", "stack1500")


@pytest.mark.parametrize("mode", ["brute", "march"])
@pytest.mark.parametrize("scene", SHARD_SCENES)
def test_shards_rebuild_the_scaled_frame(scenes, live, scene, mode):
    """Shards of ranks 0..2 under scale_2^10, and rt_unshard_device rebuilds the reference's frame."""
    import torch
    c = CASES[f"A1|{scene}|{C.S1024}|{mode}"]
    gs = scenes(scene).gs
    _, img = live.expect(c)
    assert A.sha(img) == c["exp"]["frame_sha"]
    Wd, Ht, _ = c["frame"]
    n = 3
    f = frame_of(gs, c, c["frame"], rtm.RT_KERNEL_AUTO)
    elems = rtm.shard_elems(Wd, Ht, n)
    g = sentinel(torch, n * elems)
    st = torch.cuda.current_stream().cuda_stream
    for r in range(n):
        gs.render_shard_device(f, r, n, g.data_ptr() + 4 * r * elems, st)
    out = sentinel(torch, Wd * Ht)
    rtm.unshard_device(Wd, Ht, n, g.data_ptr(), out.data_ptr(), st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host_u32(out).reshape(Ht, Wd), img)


@pytest.mark.parametrize("mode", ["brute", "march"])
def test_camera_changes_between_alt_and_grid_frames(scenes, live, mode):
    """identity -> scale_2^10 -> identity, each followed by a grid AUTO frame of the same camera, twice over: a march
    or brute launch reads no per-origin records and must leave the grid path's state alone.  Every frame against its
    own expectation (the grid frames: tests/golden/cameras.json)."""
    import torch
    gs = scenes("scene1").gs
    fx = C.fixture()
    for rnd in range(2):
        for i, factor in enumerate(("identity", C.S1024, "identity")):
            c = CASES[f"A1|scene1|{factor}|{mode}"]
            assert C.bits(c["cam"]) == fx["cams"]["scene1"][factor]
            _, img = live.expect(c)
            assert A.sha(img) == c["exp"]["frame_sha"]
            got = render(torch, gs, frame_of(gs, c, c["frame"], rtm.RT_KERNEL_AUTO), f"{mode} {factor}")
            np.testing.assert_array_equal(got, img, err_msg=f"{mode}: round {rnd} frame {i} ({factor})")
            grid = render(torch, gs, frame_of(gs, c, C.CAM_FRAME, rtm.RT_KERNEL_AUTO, rtm.RT_ISECT_GRID), f"grid {factor}")
            assert A.sha(grid) == fx["cases"][f"scene1|{factor}"]["bgra_sha256"], f"{mode}: round {rnd} grid frame {i} ({factor})"
