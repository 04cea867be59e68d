"""rt_trace_rays_device / rt_primary_rays_device (GpuScene.trace_rays / primary_rays) against the REFERENCE.

Fixtures: tests/golden/synth and synth.json (the reference's own Grid::Intersect records per camera sample,
oracle/gen_golden_synth.py; the scenes are described in tests/synth_scenes.py).  The camera rays come from
rt_primary_rays_device and are first compared, bit for bit, with the reference's GenerateRay
(oracle.kat("genray"), which tests/test_oracle_golden.py pins to the reference's recorded rays); traced as
caller-supplied rays they must then reproduce the fixtures: all eight geometric record columns through the
counting arm (RT_RAYS_COUNT), tri / t / u / v through the fast arm -- in camera order, and again shuffled so
that a wave's 64 rays share neither origin nor cells.

Bar: bit-exact.  Every output buffer is pre-filled with 0x5A5A5A5A and carries 64 elements past n, which
must still hold the sentinel afterwards.  The camera sets are traced once per module and shared.
"""
import ctypes
import gzip
import hashlib
import os

import numpy as np
import pytest

import synth_scenes as S
from conftest import load_package

pytestmark = pytest.mark.gpu
rtm = load_package()
META = S.meta()
CASES = sorted(META["cases"])
NOTRI = 0xFFFFFFFF
TAIL = 64
GEOM_COLS = ("hit", "tri", "voxel", "t", "u", "v", "steps", "tests")
FAST_COLS = ("hit", "tri", "t", "u", "v")
SHARED_MESH = ("axis_x", "axis_y", "axis_z", "eye_on_face", "eye_on_plane", "away", "far_eye")


# ------------------------------------------------------------------ helpers
def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def sentinel(torch, n):
    return torch.full((n,), S.SENTINEL, dtype=torch.int32, device="cuda")


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def raw_primary(torch, gs, f):
    """rt_primary_rays_device into a sentinel buffer with a 64-ray tail: (device rays [n, 6] f32, host copy)."""
    n = f.width * f.height * max(1, f.spp)
    buf = sentinel(torch, (n + TAIL) * 6)
    L = rtm.tracer_lib()
    rc = L.rt_primary_rays_device(gs._h, ctypes.byref(f), ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(stream_of(torch)))
    assert rc == 0
    torch.cuda.synchronize()
    h = host_u32(buf)
    assert (h[n * 6:] == S.SENTINEL).all(), "rt_primary_rays_device wrote past n"
    assert not (h[:n * 6] == S.SENTINEL).any(), "rt_primary_rays_device left rays unwritten"
    return buf[:n * 6].view(torch.float32).view(n, 6), h[:n * 6].view(np.float32).reshape(n, 6).copy()


def raw_trace(torch, gs, d_rays, count, n=None, flags=None, expect_rc=0):
    """rt_trace_rays_device on a device tensor [n, 6] into sentinel buffers with 64-element tails; returns
    (hits u32 [n, 4], records u32 [n, 12] or None) after checking the tails (and, for a rejected call, that
    nothing at all was written)."""
    n = d_rays.shape[0] if n is None else n
    hits = sentinel(torch, (n + TAIL) * 4)
    rec = sentinel(torch, (n + TAIL) * 12) if count else None
    if flags is None:
        flags = rtm.RT_RAYS_COUNT if count else 0
    L = rtm.tracer_lib()
    rc = L.rt_trace_rays_device(gs._h, ctypes.c_void_p(d_rays.data_ptr()), n, flags, ctypes.c_void_p(hits.data_ptr()),
                                ctypes.c_void_p(rec.data_ptr()) if count else None, ctypes.c_void_p(stream_of(torch)))
    assert rc == expect_rc, rc
    torch.cuda.synchronize()
    h = host_u32(hits)
    r = host_u32(rec) if count else None
    written = n if rc == 0 else 0
    assert (h[written * 4:] == S.SENTINEL).all(), "hits written past n"
    assert not (h[:written * 4] == S.SENTINEL).any(), "hits left unwritten"
    if count:
        assert (r[written * 12:] == S.SENTINEL).all(), "records written past n"
        assert not (r[:written * 12] == S.SENTINEL).any(), "records left unwritten"
        r = r[:written * 12].reshape(written, 12)
    return h[:written * 4].reshape(written, 4), r


def hits_as_rec12(h):
    """rt_ray_hit words [n, 4] -> rt_sample_rec words with the columns a hit record defines."""
    rec = np.zeros((h.shape[0], 12), np.uint32)
    rec[:, 0] = h[:, 0] != NOTRI
    rec[:, 1] = h[:, 0]
    rec[:, 5:8] = h[:, 1:4]
    return rec


def check_count(h, r, e, what):
    """The counting arm against fixture entry e: the eight geometric columns; r = g = b = pad = 0; and its
    rt_ray_hit output equal to the record's tri, t, u, v."""
    assert (r[:, 8:] == 0).all(), what
    S.check_rec11(S.to_rec11(r), e, cols=GEOM_COLS, what=what)
    np.testing.assert_array_equal(hits_as_rec12(h)[:, [0, 1, 5, 6, 7]], r[:, [0, 1, 5, 6, 7]], err_msg=what)
    miss = r[:, 0] == 0
    assert (r[miss, 1] == NOTRI).all() and (r[miss, 5:8] == 0).all(), what


def check_fast(h, e, what):
    miss = h[:, 0] == NOTRI
    assert (h[miss, 1:] == 0).all(), what
    S.check_rec11(S.to_rec11(hits_as_rec12(h)), e, cols=FAST_COLS, what=what)


def check_sorted(torch, gs, d_rays, hits, rec, n=None):
    """RT_RAYS_SORT (alone, and with RT_RAYS_COUNT when rec is given) gives the unsorted call's bits, in
    input order."""
    SORT = rtm.RT_RAYS_SORT
    np.testing.assert_array_equal(raw_trace(torch, gs, d_rays, False, n=n, flags=SORT)[0], hits, err_msg="sorted fast arm")
    if rec is not None:
        h, r = raw_trace(torch, gs, d_rays, True, n=n, flags=SORT | rtm.RT_RAYS_COUNT)
        np.testing.assert_array_equal(h, hits, err_msg="sorted count arm: hits")
        np.testing.assert_array_equal(r, rec, err_msg="sorted count arm: records")


def frame_for(gs, W, H, spp, cam=None, fov=None):
    f = gs.frame(W, H, spp)
    if cam is not None:
        for k in range(16):
            f.cam[k] = float(cam[k])
        f.fov = float(fov)
    return f


def check_genray(oracle, rays, f):
    """rays [n, 6] (y, x, sample order) against the reference's GenerateRay for the same pixel, sample, W, H,
    camera and fov (orc_kat_genray's 23-word input: cam[16], px, py, W, H as integer bits, sx, sy, fov)."""
    W, H, spp = f.width, f.height, max(1, f.spp)
    smp = rtm.sample_table(spp)
    y, x, s = [a.reshape(-1) for a in np.meshgrid(np.arange(H), np.arange(W), np.arange(spp), indexing="ij")]
    rin = np.zeros((W * H * spp, 23), np.float32)
    rin[:, :16] = np.array(list(f.cam), np.float32)
    bits = rin.view(np.uint32)
    bits[:, 16], bits[:, 17], bits[:, 18], bits[:, 19] = x, y, W, H
    rin[:, 20], rin[:, 21], rin[:, 22] = smp[s, 0], smp[s, 1], np.float32(f.fov)
    exp = oracle.kat("genray", rin, 6)
    np.testing.assert_array_equal(rays.view(np.uint32), exp.view(np.uint32), err_msg="primary rays vs GenerateRay")


def frames_of(e):
    return [e] + ([e["axis_frame"]] if "axis_frame" in e else [])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rays")
    cache = {}

    def get(entry):
        key = entry["scene"]
        if key not in cache:
            hs = rtm.HostScene.load(S.scene_file(entry, tmp))
            cache[key] = (hs, rtm.GpuScene(hs, 0))
        return cache[key]
    get.tmp = tmp
    yield get
    for hs, gs in cache.values():
        gs.close()
        hs.close()


@pytest.fixture(scope="module")
def camera_sets(scenes, oracle):
    """Per shipped scene: the sixteen seeded cameras' rays (96x54x4 each) concatenated on the device, the
    cameras' fixture entries, and the fast arm's result for them in camera order -- computed once."""
    cache = {}

    def get(scene):
        if scene not in cache:
            import torch
            hs, gs = scenes({"scene": scene})
            views = [v for _, v in sorted(META["cameras"].items()) if v["scene"] == scene]
            assert len(views) == 16
            parts = []
            for v in views:
                f = frame_for(gs, v["W"], v["H"], v["spp"], S.bits_f32(v["cam_bits"]), S.bits_f32([v["fov_bits"]])[0])
                d, h = raw_primary(torch, gs, f)
                check_genray(oracle, h, f)
                parts.append(d)
            rays = torch.cat(parts).contiguous()
            quiet, _ = raw_trace(torch, gs, rays, False)
            cache[scene] = (gs, views, rays, quiet)
        return cache[scene]
    return get


# ------------------------------------------------------------------ 1. reference-pinned, camera order
@pytest.mark.parametrize("name", CASES)
def test_camera_rays_match_the_reference(scenes, oracle, name):
    """Every synthetic case at 62x46x4 (and 63x47x4 for the axis cases): the primary rays against GenerateRay,
    then both arms against the reference's records.  stack2100 (packed_cells == 0) walks the plain CSR
    fallback; the others the box runs."""
    import torch
    for e in frames_of(META["cases"][name]):
        hs, gs = scenes(e)
        f = gs.frame(e["W"], e["H"], e["spp"])
        d_rays, rays = raw_primary(torch, gs, f)
        check_genray(oracle, rays, f)
        h, r = raw_trace(torch, gs, d_rays, True)
        check_count(h, r, e, f"{e['name']} count arm")
        h, _ = raw_trace(torch, gs, d_rays, False)
        check_fast(h, e, f"{e['name']} fast arm")
    info = gs.info()
    assert info["packed_cells"] == (0 if name == "stack2100" else 1), info


def test_python_surface_equals_the_raw_calls(scenes):
    """GpuScene.primary_rays / trace_rays (torch tensors, zero-copy; numpy, uploaded) return the raw calls' bits."""
    import torch
    e = META["cases"]["inside"]
    hs, gs = scenes(e)
    f = gs.frame(e["W"], e["H"], e["spp"])
    d_rays, rays = raw_primary(torch, gs, f)
    got = gs.primary_rays(f)
    assert got.dtype == torch.float32 and tuple(got.shape) == (e["W"] * e["H"] * e["spp"], 6) and got.is_cuda
    np.testing.assert_array_equal(host_u32(got), rays.view(np.uint32))
    h, r = raw_trace(torch, gs, d_rays, True)
    for src in (d_rays, rays):
        for count in (False, True):
            res = gs.trace_rays(src, count=count)
            torch.cuda.synchronize()
            is_t = isinstance(src, torch.Tensor)
            col = (lambda a: host_u32(a.contiguous())) if is_t else (lambda a: np.ascontiguousarray(a).view(np.uint32))
            assert (res.tri.is_cuda if is_t else isinstance(res.tri, np.ndarray))
            for k, name in enumerate(("tri", "t", "u", "v")):
                np.testing.assert_array_equal(col(getattr(res, name)), h[:, k], err_msg=f"{name} count={count}")
            if count:
                words = host_u32(res.rec) if is_t else res.rec.view(np.uint32).reshape(-1, 12)
                assert is_t or res.rec.dtype == rtm.SAMPLE_REC_DTYPE
                np.testing.assert_array_equal(words, r)
            else:
                assert res.rec is None
    for count in (False, True):
        res = gs.trace_rays(d_rays, count=count, sort=True)
        np.testing.assert_array_equal(host_u32(res.hits), h, err_msg=f"sort=True count={count}")
        if count:
            np.testing.assert_array_equal(host_u32(res.rec), r)


# ------------------------------------------------------------------ 2. incoherent, reference-pinned
def test_shuffled_views_of_one_mesh(scenes, oracle):
    """Seven cases share one mesh byte for byte; their 79,856 camera rays, shuffled with PCG64(41), traced as
    one call on ONE scene, un-shuffled, must give each view's own fixture -- with both arms."""
    import torch
    bodies = set()
    for name in SHARED_MESH:
        with gzip.open(os.path.join(S.SYNTH, name + ".rtscene.gz"), "rb") as fh:
            bodies.add(hashlib.sha256(fh.read()[80:]).hexdigest())
    assert len(bodies) == 1, "the seven cases no longer share one mesh"
    ents = [META["cases"][n] for n in SHARED_MESH]
    assert sum(e["hit_samples"] for e in ents) == 20548 and sum(e["miss_samples"] for e in ents) == 59308
    _, gs = scenes(ents[0])
    parts = []
    for e in ents:
        hs = rtm.HostScene.load(S.scene_file(e, scenes.tmp))
        try:
            f = frame_for(gs, e["W"], e["H"], e["spp"], hs.cam, hs.fov)
        finally:
            hs.close()
        d, h = raw_primary(torch, gs, f)
        check_genray(oracle, h, f)
        parts.append(d)
    rays = torch.cat(parts).contiguous()
    n = rays.shape[0]
    assert n == 79856
    perm = np.random.Generator(np.random.PCG64(41)).permutation(n)
    shuffled = rays[torch.from_numpy(perm).cuda()].contiguous()
    hc, rc = raw_trace(torch, gs, shuffled, True)
    hf, _ = raw_trace(torch, gs, shuffled, False)
    check_sorted(torch, gs, shuffled, hf, rc)
    inv = np.argsort(perm)
    hc, rc, hf = hc[inv], rc[inv], hf[inv]
    assert int((rc[:, 0] == 1).sum()) == 20548
    o = 0
    for e in ents:
        k = e["W"] * e["H"] * e["spp"]
        check_count(hc[o:o + k], rc[o:o + k], e, f"shuffled {e['name']} count arm")
        check_fast(hf[o:o + k], e, f"shuffled {e['name']} fast arm")
        o += k


@pytest.mark.parametrize("scene", ["scene8", "scene1"])
def test_shuffled_seeded_cameras(camera_sets, scene):
    """Sixteen seeded cameras of a shipped scene (331,776 rays): in camera order and shuffled with PCG64(41),
    both arms; each camera's un-shuffled tri column must hash to the reference's hits_sha256."""
    import torch
    gs, views, rays, quiet = camera_sets(scene)
    n = rays.shape[0]
    assert n == 331776
    perm = np.random.Generator(np.random.PCG64(41)).permutation(n)
    shuffled = rays[torch.from_numpy(perm).cuda()].contiguous()
    inv = np.argsort(perm)
    hf = raw_trace(torch, gs, shuffled, False)[0]
    hc, rc = raw_trace(torch, gs, shuffled, True)
    check_sorted(torch, gs, shuffled, hf, rc)
    check_sorted(torch, gs, rays, quiet, None)
    hf, hc, rc = hf[inv], hc[inv], rc[inv]
    np.testing.assert_array_equal(hf, quiet, err_msg="shuffled fast arm vs camera order")
    np.testing.assert_array_equal(hc, quiet, err_msg="shuffled count arm vs fast arm")
    np.testing.assert_array_equal(hits_as_rec12(hc)[:, [0, 1, 5, 6, 7]], rc[:, [0, 1, 5, 6, 7]])
    o = 0
    for v in views:
        k = v["W"] * v["H"] * v["spp"]
        for arm, h in (("camera order", quiet), ("fast", hf), ("count", hc)):
            assert sha(h[o:o + k, 0]) == v["hits_sha256"], (scene, v["view"], arm)
        assert int((quiet[o:o + k, 0] != NOTRI).sum()) == v["hit_samples"], v["view"]
        o += k


# ------------------------------------------------------------------ 3. sizes
def test_sizes_and_an_offset_view(scenes):
    """n = 0, 1, 63, 64, 65, 255, 256, 257 from the front of `inside`'s rays, and a view that starts at row 1
    (24 bytes into the allocation): each equals the corresponding slice of the full call."""
    import torch
    e = META["cases"]["inside"]
    hs, gs = scenes(e)
    d_rays, _ = raw_primary(torch, gs, gs.frame(e["W"], e["H"], e["spp"]))
    full_c = raw_trace(torch, gs, d_rays, True)
    full_f = raw_trace(torch, gs, d_rays, False)[0]
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        h, r = raw_trace(torch, gs, d_rays, True, n=n)
        np.testing.assert_array_equal(h, full_c[0][:n])
        np.testing.assert_array_equal(r, full_c[1][:n])
        np.testing.assert_array_equal(raw_trace(torch, gs, d_rays, False, n=n)[0], full_f[:n])
        check_sorted(torch, gs, d_rays, full_f[:n], full_c[1][:n], n=n)       # (its scratch grows with n)
    check_sorted(torch, gs, d_rays, full_f, full_c[1])
    check_sorted(torch, gs, d_rays, full_f[:65], full_c[1][:65], n=65)        # ... and is kept for a smaller n
    view = d_rays[1:]
    assert view.data_ptr() == d_rays.data_ptr() + 24 and view.is_contiguous()
    np.testing.assert_array_equal(raw_trace(torch, gs, view, False)[0], full_f[1:])
    h, r = raw_trace(torch, gs, view, True)
    np.testing.assert_array_equal(r, full_c[1][1:])
    res = gs.trace_rays(view)
    np.testing.assert_array_equal(host_u32(res.hits), full_f[1:])
    empty = gs.trace_rays(d_rays[:0])
    assert tuple(empty.hits.shape) == (0, 4)


# ------------------------------------------------------------------ 4. arms agree on rays no camera makes
def unit_dirs(r, n):
    d = r.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def off_camera_rays(rays, rec, lo, hi):
    """Secondary rays (4 seeded unit directions from every primary hit point), 4,096 rays from origins uniform in
    3x the grid box, 512 exact +-axis directions and 512 with one or two exactly +-0 components."""
    r = np.random.Generator(np.random.PCG64(43))
    hit = rec[:, 0] == 1
    t = rec[hit, 5].view(np.float32)
    p = (rays[hit, :3] + rays[hit, 3:] * t[:, None]).astype(np.float32)
    sec = np.concatenate([np.repeat(p, 4, axis=0), unit_dirs(r, 4 * p.shape[0])], axis=1)
    ctr, ext = (lo + hi) * np.float32(0.5), (hi - lo)
    org = (ctr + 1.5 * ext * r.uniform(-1, 1, (4096, 3))).astype(np.float32)
    wide = np.concatenate([org, unit_dirs(r, 4096)], axis=1)
    org = (ctr + 0.75 * ext * r.uniform(-1, 1, (512, 3))).astype(np.float32)
    ax = np.zeros((512, 3), np.float32)
    ax[np.arange(512), r.integers(0, 3, 512)] = r.choice(np.array([-1.0, 1.0], np.float32), 512)
    axis = np.concatenate([org, ax], axis=1)
    org = (ctr + 0.75 * ext * r.uniform(-1, 1, (512, 3))).astype(np.float32)
    dz = unit_dirs(r, 512)
    zero = r.choice(np.array([0.0, -0.0], np.float32), (512, 3))
    for k in range(512):
        idx = r.permutation(3)[: 1 + k % 2]             # one or two components
        dz[k, idx] = zero[k, idx]
    zeros = np.concatenate([org, dz], axis=1)
    assert (np.count_nonzero(dz, axis=1) >= 1).all() and (np.count_nonzero(dz, axis=1) <= 2).all()
    return np.ascontiguousarray(np.concatenate([sec, wide, axis, zeros]), np.float32)


@pytest.mark.parametrize("name", ["inside", "stack1500"])
def test_arms_agree_off_camera(scenes, name):
    """The fast arm's tri, t, u, v equal the counting arm's, bit for bit, on rays no camera makes; the set must
    hold at least 1,000 hits and 1,000 misses (by the counting arm).  RT_RAYS_SORT gives the same bits on the
    same rays, with either arm.  Both arms are grid_intersect over one dda_setup, so this says nothing about a
    mistake they share: tests/test_gpu_ray_sets.py holds both to the reference's own Grid::Intersect on
    off-camera rays (tests/golden/rays)."""
    import torch
    e = META["cases"][name]
    hs, gs = scenes(e)
    d_rays, rays = raw_primary(torch, gs, gs.frame(e["W"], e["H"], e["spp"]))
    _, rec = raw_trace(torch, gs, d_rays, True)
    assert int((rec[:, 0] == 1).sum()) == e["hit_samples"]
    lo, hi = S.bits_f32(e["aabb_min_bits"]), S.bits_f32(e["aabb_max_bits"])
    gen = off_camera_rays(rays, rec, lo, hi)
    d_gen = torch.from_numpy(gen).cuda()
    hc, rc = raw_trace(torch, gs, d_gen, True)
    hf, _ = raw_trace(torch, gs, d_gen, False)
    nhit, nmiss = int((rc[:, 0] == 1).sum()), int((rc[:, 0] == 0).sum())
    print(f"{name}: {gen.shape[0]} rays, {nhit} hits, {nmiss} misses by the counting arm")
    assert nhit >= 1000 and nmiss >= 1000, (name, nhit, nmiss)
    np.testing.assert_array_equal(hf, hc, err_msg=f"{name}: fast arm vs counting arm")
    np.testing.assert_array_equal(hits_as_rec12(hc)[:, [0, 1, 5, 6, 7]], rc[:, [0, 1, 5, 6, 7]])
    check_sorted(torch, gs, d_gen, hc, rc)
    # The direction is used as passed: the same rays with their directions scaled by 2^-10, 7.9, 8.0, 8.5 and
    # 2^10 -- whole waves of one factor (64 consecutive rays each), then every ray a factor of its own, so the
    # wave's choice between the Newton reciprocal (|d|_inf <= 8) and the division goes both ways and splits
    # waves.  The counting arm always divides: equal bits pin the reciprocal's exactness up to 8.
    fac = np.array([2.0 ** -10, 7.9, 8.0, 8.5, 2.0 ** 10], np.float32)
    half = min(gen.shape[0] // 2, 6400)
    scaled = np.concatenate([gen[-1024:], gen[:2 * half - 1024]])       # the axis and zero-component rays first
    per_wave = fac[(np.arange(half) // 64) % 5]
    per_ray = fac[np.arange(half) % 5]
    scaled[:half, 3:] *= per_wave[:, None]
    scaled[half:, 3:] *= per_ray[:, None]
    dm = np.abs(scaled[:, 3:]).max(1)
    assert (dm > 8).sum() > 1000 and (dm <= 8).sum() > 1000 and (dm == 8).any()
    d_sc = torch.from_numpy(scaled).cuda()
    hc, rc = raw_trace(torch, gs, d_sc, True)
    hf, _ = raw_trace(torch, gs, d_sc, False)
    assert int((rc[:, 0] == 1).sum()) >= 500 and int((rc[:, 0] == 0).sum()) >= 500
    np.testing.assert_array_equal(hf, hc, err_msg=f"{name}: scaled directions, fast arm vs counting arm")
    check_sorted(torch, gs, d_sc, hc, rc)


def gate_clear(rays, hs, k):
    """Rays none of whose ray/triangle determinants can change sides of IntersectRayTri's |det| < 1e-8 gate
    (triangle.h:77) when the direction is scaled by 2^k: every |det| (fp64, all triangles of the mesh) at
    least 1e-6 -- the float32 evaluation's error bound, generously -- above the larger of 1e-8 and 1e-8 2^-k."""
    v, t = hs.mesh()
    p0, p1, p2 = (v[t[:, j], :3].astype(np.float32) for j in range(3))
    e1, e2 = (p1 - p0).astype(np.float64), (p2 - p0).astype(np.float64)
    d = rays[:, 3:].astype(np.float64)
    det = np.einsum("tj,rtj->rt", e1, np.cross(d[:, None, :], e2[None, :, :]))
    return (np.abs(det) > 1e-8 * max(1.0, 2.0 ** -k) + 1e-6).all(1)


@pytest.mark.parametrize("k", [-10, 3, 4, 10])
@pytest.mark.parametrize("name", ["inside", "axis_x"])
def test_scaled_directions_against_the_reference(scenes, name, k):
    """d is NOT normalised: the camera rays with every direction scaled by 2^k.  All of Grid::Intersect scales
    exactly with a power of two -- the box entry, the crossing times, det, and u, v not at all -- so hit, tri,
    voxel, steps, tests, u and v must equal the reference's records and t must be the reference's t times 2^-k,
    bit for bit, wherever no determinant crosses the absolute 1e-8 gate (gate_clear; at least 90 % of the
    rays, or the test fails).  2^3 keeps |d|_inf <= 8 (the Newton reciprocal's walk), 2^4 and 2^10 take the
    division's walk, 2^-10 a short direction.  Fast arm, counting arm and RT_RAYS_SORT."""
    import torch
    e = META["cases"][name]
    hs, gs = scenes(e)
    d_rays, rays = raw_primary(torch, gs, gs.frame(e["W"], e["H"], e["spp"]))
    h0, r0 = raw_trace(torch, gs, d_rays, True)
    check_count(h0, r0, e, f"{name} unscaled")
    scaled = rays.copy()
    scaled[:, 3:] = np.ldexp(rays[:, 3:], k)
    d_sc = torch.from_numpy(scaled).cuda()
    hc, rc = raw_trace(torch, gs, d_sc, True)
    hf, _ = raw_trace(torch, gs, d_sc, False)
    np.testing.assert_array_equal(hf, hc, err_msg="scaled: fast arm vs counting arm")
    check_sorted(torch, gs, d_sc, hc, rc)
    clear = gate_clear(rays, hs, k)
    print(f"{name} 2^{k}: {int(clear.sum())} of {clear.size} rays clear of the gate, {int((r0[clear, 0] == 1).sum())} hits")
    assert clear.mean() >= 0.9
    want = r0.copy()
    want[:, 5] = np.ldexp(r0[:, 5].view(np.float32), -k).view(np.uint32)
    np.testing.assert_array_equal(rc[clear], want[clear], err_msg=f"{name}: records of directions scaled by 2^{k}")


# ------------------------------------------------------------------ 5. non-finite rays
def test_non_finite_rays_are_defined_misses(scenes):
    """64 rays with a NaN, +inf or -inf in each of the six components in turn, mixed into 1,024 ordinary rays:
    the 64 report the documented miss, the others what a call without them reports."""
    import torch
    e = META["cases"]["inside"]
    hs, gs = scenes(e)
    d_rays, rays = raw_primary(torch, gs, gs.frame(e["W"], e["H"], e["spp"]))
    r = np.random.Generator(np.random.PCG64(45))
    base = rays[r.choice(rays.shape[0], 1024, replace=False)]
    bad = rays[r.choice(rays.shape[0], 64, replace=False)].copy()
    vals = np.array([np.nan, np.inf, -np.inf], np.float32)
    for k in range(64):
        bad[k, k % 6] = vals[(k // 6) % 3]
    where = np.sort(r.choice(1088, 64, replace=False))
    is_bad = np.zeros(1088, bool)
    is_bad[where] = True
    mixed = np.zeros((1088, 6), np.float32)
    mixed[is_bad], mixed[~is_bad] = bad, base
    clean_c = raw_trace(torch, gs, torch.from_numpy(base).cuda(), True)
    clean_f = raw_trace(torch, gs, torch.from_numpy(base).cuda(), False)[0]
    assert 0 < int((clean_f[:, 0] != NOTRI).sum()) <= 1024
    hc, rc = raw_trace(torch, gs, torch.from_numpy(mixed).cuda(), True)
    hf, _ = raw_trace(torch, gs, torch.from_numpy(mixed).cuda(), False)
    check_sorted(torch, gs, torch.from_numpy(mixed).cuda(), hf, rc)          # (they sort last: the largest key)
    miss_hit = np.array([NOTRI, 0, 0, 0], np.uint32)
    miss_rec = np.array([0, NOTRI, NOTRI, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.uint32)
    for h in (hc, hf):
        assert (h[is_bad] == miss_hit).all()
    assert (rc[is_bad] == miss_rec).all()
    np.testing.assert_array_equal(hf[~is_bad], clean_f)
    np.testing.assert_array_equal(hc[~is_bad], clean_c[0])
    np.testing.assert_array_equal(rc[~is_bad], clean_c[1])


# ------------------------------------------------------------------ 6. no interference
def test_rays_beside_render_launches(camera_sets, golden):
    """A 1920x1080x4 render_frame_device of scene 8 and a trace_rays of the same scene on another stream,
    interleaved 8 times without a host wait: every frame has the golden SHA, every ray result the bits of the
    quiet call (which test_shuffled_seeded_cameras pins to the reference)."""
    import torch
    gs, views, rays, quiet = camera_sets("scene8")
    W, H, spp = 1920, 1080, 4
    f = gs.frame(W, H, spp)
    s_frame, s_rays, s_rays2 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    outs = [sentinel(torch, W * H) for _ in range(8)]
    hits = [sentinel(torch, (rays.shape[0] + TAIL) * 4) for _ in range(8)]
    L = rtm.tracer_lib()
    torch.cuda.synchronize()
    for i in range(8):
        gs.render_frame_device(f, outs[i].data_ptr(), s_frame.cuda_stream)
        # calls 2, 3, 6, 7 sorted, on alternating streams: they share the scene's sort scratch
        flags, st = (rtm.RT_RAYS_SORT if i & 2 else 0), (s_rays2 if i & 1 else s_rays)
        assert L.rt_trace_rays_device(gs._h, ctypes.c_void_p(rays.data_ptr()), rays.shape[0], flags,
                                      ctypes.c_void_p(hits[i].data_ptr()), None, ctypes.c_void_p(st.cuda_stream)) == 0
    torch.cuda.synchronize()
    n = rays.shape[0]
    for i in range(8):
        assert sha(host_u32(outs[i])) == golden["frames_1080p4"]["8"]["bgra_sha256"], i
        h = host_u32(hits[i])
        assert (h[n * 4:] == S.SENTINEL).all()
        np.testing.assert_array_equal(h[:n * 4].reshape(n, 4), quiet, err_msg=f"rays beside frame {i}")


# ------------------------------------------------------------------ 7. argument checks
def test_argument_checks_on_a_live_scene(scenes):
    """NULL and misaligned device pointers and d_recs without RT_RAYS_COUNT are RT_E_INVALID and write nothing;
    host memory never reaches the library: the Python layer uploads a numpy array and refuses a CPU tensor."""
    import torch
    e = META["cases"]["inside"]
    hs, gs = scenes(e)
    d_rays, rays = raw_primary(torch, gs, gs.frame(e["W"], e["H"], e["spp"]))
    n = 256
    hits, rec = sentinel(torch, n * 4 + 2), sentinel(torch, n * 12 + 2)
    L, st = rtm.tracer_lib(), ctypes.c_void_p(stream_of(torch))
    vp = ctypes.c_void_p
    R, Hp, Rp = d_rays.data_ptr(), hits.data_ptr(), rec.data_ptr()
    CNT = rtm.RT_RAYS_COUNT
    for args in ((None, n, 0, vp(Hp), None), (vp(R), n, 0, None, None), (vp(R), n, CNT, vp(Hp), None),
                 (vp(R), n, 0, vp(Hp), vp(Rp)), (vp(R + 4), n, 0, vp(Hp), None), (vp(R), n, 0, vp(Hp + 4), None),
                 (vp(R), n, CNT, vp(Hp), vp(Rp + 4)), (vp(R), n, 8, vp(Hp), None)):
        assert L.rt_trace_rays_device(gs._h, *args, st) == 1, args
    f = gs.frame(8, 8, 1)
    assert L.rt_primary_rays_device(gs._h, ctypes.byref(f), None, st) == 1
    assert L.rt_primary_rays_device(gs._h, ctypes.byref(f), vp(Hp + 4), st) == 1
    torch.cuda.synchronize()
    assert (host_u32(hits) == S.SENTINEL).all() and (host_u32(rec) == S.SENTINEL).all()
    with pytest.raises(ValueError):
        gs.trace_rays(torch.from_numpy(rays[:n]))                  # a CPU tensor: refused, not probed
    with pytest.raises(ValueError):
        gs.trace_rays(d_rays[:, :3])
    with pytest.raises(ValueError):
        gs.trace_rays(d_rays[::2])
    with pytest.raises(ValueError):
        gs.trace_rays(d_rays.double())
    up = gs.trace_rays(rays[:n])                                   # numpy: uploaded, results downloaded
    np.testing.assert_array_equal(up.hits.view(np.uint32).reshape(n, 4), raw_trace(torch, gs, d_rays, False, n=n)[0])
