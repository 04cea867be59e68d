"""rt_occluded_rays_device (GpuScene.occluded) on the GPU: byte-exact against tests/occlusion_ref.py -- the numpy
restatement of the any-hit walk, which tests/test_occlusion_cpu.py pins to the reference's records -- and against
the fixtures of tests/golden/synth where the fixture decides (the infinite interval: the reference's own hit).

Every output buffer is pre-filled with 0x5A and carries 64 bytes past n, which must still hold 0x5A afterwards;
every written byte must be 0 or 1.  Every call is repeated with RT_RAYS_SORT and must give the same bytes (occl).
The camera rays come from rt_primary_rays_device (tests/test_gpu_rays.py pins them to the reference's GenerateRay).
"""
import ctypes

import numpy as np
import pytest

import occlusion_ref as R
import synth_scenes as S
from conftest import load_package

pytestmark = pytest.mark.gpu
rtm = load_package()
META = S.meta()
CASES = sorted(META["cases"])
NOTRI = 0xFFFFFFFF
TAIL = 64
FILL = 0x5A
FAST_COLS = ("hit", "tri", "t", "u", "v")
INF = np.float32(np.inf)


# ------------------------------------------------------------------ helpers
def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def raw_occluded(torch, gs, d_rays, d_tmm, n=None, flags=0, expect_rc=0):
    """One rt_occluded_rays_device call into a 0x5A-filled buffer with a 64-byte tail -> bytes u8 [n] (a rejected
    call: an empty array, after checking that nothing at all was written)."""
    n = d_rays.shape[0] if n is None else n
    out = torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    rc = rtm.tracer_lib().rt_occluded_rays_device(gs._h, vp(d_rays), vp(d_tmm), n, flags, vp(out),
                                                  ctypes.c_void_p(stream_of(torch)))
    assert rc == expect_rc, (rc, expect_rc)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    written = n if rc == 0 else 0
    assert (h[written:] == FILL).all(), "bytes written past n"
    assert (h[:written] <= 1).all(), "a byte that is neither 0 nor 1 (or left unwritten)"
    return h[:written].copy()


def occl(torch, gs, d_rays, d_tmm, n=None):
    """The plain call and the RT_RAYS_SORT call: the same bytes, in input order."""
    plain = raw_occluded(torch, gs, d_rays, d_tmm, n=n)
    np.testing.assert_array_equal(raw_occluded(torch, gs, d_rays, d_tmm, n=n, flags=rtm.RT_RAYS_SORT), plain,
                                  err_msg="RT_RAYS_SORT vs the plain call")
    return plain


def primary(torch, gs, e):
    """(device rays [n, 6], host copy) of a fixture entry's frame."""
    d = gs.primary_rays(gs.frame(e["W"], e["H"], e["spp"]))
    torch.cuda.synchronize()
    return d, d.cpu().numpy()


def closest(torch, gs, d_rays):
    """rt_trace_rays_device's fast arm -> u32 words [n, 4] (tri, t, u, v)."""
    res = gs.trace_rays(d_rays)
    torch.cuda.synchronize()
    return res.hits.cpu().numpy().view(np.uint32)


def hits_as_rec11(h):
    rec = np.zeros((h.shape[0], 12), np.uint32)
    rec[:, 0] = h[:, 0] != NOTRI
    rec[:, 1] = h[:, 0]
    rec[:, 5:8] = h[:, 1:4]
    return S.to_rec11(rec)


def frames_of(e):
    return [e] + ([e["axis_frame"]] if "axis_frame" in e else [])


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mixed_intervals(t_ref, is_hit, diag):
    """Per ray, tmax cycles through {t_ref, nextafter(t_ref, +inf), nextafter(t_ref, -inf), 0.5 t_ref, the box
    diagonal, +inf} and tmin through {-inf, 0, t_ref, nextafter(t_ref, -inf), 0.5 t_ref} (6 x 5 = 30 combinations,
    neighbours in a wave all different); a miss uses 0.37 x the diagonal in place of t_ref."""
    n = t_ref.shape[0]
    t = np.where(is_hit, t_ref, np.float32(0.37) * diag).astype(np.float32)
    i = np.arange(n)
    half = (np.float32(0.5) * t).astype(np.float32)
    tmax = np.choose(i % 6, [t, np.nextafter(t, INF), np.nextafter(t, -INF), half, np.full(n, diag, np.float32),
                             np.full(n, INF)]).astype(np.float32)
    tmin = np.choose((i // 6) % 5, [np.full(n, -INF), np.zeros(n, np.float32), t, np.nextafter(t, -INF), half]).astype(np.float32)
    return np.ascontiguousarray(np.stack([tmin, tmax], axis=1), np.float32)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """Per scene file: (HostScene, GpuScene, RefScene), loaded once."""
    tmp = tmp_path_factory.mktemp("occl")
    cache = {}

    def get(entry):
        key = entry["scene"]
        if key not in cache:
            hs = rtm.HostScene.load(S.scene_file(entry, tmp))
            cache[key] = (hs, rtm.GpuScene(hs, 0), R.RefScene.from_host(hs))
        return cache[key]
    yield get
    for hs, gs, _ in cache.values():
        gs.close()
        hs.close()


# ------------------------------------------------------------------ 1. the infinite interval: the fixtures decide
@pytest.mark.parametrize("name", CASES)
def test_infinite_interval_equals_the_reference_hit(scenes, name):
    """All 21 views (and the 63x47 axis frames): occluded == the reference's hit, in camera order and shuffled, with
    d_tminmax = NULL and with an explicit (-inf, +inf) array.  stack2100 walks the plain CSR ranges, the others the
    box runs."""
    import torch
    for e in frames_of(META["cases"][name]):
        hs, gs, sc = scenes(e)
        d_rays, rays = primary(torch, gs, e)
        h = closest(torch, gs, d_rays)
        S.check_rec11(hits_as_rec11(h), e, cols=FAST_COLS, what="closest hit")       # h IS the fixture's hit, tri, t
        want = (h[:, 0] != NOTRI).astype(np.uint8)
        assert int(want.sum()) == e["hit_samples"]
        n = rays.shape[0]
        got = occl(torch, gs, d_rays, None)
        np.testing.assert_array_equal(got, want, err_msg=f"{e['name']}: NULL interval, camera order")
        inf = dev(torch, np.tile(np.array([-INF, INF], np.float32), (n, 1)))
        np.testing.assert_array_equal(occl(torch, gs, d_rays, inf), want, err_msg=f"{e['name']}: explicit (-inf, +inf)")
        perm = np.random.Generator(np.random.PCG64(51)).permutation(n)
        shuffled = d_rays[torch.from_numpy(perm).cuda()].contiguous()
        np.testing.assert_array_equal(occl(torch, gs, shuffled, None), want[perm], err_msg=f"{e['name']}: shuffled")
    assert gs.info()["packed_cells"] == (0 if name == "stack2100" else 1)


# ------------------------------------------------------------------ 2. intervals, mixed inside waves
@pytest.mark.parametrize("name", CASES)
def test_intervals_mixed_inside_waves(scenes, name):
    """The same rays with per-ray intervals around each ray's own closest t (mixed_intervals), against the
    restatement.  On stack1500 / stack2100 the nearest triangle is the LAST of a 1,500 / 2,100 long list: the early
    exit inside the list and tmin past the nearest triangle both decide bytes there."""
    import torch
    for e in frames_of(META["cases"][name]):
        hs, gs, sc = scenes(e)
        d_rays, rays = primary(torch, gs, e)
        h = closest(torch, gs, d_rays)
        is_hit = h[:, 0] != NOTRI
        tmm = mixed_intervals(h[:, 1].view(np.float32), is_hit, sc.diagonal())
        want = R.walk(sc, rays, tmm, mode="any")["occluded"].astype(np.uint8)
        got = occl(torch, gs, d_rays, dev(torch, tmm))
        print(f"{e['name']}: {int(is_hit.sum())} closest hits, {int(want.sum())} of {want.size} occluded over the mixed intervals")
        np.testing.assert_array_equal(got, want, err_msg=f"{e['name']}: mixed intervals vs the restatement")
        if not e["all_miss"]:
            # the intervals decide: some hit rays are occluded, and some are not
            assert 0 < int(want[is_hit].sum()) < int(is_hit.sum())


# ------------------------------------------------------------------ 3. rays no camera makes
def hemisphere_rays(sc, rays, h, limit, seed):
    """Origins at the closest hit points o + t d (f32), 4 seeded unit directions each in the hemisphere of the hit
    triangle's geometric normal that faces the incoming ray; at most `limit` rays."""
    r = np.random.Generator(np.random.PCG64(seed))
    hit = np.flatnonzero(h[:, 0] != NOTRI)
    hit = hit[r.permutation(hit.size)[: limit // 4]]
    t = h[hit, 1].view(np.float32)
    p = (rays[hit, :3] + rays[hit, 3:] * t[:, None]).astype(np.float32)
    tri = h[hit, 0].astype(np.int64)
    nrm = np.cross((sc.v1[tri] - sc.v0[tri]).astype(np.float64), (sc.v2[tri] - sc.v0[tri]).astype(np.float64))
    nrm *= -np.sign((nrm * rays[hit, 3:]).sum(1, keepdims=True))
    p, nrm = np.repeat(p, 4, axis=0), np.repeat(nrm, 4, axis=0)
    d = r.normal(size=p.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.where((d * nrm).sum(1, keepdims=True) < 0, -1.0, 1.0)
    return np.ascontiguousarray(np.concatenate([p, d.astype(np.float32)], axis=1), np.float32)


@pytest.mark.parametrize("name", ["inside", "degenerate", "stack1500"])
def test_hemisphere_rays_from_hit_points(scenes, name):
    """An ambient-occlusion bounce, 4 rays from every closest hit point (at most 40,000): tmin = 1e-4, tmax cycling
    through {0.05, 0.5, +inf} per ray, in bounce order and shuffled, against the restatement."""
    import torch
    limit = 40000
    e = META["cases"][name]
    hs, gs, sc = scenes(e)
    d_rays, rays = primary(torch, gs, e)
    gen = hemisphere_rays(sc, rays, closest(torch, gs, d_rays), limit, 53)
    n = gen.shape[0]
    assert 1000 <= n <= limit
    tmm = np.stack([np.full(n, 1e-4, np.float32), np.array([0.05, 0.5, INF], np.float32)[np.arange(n) % 3]], axis=1)
    want = R.walk(sc, gen, tmm, mode="any")["occluded"].astype(np.uint8)
    print(f"{name}: {n} hemisphere rays, {int(want.sum())} occluded; by tmax: "
          f"{[int(want[k::3].sum()) for k in range(3)]} of {[want[k::3].size for k in range(3)]}")
    assert 0 < int(want.sum()) < n
    np.testing.assert_array_equal(occl(torch, gs, dev(torch, gen), dev(torch, tmm)), want, err_msg=f"{name}: bounce order")
    perm = np.random.Generator(np.random.PCG64(54)).permutation(n)
    np.testing.assert_array_equal(occl(torch, gs, dev(torch, gen[perm]), dev(torch, tmm[perm])), want[perm],
                                  err_msg=f"{name}: shuffled")


# ------------------------------------------------------------------ 4. the direction is used as passed
def gate_clear(rays, sc, k):
    """Rays none of whose determinants can change sides of IntersectRayTri's absolute |det| < 1e-8 gate when the
    direction is scaled by 2^k (tests/test_gpu_rays.py gate_clear): every |det| (fp64, all triangles) at least 1e-6
    above the larger of 1e-8 and 1e-8 2^-k."""
    e1, e2 = (sc.v1 - sc.v0).astype(np.float64), (sc.v2 - sc.v0).astype(np.float64)
    d = rays[:, 3:].astype(np.float64)
    det = np.einsum("tj,rtj->rt", e1, np.cross(d[:, None, :], e2[None, :, :]))
    return (np.abs(det) > 1e-8 * max(1.0, 2.0 ** -k) + 1e-6).all(1)


@pytest.fixture(scope="module")
def inside_set(scenes):
    """`inside`'s camera rays with their mixed intervals and the plain call's bytes, shared by the tests below."""
    import torch
    e = META["cases"]["inside"]
    hs, gs, sc = scenes(e)
    d_rays, rays = primary(torch, gs, e)
    h = closest(torch, gs, d_rays)
    tmm = mixed_intervals(h[:, 1].view(np.float32), h[:, 0] != NOTRI, sc.diagonal())
    d_tmm = dev(torch, tmm)
    return gs, sc, d_rays, rays, d_tmm, tmm, occl(torch, gs, d_rays, d_tmm)


@pytest.mark.parametrize("k", [-10, 3, 4, 10])
def test_power_of_two_scaling(inside_set, k):
    """d x 2^k with (tmin, tmax) x 2^-k: every quantity of the walk scales exactly, so the bytes are the unscaled
    call's wherever no determinant crosses the absolute 1e-8 gate (gate_clear: at least 90 % of the rays), and the
    restatement's everywhere.  2^3 is the last length on the Newton reciprocal, 2^4 the first on the division."""
    import torch
    gs, sc, d_rays, rays, d_tmm, tmm, base = inside_set
    scaled = rays.copy()
    scaled[:, 3:] = np.ldexp(rays[:, 3:], k)
    stm = np.ldexp(tmm, -k).astype(np.float32)
    got = occl(torch, gs, dev(torch, scaled), dev(torch, stm))
    clear = gate_clear(rays, sc, k)
    assert clear.mean() >= 0.9
    np.testing.assert_array_equal(got[clear], base[clear], err_msg=f"2^{k}: scaled vs unscaled bytes")
    want = R.walk(sc, scaled, stm, mode="any")["occluded"].astype(np.uint8)
    np.testing.assert_array_equal(got, want, err_msg=f"2^{k}: scaled vs the restatement")
    assert 0 < int(got.sum()) < got.size


def test_direction_lengths_around_the_reciprocal_limit(inside_set):
    """Directions of |d|_inf = 7.9, 8.0, 8.5 (and 1) exactly -- each ray scaled to the length, then its largest
    component set to it -- per ray, so the wave's vote between the Newton reciprocal (|d|_inf <= 8) and the division
    goes both ways and splits waves; then whole waves of one length.  The intervals are scaled along.  Against the
    restatement (these are new rays: the unscaled bytes say nothing about them)."""
    import torch
    gs, sc, d_rays, rays, d_tmm, tmm, base = inside_set
    fac = np.array([7.9, 8.0, 8.5, 1.0], np.float32)
    n = rays.shape[0]
    dm0 = np.abs(rays[:, 3:]).max(1)
    major = np.abs(rays[:, 3:]).argmax(1)
    for label, f in (("per ray", fac[np.arange(n) % 4]), ("per wave", fac[(np.arange(n) // 64) % 4])):
        g = (f / dm0).astype(np.float32)
        scaled = rays.copy()
        scaled[:, 3:] *= g[:, None]
        scaled[np.arange(n), 3 + major] = np.copysign(f, rays[np.arange(n), 3 + major])
        stm = (tmm / g[:, None]).astype(np.float32)
        dm = np.abs(scaled[:, 3:]).max(1)
        assert (dm > 8).sum() > 1000 and (dm < 8).sum() > 1000 and (dm == 8).sum() > 1000
        want = R.walk(sc, scaled, stm, mode="any")["occluded"].astype(np.uint8)
        np.testing.assert_array_equal(occl(torch, gs, dev(torch, scaled), dev(torch, stm)), want, err_msg=label)
        assert 0 < int(want.sum()) < n


# ------------------------------------------------------------------ 5. sizes
def test_sizes_and_an_offset_view(inside_set):
    """n = 1, 63, 64, 65, 255, 256, 257 from the front of the set, and views that start 24 bytes (rays) and 8 bytes
    (intervals) into their allocations: each equals the slice of the full call.  n = 0 writes nothing."""
    import torch
    gs, sc, d_rays, rays, d_tmm, tmm, base = inside_set
    for n in (1, 63, 64, 65, 255, 256, 257):
        np.testing.assert_array_equal(occl(torch, gs, d_rays, d_tmm, n=n), base[:n], err_msg=f"n = {n}")
    rv, tv = d_rays[1:], d_tmm[1:]
    assert rv.data_ptr() == d_rays.data_ptr() + 24 and tv.data_ptr() == d_tmm.data_ptr() + 8
    np.testing.assert_array_equal(occl(torch, gs, rv, tv), base[1:], err_msg="offset views")
    assert occl(torch, gs, d_rays, d_tmm, n=0).size == 0         # (the tail check covers the whole buffer)
    assert occl(torch, gs, d_rays, None, n=0).size == 0
    assert tuple(gs.occluded(d_rays[:0]).shape) == (0,)


def test_python_surface_equals_the_raw_calls(inside_set):
    """GpuScene.occluded: torch tensors in place -> torch.uint8 [n] on the device; numpy uploaded -> bool [n]."""
    import torch
    gs, sc, d_rays, rays, d_tmm, tmm, base = inside_set
    none = raw_occluded(torch, gs, d_rays, None)
    for sort in (False, True):
        t = gs.occluded(d_rays, d_tmm, sort=sort)
        assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (rays.shape[0],)
        np.testing.assert_array_equal(t.cpu().numpy(), base)
        np.testing.assert_array_equal(gs.occluded(d_rays, sort=sort).cpu().numpy(), none)
        a = gs.occluded(rays, tmm, sort=sort)
        assert isinstance(a, np.ndarray) and a.dtype == bool
        np.testing.assert_array_equal(a, base.astype(bool))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    t = gs.occluded(d_rays, d_tmm, stream=side.cuda_stream)
    side.synchronize()
    np.testing.assert_array_equal(t.cpu().numpy(), base)
    with pytest.raises(ValueError):
        gs.occluded(d_rays, tmm)                     # mixed kinds
    with pytest.raises(ValueError):
        gs.occluded(d_rays, d_tmm[:-1])
    with pytest.raises(ValueError):
        gs.occluded(d_rays[::2], d_tmm[::2])
    with pytest.raises(ValueError):
        gs.occluded(torch.from_numpy(rays))          # a CPU tensor: refused, not probed


# ------------------------------------------------------------------ 6. zero without a walk
def test_zero_without_a_walk(inside_set):
    """Rays that hit over (-inf, +inf), each made void in one way -- a NaN / +inf / -inf in each ray component in
    turn, a NaN tmin, a NaN tmax, tmin == tmax, tmin > tmax -- and rays that miss the grid box, mixed into ordinary
    rays: the void ones report 0, the others what a call without them reports."""
    import torch
    gs, sc, d_rays, rays, d_tmm, tmm, base = inside_set
    r = np.random.Generator(np.random.PCG64(55))
    full = raw_occluded(torch, gs, d_rays, None)
    hitters = np.flatnonzero(full == 1)
    assert hitters.size > 200
    nbad = 18 + 4 * 8
    bad = rays[r.choice(hitters, nbad, replace=False)].copy()
    btm = np.tile(np.array([-INF, INF], np.float32), (nbad, 1))
    vals = np.array([np.nan, np.inf, -np.inf], np.float32)
    for k in range(18):
        bad[k, k % 6] = vals[k // 6]
    for j in range(8):
        t = np.float32(0.25 * (j + 1))
        btm[18 + j] = (np.nan, INF) if j % 2 else (-INF, np.nan)
        btm[26 + j] = (t, t)
        btm[34 + j] = (t, np.nextafter(t, -INF)) if j % 2 else (INF, -INF)
        btm[42 + j] = (np.nan, np.nan) if j % 2 else (0.0, -0.0)
    # rays that miss the box: origins 3 diagonals from its centre, directions at right angles to the way there
    # (a ray pointing AWAY from the box does not miss it by the reference's IntersectRayAABB, which accepts a box
    # behind the origin: such a ray walks the grid at negative t and finds nothing either)
    ctr = (sc.bmin + sc.bmax) * np.float32(0.5)
    away = r.normal(size=(64, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    side = np.cross(away, r.normal(size=(64, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    outside = np.concatenate([ctr + (away * 3.0 * float(sc.diagonal())).astype(np.float32), side.astype(np.float32)],
                             axis=1).astype(np.float32)
    assert (R.walk(sc, outside, mode="closest")["steps"] == 0).all(), "a ray meant to miss the box enters it"
    pick = r.choice(rays.shape[0], 1024, replace=False)
    clean, ctm = rays[pick], tmm[pick]
    allr = np.concatenate([clean, bad, outside])
    allt = np.concatenate([ctm, btm, np.tile(np.array([-INF, INF], np.float32), (64, 1))])
    perm = r.permutation(allr.shape[0])
    got = occl(torch, gs, dev(torch, allr[perm]), dev(torch, allt[perm]))
    back = np.empty_like(got)
    back[perm] = got
    np.testing.assert_array_equal(back[:1024], base[pick], err_msg="the ordinary rays beside the void ones")
    assert 0 < int(back[:1024].sum()) < 1024
    assert (back[1024:] == 0).all(), np.flatnonzero(back[1024:])
    want = R.walk(sc, allr, allt, mode="any")["occluded"].astype(np.uint8)
    np.testing.assert_array_equal(back, want)


# ------------------------------------------------------------------ 7. beside render launches
def test_occlusion_beside_render_launches(scenes, golden):
    """Four 1920x1080x4 frames of scene 8 on one stream and four occlusion calls of the same scene on two others,
    interleaved without a host wait, calls 2 and 3 sorted (they share the scene's sort scratch): every frame has the
    golden SHA, every call the bytes of the separate call."""
    import hashlib

    import torch
    hs, gs, sc = scenes({"scene": "scene8"})
    d_rays = gs.primary_rays(gs.frame(192, 108, 4))
    torch.cuda.synchronize()
    n = d_rays.shape[0]
    h = closest(torch, gs, d_rays)
    d_tmm = dev(torch, mixed_intervals(h[:, 1].view(np.float32), h[:, 0] != NOTRI, sc.diagonal()))
    quiet = occl(torch, gs, d_rays, d_tmm)
    assert 0 < int(quiet.sum()) < n
    W, H, spp = 1920, 1080, 4
    f = gs.frame(W, H, spp)
    s_frame, s_a, s_b = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    outs = [torch.full((W * H,), S.SENTINEL, dtype=torch.int32, device="cuda") for _ in range(4)]
    occ = [torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda") for _ in range(4)]
    L = rtm.tracer_lib()
    torch.cuda.synchronize()
    for i in range(4):
        gs.render_frame_device(f, outs[i].data_ptr(), s_frame.cuda_stream)
        flags, st = (rtm.RT_RAYS_SORT if i & 2 else 0), (s_b if i & 1 else s_a)
        assert L.rt_occluded_rays_device(gs._h, vp(d_rays), vp(d_tmm), n, flags, vp(occ[i]), ctypes.c_void_p(st.cuda_stream)) == 0
    torch.cuda.synchronize()
    for i in range(4):
        sha = hashlib.sha256(outs[i].cpu().numpy().view(np.uint32).tobytes()).hexdigest()
        assert sha == golden["frames_1080p4"]["8"]["bgra_sha256"], i
        o = occ[i].cpu().numpy()
        assert (o[n:] == FILL).all()
        np.testing.assert_array_equal(o[:n], quiet, err_msg=f"occlusion call beside frame {i}")


# ------------------------------------------------------------------ 8. rejected calls
def test_rejected_calls_write_nothing(inside_set):
    """RT_RAYS_COUNT, an unknown flag, NULL and misaligned pointers on a live scene: RT_E_INVALID, and neither the
    output nor a canary beside the inputs is touched."""
    import torch
    gs, sc, d_rays, rays, d_tmm, tmm, base = inside_set
    n = 256
    out = torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    L, st = rtm.tracer_lib(), ctypes.c_void_p(stream_of(torch))
    c = ctypes.c_void_p
    Rp, Tp, Op = d_rays.data_ptr(), d_tmm.data_ptr(), out.data_ptr()
    CNT, SORT = rtm.RT_RAYS_COUNT, rtm.RT_RAYS_SORT
    for args in ((c(Rp), c(Tp), n, CNT, c(Op)), (c(Rp), c(Tp), n, CNT | SORT, c(Op)), (c(Rp), c(Tp), n, 4, c(Op)),
                 (c(Rp), None, n, SORT | 64, c(Op)), (None, c(Tp), n, 0, c(Op)), (c(Rp), c(Tp), n, 0, None),
                 (c(Rp + 4), c(Tp), n, 0, c(Op)), (c(Rp), c(Tp + 4), n, 0, c(Op)), (c(Rp), c(Tp + 4), n, SORT, c(Op)),
                 (c(Rp), c(Tp), 0x80000000, 0, c(Op))):
        assert L.rt_occluded_rays_device(gs._h, *args, st) == 1, args
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all()
    np.testing.assert_array_equal(d_rays.cpu().numpy().view(np.uint32), rays.view(np.uint32))
    np.testing.assert_array_equal(d_tmm.cpu().numpy().view(np.uint32), tmm.view(np.uint32))
    # an odd output address is fine: bytes have no alignment
    got = torch.full((n + TAIL + 1,), FILL, dtype=torch.uint8, device="cuda")
    assert L.rt_occluded_rays_device(gs._h, c(Rp), c(Tp), n, 0, c(got.data_ptr() + 1), st) == 0
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    assert g[0] == FILL and (g[n + 1:] == FILL).all()
    np.testing.assert_array_equal(g[1:n + 1], base[:n])
