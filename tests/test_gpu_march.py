"""rt_march_rays_device (GpuScene.march) on the GPU, bit for bit: against the reference's own RayMarch (the golden march
crops and frames of scenes 1, 2 and 3, and the frame path's records), against tests/march_ref.py (the contract's
loop over the oracle's DistancePointTri for every pair) on meshes at the hierarchy's edges and on a wave whose lanes
disagree, and against the composition a caller had before (a loop of GpuScene.distance calls with torch arithmetic)
where the all-pairs reference is too slow.  No ray is excluded from any comparison.

Every call goes through the C ABI into a buffer pre-filled with a sentinel that carries 64 records past n, which must
still hold the sentinel afterwards; every case runs the default arm, RT_MARCH_SORT, RT_MARCH_EXHAUSTIVE and both
flags, and all four must give the same bytes.
"""
import ctypes

import numpy as np
import pytest

import distance_ref as D
import march_ref as M
import synth_scenes as S
from conftest import ALT_REC_DTYPE, load_package, read_gz

pytestmark = pytest.mark.gpu
rtm = load_package()
NOTRI = M.NOTRI
TAIL = 64
SENT = 0x5A5A5A5A
F = np.float32
ARMS = {"default": 0, "sort": rtm.RT_MARCH_SORT, "exhaustive": rtm.RT_MARCH_EXHAUSTIVE,
        "sort|exhaustive": rtm.RT_MARCH_SORT | rtm.RT_MARCH_EXHAUSTIVE}


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def raw_march(torch, gs, d_rays, n=None, flags=0, params=None, expect_rc=0, stream=None):
    """One rt_march_rays_device call into a sentinel-filled buffer with a 64-record tail -> records MARCH_HIT_DTYPE
    [n]; nothing may be written past n (nor at all by a rejected call)."""
    n = d_rays.shape[0] if n is None else n
    out = torch.full((n + TAIL, 4), SENT, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    p = ctypes.byref(rtm.MarchParams(*params)) if params is not None else None
    rc = rtm.tracer_lib().rt_march_rays_device(gs._h, vp(d_rays), n, p, flags, vp(out), ctypes.c_void_p(st))
    assert rc == expect_rc, (rc, expect_rc)
    torch.cuda.synchronize()
    written = n if rc == 0 else 0
    h = out.cpu().numpy().view(np.uint32)
    assert (h[written:] == SENT).all(), "records written past n"
    return h[:written].copy().view(rtm.MARCH_HIT_DTYPE).reshape(written)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def same_records(got, want, what, rays=None):
    for k in ("steps", "t", "dist", "tri"):
        bad = np.flatnonzero(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert bad.size == 0, (what, k, bad[:8], None if rays is None else rays[bad[:8]], got[bad[:8]], want[bad[:8]])


# The exhaustive arm takes a wave through every triangle at every step, however few rays there are: on the killeroo
# (24,336 triangles) that is about a second per 128-step call, so its cases there run the four arms at KILLEROO_STEPS
# and the two culled arms at full length against the composition.
CULLED = ("default", "sort")
KILLEROO_STEPS = 12
COMPOSE_STEPS = 96          # (a miss of the composition marches on far from the mesh, where nothing is culled)


def all_arms(torch, gs, rays, what, params=None, arms=tuple(ARMS)):
    """The arms on one ray set: the same bytes; a miss is exactly (0, 0, NOTRI, 0).  -> the default arm's."""
    d_rays = rays if isinstance(rays, torch.Tensor) else dev(torch, rays)
    host = d_rays.cpu().numpy()
    recs = {arm: raw_march(torch, gs, d_rays, flags=ARMS[arm], params=params) for arm in arms}
    for arm in arms[1:]:
        same_records(recs[arm], recs["default"], f"{what} [{arm} against default]", host)
    r = recs["default"]
    miss = r[r["steps"] == 0]
    assert (miss.view(np.uint32).reshape(-1, 4) == np.array([0, 0, NOTRI, 0], np.uint32)).all(), what
    assert not np.isnan(r["dist"]).any()
    return r


@pytest.fixture(scope="module")
def scenes():
    """Per key: (HostScene, GpuScene, triangle corners f32 [nt, 3, 3]), made once.  A key is a shipped scene's number
    or a (name, mesh) pair built with HostScene.from_mesh on a coarse grid."""
    cache = {}

    def get(key, tris=None):
        if key not in cache:
            if tris is None:
                hs = rtm.HostScene.load(key)
            else:
                v, t = S.mesh_of(tris)
                hs = rtm.HostScene.from_mesh(v, t, 45.0, S.axis_cam(2, -1, (0.0, 0.0, 3.0)), grid_res=8)
            v, t = hs.mesh()
            cache[key] = (hs, rtm.GpuScene(hs, 0), D.triangles_of(v, t))
        return cache[key]
    yield get
    for hs, gs, _ in cache.values():
        gs.close()
        hs.close()


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(1))[:, None]


def ray_mix(tris, n, seed):
    """n rays around a mesh, f32 [n, 6]: from outside at points of the surface (hits), from inside in random
    directions, from near the surface along it, and away from the mesh (misses); lengths 0.25 .. 1."""
    r = np.random.Generator(np.random.PCG64(seed))
    v = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    mid, diag = 0.5 * (lo + hi), float(np.sqrt(((hi - lo) ** 2).sum())) or 1.0
    pick = tris[r.integers(0, tris.shape[0], n)].astype(np.float64)
    on = (pick * r.dirichlet((1.0, 1.0, 1.0), n)[:, :, None]).sum(1)
    out = mid + 1.5 * diag * unit(r.normal(size=(n, 3)))
    kind = np.arange(n) % 4
    o = np.where((kind == 0)[:, None], out, np.where((kind == 1)[:, None], r.uniform(lo, hi, (n, 3)),
                 np.where((kind == 2)[:, None], on + 0.01 * diag * r.normal(size=(n, 3)), out)))
    d = np.where((kind == 0)[:, None], unit(on - out), np.where((kind == 3)[:, None], unit(out - mid + 0.3 * diag * r.normal(size=(n, 3))),
                 unit(r.normal(size=(n, 3)))))
    d = d * r.choice([0.25, 0.5, 1.0], n)[:, None]
    return np.ascontiguousarray(np.concatenate([o, d], 1), np.float32)


def compose(torch, gs, d_rays, max_steps=128, min_dist=1e-3):
    """What a caller had before: the contract's loop as GpuScene.distance calls with torch float32 arithmetic between
    them, one torch operation per rounding, on the rays still marching -> MARCH_HIT_DTYPE records."""
    n = d_rays.shape[0]
    o, d = d_rays[:, :3].contiguous(), d_rays[:, 3:].contiguous()
    t = torch.zeros(n, dtype=torch.float32, device="cuda")
    out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    out[:, 2] = -1
    idx = torch.arange(n, device="cuda")
    md = torch.tensor(min_dist, dtype=torch.float32, device="cuda")
    for s in range(max_steps):
        if idx.numel() == 0:
            break
        prod = t[idx, None] * d[idx]
        pos = (o[idx] + prod).contiguous()
        res = gs.distance(pos)
        tn = t[idx] + res.dist
        t[idx] = tn
        h = res.dist < md
        done = idx[h]
        out[done, 0] = tn[h].view(torch.int32)
        out[done, 1] = res.dist[h].view(torch.int32)
        out[done, 2] = res.raw[h, 1]
        out[done, 3] = s + 1
        idx = idx[~h]
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).copy().view(rtm.MARCH_HIT_DTYPE).reshape(n)


# ------------------------------------------------------------------ the reference's own march
CROPS = ["march_scene1_952_532_8x8", "march_scene2_952_532_8x8", "march_scene3_952_532_8x8",
         "march_scene1_1500_300_8x4", "march_scene3_1500_300_8x4"]
FRAMES = ["march_scene1_48x27x1", "march_scene2_48x27x1", "march_scene3_48x27x1", "march_scene1_64x48x4",
          "march_scene3_31x19x2"]


def check_against_frame_path(rec, got, what):
    """march records against rt_trace_samples records of RT_ISECT_RAY_MARCH: hit, t bits and steps (a miss there
    reports its 128 steps; its t is not part of either contract)."""
    hit = got["hit"] == 1
    np.testing.assert_array_equal(rec["steps"] != 0, hit, err_msg=what)
    np.testing.assert_array_equal(rec["t"][hit].view(np.uint32), got["t"][hit].view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(rec["steps"][hit], got["steps"][hit], err_msg=what)
    assert (got["steps"][~hit] == 128).all(), what


def test_golden_crops_and_the_frame_path(golden_alt, scenes):
    import torch
    for name in CROPS:
        c = next(x for x in golden_alt["crops"] if x["name"] == name)
        hs, gs, tris = scenes(c["scene"])
        f = gs.frame(c["W"], c["H"], c["spp"], intersector=rtm.RT_ISECT_RAY_MARCH)
        rays = gs.primary_rays(f).view(c["H"], c["W"], c["spp"], 6)
        crop = rays[c["y0"]:c["y0"] + c["h"], c["x0"]:c["x0"] + c["w"]].reshape(-1, 6).contiguous()
        del rays
        rec = all_arms(torch, gs, crop, name)
        exp = read_gz(f"alt/{name}.rec.gz", ALT_REC_DTYPE)
        hit = exp["hit"] == 1
        np.testing.assert_array_equal(rec["steps"] != 0, hit, err_msg=name)
        np.testing.assert_array_equal(rec["t"][hit].view(np.uint32), exp["t"][hit].view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(rec["steps"][hit], exp["steps"][hit], err_msg=name)
        check_against_frame_path(rec, gs.trace_samples(f, c["x0"], c["y0"], c["w"], c["h"]), name)
        assert (rec["tri"][hit] < tris.shape[0]).all() and (rec["dist"][hit] < F(1e-3)).all()


@pytest.mark.parametrize("name", FRAMES)
def test_golden_frames_and_the_frame_path(golden_alt, scenes, name):
    """The frames hold misses too: the golden pixels follow from the march records (march_ref.frame_pixels, which
    tests/test_march_cpu.py pins to these frames), and the frame path's records agree sample for sample."""
    import torch
    fr = next(x for x in golden_alt["frames"] if x["name"] == name)
    hs, gs, tris = scenes(fr["scene"])
    f = gs.frame(fr["W"], fr["H"], fr["spp"], intersector=rtm.RT_ISECT_RAY_MARCH)
    rec = all_arms(torch, gs, gs.primary_rays(f), name)
    pix = M.frame_pixels(rec, fr["W"], fr["H"], fr["spp"])
    np.testing.assert_array_equal(pix & 0xFFFFFF, read_gz(f"alt/{name}.bgra.gz", "<u4") & 0xFFFFFF, err_msg=name)
    check_against_frame_path(rec, gs.trace_samples(f, 0, 0, fr["W"], fr["H"]), name)
    assert 0 < (rec["steps"] != 0).sum()


# ------------------------------------------------------------------ march_ref at the structure's edges
@pytest.mark.parametrize("K", [3, 31, 32, 33, 64, 65, 1023, 1025, 32769])
def test_march_ref_at_hierarchy_edges(oracle, scenes, K):
    """synth_scenes.sparse(seed, n = K - 2) has K triangles: the small-mesh rule (64 / 65), one and two blocks, one and
    two upper levels.  Rays x triangles x steps sizes the all-pairs reference: 256 rays up to 65 triangles, 64 at
    about 1,024, 16 rays of at most 48 steps at 32,769."""
    import torch
    hs, gs, tris = scenes(("sparse", K), S.sparse(300 + K, n=K - 2))
    assert tris.shape[0] == K
    n, steps = (256, 128) if K <= 65 else (64, 128) if K <= 1025 else (16, 48)
    rays = ray_mix(tris, n, K)
    want = M.march(oracle, rays, tris, max_steps=steps)
    got = all_arms(torch, gs, rays, f"sparse K = {K}", params=(steps, 1e-3))
    same_records(got, want, f"sparse K = {K}", rays)
    hits = int((want["steps"] != 0).sum())
    assert 0 < hits < n, hits
    print(f"K = {K}: {hits} of {n} rays hit, steps {want['steps'][want['steps'] != 0].min()} .. {want['steps'].max()}")


def test_degenerate_mesh_and_duplicate_pairs(oracle, scenes):
    """synth_scenes.degenerate(28): collinear triangles, point triangles (NaN distances) and exact duplicates.  Rays at
    the duplicated triangles' centroids, at vertices and at random: tri is never the higher index of a pair."""
    import torch
    mesh = S.degenerate(28)
    hs, gs, tris = scenes(("degenerate", 28), mesh)
    np.testing.assert_array_equal(tris, mesh)
    dup_hi = np.array([40 + 3 * m + 2 for m in range(8)])
    dup_lo = np.array([3 * m for m in range(8)])
    np.testing.assert_array_equal(tris[dup_hi], tris[dup_lo])
    r = np.random.Generator(np.random.PCG64(5))
    cents = (tris[dup_lo].astype(np.float64).sum(1) / 3.0)
    tgt = np.concatenate([np.repeat(cents, 8, 0), tris.reshape(-1, 3)[::5].astype(np.float64)])
    o = tgt + 0.4 * unit(r.normal(size=tgt.shape))
    rays = np.concatenate([np.concatenate([o, unit(tgt - o)], 1).astype(np.float32), ray_mix(tris, 64, 6)])
    want = M.march(oracle, rays, tris)
    got = all_arms(torch, gs, rays, "degenerate")
    same_records(got, want, "degenerate", rays)
    assert not np.isin(got["tri"], dup_hi).any()
    assert np.isin(got["tri"], dup_lo).sum() >= 8                 # the pairs are reached


# ------------------------------------------------------------------ a wave whose lanes disagree
def disagreeing_wave(tris, seed):
    """64 rays for one wave: origins on the surface (a hit at step 1), late hits, misses that march every step (a zero
    direction off the surface), misses that recede (stopped early), NaN / +-inf / +-3e38 / denormal components, and
    origins at +-1e19."""
    r = np.random.Generator(np.random.PCG64(seed))
    base = ray_mix(tris, 64, seed + 1)
    rays = base.copy()
    on = (tris[r.integers(0, tris.shape[0], 8)] * F(1.0 / 3.0)).sum(1)
    rays[0:8, :3] = on                                            # on the surface: step 1
    rays[8:12, 3:] = 0.0                                          # marching on the spot
    rays[12:16, 3:] *= F(2.0 ** -7)                               # crawling: a late hit or a full-length miss
    k = 16
    for v in (np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-40, -1e-40, 1.4e-45):
        rays[k, r.integers(0, 3)] = v                             # in the origin
        rays[k + 1, 3 + r.integers(0, 3)] = v                     # in the direction
        k += 2
    rays[32, :3] = 1e19
    rays[33, :3] = -1e19
    rays[34, 0] = 1e19
    rays[34, 3:] = (-1.0, 0.0, 0.0)                               # from 1e19 towards the mesh
    rays[35] = (np.nan,) * 6
    rays[36, 3:] = np.inf
    rays[37, 3:] = 3e38
    return np.ascontiguousarray(rays, np.float32)


STEPS = [1, 2, 128, 129, 1000]
MIN_DISTS = [0.0, -1.0, 1e-6, 1e-3, 1.0, float("inf")]


def test_a_wave_whose_lanes_disagree(oracle, scenes):
    """One reference run of 1,000 steps per min_dist gives every max_steps: a ray that hits at step s is a hit
    exactly when s <= max_steps.  65 triangles (three blocks: the culled arm) keep the all-pairs reference affordable."""
    import torch
    hs, gs, tris = scenes(("sparse", 65), S.sparse(300 + 65, n=63))
    rays = disagreeing_wave(tris, 3)
    d_rays = dev(torch, rays)
    seen = set()
    for md in MIN_DISTS:
        full = M.march(oracle, rays, tris, max_steps=1000, min_dist=md)
        for steps in STEPS:
            want = full.copy()
            late = want["steps"] > steps
            want["t"][late], want["dist"][late], want["tri"][late], want["steps"][late] = 0, 0, NOTRI, 0
            got = all_arms(torch, gs, d_rays, f"wave {steps} {md}", params=(steps, md))
            same_records(got, want, f"max_steps {steps}, min_dist {md}", rays)
            seen.update(np.unique(got["steps"]).tolist())
        if md == float("inf"):
            assert (full["steps"] == 1).all()
        if md <= 0.0:
            assert (full["steps"] == 0).all()
    assert {0, 1}.issubset(seen) and len(seen) > 3, sorted(seen)


def test_the_wave_on_larger_meshes(scenes):
    """The same 64 rays on two levels (1,025 triangles) and on the killeroo: the default arm against the exhaustive,
    and on the killeroo against the composition too.  (A non-finite position culls nothing, so these rays cost the
    default arm what they cost the exhaustive one: KILLEROO_STEPS there.)"""
    import torch
    for key, mesh, cases in ((("sparse", 1025), S.sparse(300 + 1025, n=1023), ((128, 1e-3), (300, 1e-6), (2, 1.0))),
                             (8, None, ((KILLEROO_STEPS, 1e-3), (2, 1.0)))):
        hs, gs, tris = scenes(key, mesh)
        rays = disagreeing_wave(tris, 4)
        d_rays = dev(torch, rays)
        for params in cases:
            r = all_arms(torch, gs, d_rays, f"{key} {params}", params=params)
            assert (r["steps"][:8] == 1).all()                    # the origins on the surface
            if key == 8:
                same_records(r, compose(torch, gs, d_rays, *params), f"killeroo {params} against the composition", rays)


# ------------------------------------------------------------------ composition on the killeroo
def test_composition_on_the_killeroo(scenes):
    """4,097 rays in camera order, shuffled, and one bounce off the primary hits: a loop of GpuScene.distance calls
    with torch arithmetic gives the same records.  24,336 triangles: the case the all-pairs reference cannot afford."""
    import torch
    hs, gs, tris = scenes(8)
    f = gs.frame(96, 54, 1)
    cam = gs.primary_rays(f)[540:540 + 4097].contiguous()
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(41)).permutation(4097)).cuda()
    h = gs.trace_rays(cam)
    hit = h.hits[:, 0] != -1
    assert 500 < int(hit.sum()) < 4097
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    p = cam[:, :3] + cam[:, 3:] * h.t[:, None]
    p = torch.where(hit[:, None], p, cam[:, :3])
    w = torch.randn((4097, 3), generator=g, device="cuda")
    bounce = torch.cat([p - cam[:, 3:] * 0.01, w / w.norm(dim=1, keepdim=True)], 1).contiguous()
    for what, rays in (("camera order", cam), ("shuffled", cam[perm].contiguous()), ("bounce", bounce)):
        want = compose(torch, gs, rays, COMPOSE_STEPS)
        got = all_arms(torch, gs, rays, what, params=(COMPOSE_STEPS, 1e-3), arms=CULLED)
        same_records(got, want, what, rays.cpu().numpy())
        short = all_arms(torch, gs, rays, what, params=(KILLEROO_STEPS, 1e-3))
        late = want["steps"] > KILLEROO_STEPS
        want["t"][late], want["dist"][late], want["tri"][late], want["steps"][late] = 0, 0, NOTRI, 0
        same_records(short, want, f"{what}, {KILLEROO_STEPS} steps", rays.cpu().numpy())
        hits = int((got["steps"] != 0).sum())
        assert 0 < hits < 4097, (what, hits)
        print(f"{what}: {hits} of 4097 rays hit, steps up to {got['steps'].max()}, "
              f"idle share without the stop {M.idle_share(got['steps'], COMPOSE_STEPS):.3f}")


# ------------------------------------------------------------------ direction scales
def test_direction_scales_default_equals_exhaustive(scenes):
    """One ray set at direction scales 2^-10 ... 2^10 on two meshes: every record of the default arm (the cull and
    the receding-miss stop, whose rate condition scales with the direction) equals the exhaustive arm's -- on the
    killeroo at KILLEROO_STEPS, and at full length the composition's, which has no early stop either."""
    import torch
    for key, mesh in ((("sparse", 1025), S.sparse(300 + 1025, n=1023)), (8, None)):
        hs, gs, tris = scenes(key, mesh)
        base = ray_mix(tris, 96, 17)
        base[:, 3:] = unit(base[:, 3:]).astype(np.float32)
        sc = (2.0 ** np.arange(-10, 11)).astype(np.float32)
        rays = np.repeat(base, sc.size, 0)
        rays[:, 3:] *= np.tile(sc, base.shape[0])[:, None]
        d_rays = dev(torch, rays)
        if key == 8:
            all_arms(torch, gs, d_rays, "scales killeroo, short", params=(KILLEROO_STEPS, 1e-3))
            r = all_arms(torch, gs, d_rays, "scales killeroo", arms=CULLED)
            same_records(r, compose(torch, gs, d_rays), "scales killeroo against the composition", rays)
        else:
            r = all_arms(torch, gs, d_rays, f"scales {key}")
        by_scale = (r["steps"] != 0).reshape(base.shape[0], sc.size)
        assert by_scale.any() and not by_scale.all()


# ------------------------------------------------------------------ mechanics
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_ray_counts_and_canaries(oracle, scenes, n):
    import torch
    hs, gs, tris = scenes(("sparse", 1025), S.sparse(300 + 1025, n=1023))          # culled, two levels
    if n == 0:
        d_rays = torch.zeros((1, 6), dtype=torch.float32, device="cuda")
        for flags in ARMS.values():
            assert raw_march(torch, gs, d_rays, n=0, flags=flags).size == 0
        res = gs.march(np.zeros((0, 6), np.float32))
        assert res.hit.shape == (0,) and res.t.shape == (0,) and res.raw.shape == (0,)
        return
    rays = ray_mix(tris, 4100, 9)[np.random.Generator(np.random.PCG64(n)).permutation(4100)[:n]]
    d_rays = dev(torch, rays)
    got = all_arms(torch, gs, d_rays, f"n = {n}")
    same_records(got, compose(torch, gs, d_rays), f"n = {n} against the composition", rays)
    m = min(n, 24)
    same_records(got[:m], M.march(oracle, rays[:m], tris), f"n = {n} against march_ref", rays[:m])


def test_c_abi_argument_errors_write_nothing(scenes):
    import torch
    hs, gs, tris = scenes(1)
    L = rtm.tracer_lib()
    d_rays = torch.zeros((8, 6), dtype=torch.float32, device="cuda")
    for flags in (4, 0x10, 0x80000000, 1 | 2 | 4):
        raw_march(torch, gs, d_rays, flags=flags, expect_rc=1)
    for params in ((0, 1e-3), (4097, 1e-3), (0xFFFFFFFF, 1e-3), (128, float("nan"))):
        raw_march(torch, gs, d_rays, params=params, expect_rc=1)
    out = torch.full((16, 4), SENT, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, o = d_rays.data_ptr(), out.data_ptr()

    def call(scene, pp, n, oo):
        return L.rt_march_rays_device(scene, ctypes.c_void_p(pp), n, None, 0, ctypes.c_void_p(oo), st)

    assert call(None, p, 8, o) == 1                            # a NULL scene, d_rays, d_out
    assert call(gs._h, None, 8, o) == 1
    assert call(gs._h, p, 8, None) == 1
    assert call(gs._h, p + 4, 4, o) == 1                       # d_rays, d_out off 8 bytes
    assert call(gs._h, p, 4, o + 4) == 1
    assert call(gs._h, p, 0x80000000, o) == 1                  # n >= 2^31
    assert call(gs._h, p, 0, None) == 0                        # n == 0: RT_OK, nothing looked at
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENT).all()


def test_python_layer(oracle, scenes):
    """numpy in -> numpy out, torch in -> torch out (in place), the flags and parameters, a caller's stream, and every
    refused input."""
    import torch
    hs, gs, tris = scenes(2)
    rays = ray_mix(tris, 40, 3)
    want = M.march(oracle, rays, tris)
    for kw in ({}, {"sort": True}, {"exhaustive": True}, {"sort": True, "exhaustive": True}):
        res = gs.march(rays, **kw)
        assert isinstance(res.t, np.ndarray) and res.raw.dtype == rtm.MARCH_HIT_DTYPE and res.hit.dtype == bool
        same_records(res.raw, want, f"numpy {kw}", rays)
        np.testing.assert_array_equal(res.hit, want["steps"] != 0)
        assert (res.t.view(np.uint32) == want["t"].view(np.uint32)).all() and (res.steps == want["steps"]).all()
        res = gs.march(dev(torch, rays), **kw)
        torch.cuda.synchronize()
        assert isinstance(res.t, torch.Tensor) and res.t.is_cuda and res.t.dtype == torch.float32
        assert tuple(res.raw.shape) == (40, 4) and res.hit.dtype == torch.bool
        same_records(res.raw.cpu().numpy().view(np.uint32).copy().view(rtm.MARCH_HIT_DTYPE).reshape(40), want, f"torch {kw}", rays)
        np.testing.assert_array_equal(res.hit.cpu().numpy(), want["steps"] != 0)
        np.testing.assert_array_equal(res.dist.cpu().numpy().view(np.uint32), want["dist"].view(np.uint32))
        np.testing.assert_array_equal(res.tri.cpu().numpy().view(np.uint32), want["tri"])
    res = gs.march(rays, max_steps=7, min_dist=0.05)
    same_records(res.raw, M.march(oracle, rays, tris, max_steps=7, min_dist=0.05), "parameters", rays)
    s = torch.cuda.Stream()
    d_rays = dev(torch, rays)
    torch.cuda.synchronize()
    res = gs.march(d_rays, stream=s.cuda_stream)
    s.synchronize()
    same_records(res.raw.cpu().numpy().view(np.uint32).copy().view(rtm.MARCH_HIT_DTYPE).reshape(40), want, "stream", rays)
    res = gs.march(rays, sort=True, stream=s.cuda_stream)
    same_records(res.raw, want, "numpy on a stream", rays)
    good = torch.zeros((6, 6), dtype=torch.float32, device="cuda")
    for bad in (good.double(), good.half(), good.reshape(-1), good[:, :5], torch.zeros((6, 7), device="cuda"),
                torch.zeros((6, 12), device="cuda")[:, :6], good[::2], good.cpu(), good.cpu().numpy().astype(np.float64),
                good.cpu().numpy()[::2], good.cpu().numpy().reshape(-1), [[0.0] * 6], None):
        with pytest.raises(ValueError):
            gs.march(bad)
    for kw in ({"max_steps": 0}, {"max_steps": 4097}, {"min_dist": float("nan")}):
        with pytest.raises(ValueError):
            gs.march(good, **kw)


def test_graph_capture_and_replay(oracle, scenes):
    """One warm-up call, the call (no RT_MARCH_SORT) captured in a graph, two replays into a cleared buffer: the same
    bytes each time."""
    import torch
    hs, gs, tris = scenes(("sparse", 1025), S.sparse(300 + 1025, n=1023))
    rays = ray_mix(tris, 130, 77)
    n = rays.shape[0]
    d_rays = dev(torch, rays)
    out = torch.full((n + TAIL, 4), SENT, dtype=torch.int32, device="cuda")
    L = rtm.tracer_lib()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert L.rt_march_rays_device(gs._h, vp(d_rays), n, None, 0, vp(out), ctypes.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    first = out.cpu().numpy().copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        assert L.rt_march_rays_device(gs._h, vp(d_rays), n, None, 0, vp(out), ctypes.c_void_p(s.cuda_stream)) == 0
    for _ in range(2):
        out.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), first)
    rec = first[:n].view(np.uint32).copy().view(rtm.MARCH_HIT_DTYPE).reshape(n)
    assert (first[n:].view(np.uint32) == SENT).all()
    same_records(rec[:32], M.march(oracle, rays[:32], tris), "graph", rays[:32])
    same_records(rec, compose(torch, gs, d_rays), "graph against the composition", rays)


def test_calls_interleaved_with_frames_and_sorted_queries(scenes):
    """Marches between render frames and between sorted distance / trace_rays calls, which share the sort scratch:
    every result is what it is alone."""
    import torch
    hs, gs, tris = scenes(8)
    f = gs.frame(160, 90, 2)
    before = gs.render_frame(f).copy()
    fm = gs.frame(64, 36, 1, intersector=rtm.RT_ISECT_RAY_MARCH)
    march_frame = gs.render_frame(fm).copy()
    rays = dev(torch, ray_mix(tris, 700, 1))
    pts = rays[:, :3].contiguous()
    alone = gs.march(rays).raw.clone()
    dist_alone = gs.distance(pts, sort=True).raw.clone()
    hits_alone = gs.trace_rays(rays, sort=True).hits.clone()
    torch.cuda.synchronize()
    short_alone = gs.march(rays, max_steps=8).raw.clone()
    for kw in ({}, {"sort": True}, {"exhaustive": True, "max_steps": 8}, {"sort": True}):
        d = gs.distance(pts[:300 if kw.get("sort") else 700].contiguous(), sort=True)
        m = gs.march(rays, **kw)
        h = gs.trace_rays(rays, sort=True)
        m2 = gs.march(rays[:65].contiguous(), sort=True)
        torch.cuda.synchronize()
        assert torch.equal(m.raw, short_alone if "max_steps" in kw else alone)
        assert torch.equal(m2.raw, alone[:65]) and torch.equal(h.hits, hits_alone)
        assert torch.equal(d.raw, dist_alone[:d.raw.shape[0]])
        np.testing.assert_array_equal(gs.render_frame(f), before)
    np.testing.assert_array_equal(gs.render_frame(fm), march_frame)
