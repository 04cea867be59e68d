"""A numpy float32 restatement of what rt_render_ao_device does between its walks (include/rt_tracer.h, steps 3-8 of
the contract): one numpy operation per contract operation, nothing fused (two ufunc calls cannot contract into an
FMA), the tables read from the library.  Shared by tests/test_ao_cpu.py, which checks its invariants and known
answers with tests/occlusion_ref.py's walks, and tests/test_gpu_ao.py, which holds the kernel to the composition
primary_rays -> trace_rays -> form() -> occluded -> counts() -> pixels(), byte for byte.  A plain module, numpy only.

Samples are in (y, x, sample) order, i = (y * W + x) * spp + s, as rt_primary_rays_device writes its rays.
"""
import numpy as np

F = np.float32
NOTRI = 0xFFFFFFFF
MISS = 0xFF                     # the count byte of a sample whose camera ray hits nothing


def sample_coords(W, H, spp):
    """(y, x, s) of every sample, flat, in (y, x, sample) order."""
    y, x, s = np.meshgrid(np.arange(H), np.arange(W), np.arange(spp), indexing="ij")
    return y.reshape(-1), x.reshape(-1), s.reshape(-1)


def rotation_index(x, y, s):
    """Step 5: j = ((x & 3) | ((y & 3) << 2)) ^ (sample & 15)."""
    return ((x & 3) | ((y & 3) << 2)) ^ (s & 15)


def dot3(a, b):
    """(a.x*b.x + a.y*b.y) + a.z*b.z on [m, 3] arrays."""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def normal_and_point(sc, rays, tri, t):
    """Step 4 for hit samples: rays [m, 6], tri [m] (triangle ids), t [m] -> (n [m, 3], p [m, 3]).
    sc: occlusion_ref.RefScene (v0, v1, v2 per triangle)."""
    with np.errstate(all="ignore"):
        o, d = rays[:, :3], rays[:, 3:]
        e1, e2 = sc.v1[tri] - sc.v0[tri], sc.v2[tri] - sc.v0[tri]
        g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                      e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(F)
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F)
        n = (g / ln[:, None]).astype(F)
        flip = dot3(n, d) > F(0)                   # false for a NaN n
        n = np.where(flip[:, None], -n, n).astype(F)
        p = (o + t[:, None] * d).astype(F)
    return n, p


def tangent_frame(n):
    """Step 4's frame of n [m, 3] (Duff et al. 2017) -> (T1, T2), each [m, 3]."""
    with np.errstate(all="ignore"):
        nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
        sg = np.copysign(F(1), nz).astype(F)
        a = (F(-1) / (sg + nz)).astype(F)
        b = ((nx * ny) * a).astype(F)
        t1 = np.stack([F(1) + (sg * (nx * nx)) * a, sg * b, -(sg * nx)], axis=1).astype(F)
        t2 = np.stack([b, sg + (ny * ny) * a, -ny], axis=1).astype(F)
    return t1, t2


def form(sc, rays, tri, t, dirs, rot, W, H, spp):
    """Steps 4-5 for a whole frame.  rays [n, 6] (rt_primary_rays_device's), tri u32 [n] and t f32 [n]
    (rt_trace_rays_device's; tri 0xFFFFFFFF = a miss), dirs f32 [K, 3] (the local directions: ao_table(K) or the
    caller's), rot: ao_rotations() f32 [16, 2] for RT_AO_ROTATE, None without.
    Returns a dict: hit (bool [n]), idx (the hit samples), n, p, t1, t2 ([m, 3] per hit sample), w ([m, K, 3]),
    ao_rays ([m * K, 6]: the AO rays (p, w), direction k of hit sample i at row i * K + k)."""
    rays = np.ascontiguousarray(rays, F)
    dirs = np.ascontiguousarray(dirs, F)
    K = dirs.shape[0]
    tri = np.asarray(tri).astype(np.int64)
    hit = tri != NOTRI
    idx = np.flatnonzero(hit)
    n, p = normal_and_point(sc, rays[idx], tri[idx], np.asarray(t, F)[idx])
    t1, t2 = tangent_frame(n)
    m = idx.size
    lx = np.broadcast_to(dirs[:, 0], (m, K)).astype(F)
    ly = np.broadcast_to(dirs[:, 1], (m, K)).astype(F)
    lz = np.broadcast_to(dirs[:, 2], (m, K)).astype(F)
    with np.errstate(all="ignore"):
        if rot is not None:
            y, x, s = sample_coords(W, H, spp)
            j = rotation_index(x, y, s)[idx]
            c, sn = np.asarray(rot, F)[j, 0][:, None], np.asarray(rot, F)[j, 1][:, None]
            lx, ly = (c * lx - sn * ly).astype(F), (sn * lx + c * ly).astype(F)
        w = np.empty((m, K, 3), F)
        for a in range(3):
            w[:, :, a] = (lx * t1[:, a:a + 1] + ly * t2[:, a:a + 1]) + lz * n[:, a:a + 1]
    ao = np.empty((m, K, 6), F)
    ao[:, :, :3] = p[:, None, :]
    ao[:, :, 3:] = w
    return {"hit": hit, "idx": idx, "n": n, "p": p, "t1": t1, "t2": t2, "w": w,
            "ao_rays": np.ascontiguousarray(ao.reshape(m * K, 6))}


def counts(occluded, hit, K):
    """Step 7's count per sample: occluded [m * K] (bytes or bools, form()'s ao_rays order) -> u8 [n], MISS where the
    camera ray hit nothing."""
    out = np.full(hit.shape[0], MISS, np.uint8)
    out[hit] = np.asarray(occluded).astype(np.uint8).reshape(-1, K).sum(1, dtype=np.uint32).astype(np.uint8)
    return out


def pixels(cnt, K, W, H, spp):
    """Steps 3, 7, 8: counts u8 [n] -> packed pixels u32 [H, W] (colour, the sum in sample order, average, gamma,
    ToBGRA8 -- renderer.cpp:121-133 with the correctly rounded square root, as the render kernels)."""
    cnt = np.asarray(cnt, np.uint8).reshape(H, W, spp)
    y = np.broadcast_to(np.arange(H, dtype=np.int64)[:, None, None], cnt.shape)
    miss = cnt == MISS
    with np.errstate(all="ignore"):
        open_share = (F(K) - cnt.astype(F)).astype(F) / F(K)        # float(K - c) / float(K): K - c is exact
        col = np.where(miss, y.astype(F) / F(H), open_share).astype(F)
        total = col[:, :, 0].copy()
        for s in range(1, spp):
            total = (total + col[:, :, s]).astype(F)
        g = np.sqrt((total * F(1.0 / spp)).astype(F)).astype(F)     # spp is a power of two: the average is exact
        ch = np.where(g > F(1), 255, np.trunc((g * F(255)).astype(F)).astype(np.int64) & 255).astype(np.uint32)
    return (ch << 16 | ch << 8 | ch).astype(np.uint32)


def render(sc, walk, rays, dirs, rot, tmin, tmax, W, H, spp):
    """The whole contract on the host: walk = occlusion_ref.walk.  -> (counts u8 [H, W, spp], pixels u32 [H, W], the
    form() dict with "occluded" added)."""
    res = walk(sc, rays, mode="closest")
    tri = np.where(res["hit"], res["tri"], np.uint32(NOTRI))
    f = form(sc, rays, tri, res["t"], dirs, rot, W, H, spp)
    m = f["ao_rays"].shape[0]
    tmm = np.tile(np.array([tmin, tmax], F), (m, 1))
    f["occluded"] = walk(sc, f["ao_rays"], tmm, mode="any")["occluded"] if m else np.zeros(0, bool)
    K = np.asarray(dirs).shape[0]
    cnt = counts(f["occluded"], f["hit"], K)
    return cnt.reshape(H, W, spp), pixels(cnt, K, W, H, spp), f
