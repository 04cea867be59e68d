"""The reference of rt_march_rays_device (GpuScene.march): the contract's loop of include/rt_tracer.h in numpy float32,
every operation one rounding, over tests/distance_ref.py's DistanceBruteForce (the oracle's DistancePointTri for every
(position, triangle) pair, the reference's loop, the lowest-index rule).

    t = 0
    for s in range(max_steps):
        pos  = o + t * d                      the product rounded, then the sum
        dist, tri = distance_ref.reference(pos)
        t    = t + dist
        if dist < min_dist: HIT at step s + 1 (t after the add, the last dist, its tri)
    MISS: t = 0, dist = 0, tri = 0xFFFFFFFF, steps = 0

No ray is excluded from any comparison: the loop is defined for every float.  `stop_condition` restates the default
arm's receding-miss stop (csrc/rt_march.hip) so that its proof can be tested against the loop above.
"""
import numpy as np

import distance_ref as D

NOTRI = D.NOTRI
FLT_MAX = D.FLT_MAX
FLT_MIN = np.finfo(np.float32).tiny
# rt_march_hit (the package's MARCH_HIT_DTYPE)
HIT_DTYPE = np.dtype([("t", "<f4"), ("dist", "<f4"), ("tri", "<u4"), ("steps", "<u4")])
f32 = np.float32


def positions(o, d, t):
    """pos = o + t * d per component, the product rounded, then the sum."""
    with np.errstate(all="ignore"):
        return (o + (t[:, None] * d).astype(f32)).astype(f32)


def march(oracle, rays, tris, max_steps=128, min_dist=1e-3, trace=None):
    """rays f32 [n, 6], tris f32 [nt, 3, 3] -> HIT_DTYPE records [n] in the contract's layout (hit is steps != 0).
    trace: a list that receives (the marching rays' indices, their positions) of every step."""
    rays = np.ascontiguousarray(rays, f32)
    n = rays.shape[0]
    o, d = rays[:, :3], rays[:, 3:]
    md = f32(min_dist)
    t = np.zeros(n, f32)
    out = np.zeros(n, HIT_DTYPE)
    out["tri"] = NOTRI
    idx = np.arange(n)
    for s in range(max_steps):
        if idx.size == 0:
            break
        pos = positions(o[idx], d[idx], t[idx])
        if trace is not None:
            trace.append((idx.copy(), pos))
        dist, tri = D.reference(oracle, pos, tris)
        with np.errstate(all="ignore"):
            t[idx] = (t[idx] + dist).astype(f32)
            h = dist < md
        done = idx[h]
        out["t"][done], out["dist"][done], out["tri"][done], out["steps"][done] = t[done], dist[h], tri[h], s + 1
        idx = idx[~h]
    return out


def frame_pixels(rec, W, H, spp):
    """The reference's march frame from march records (renderer.cpp:88-133): a hit is shaded t / 3, a miss
    float(y) / float(H); the samples summed in order, averaged, gamma 2 and ToBGRA8."""
    y = np.repeat(np.arange(H), W * spp).astype(f32)
    with np.errstate(all="ignore"):
        col = np.where(rec["steps"] != 0, rec["t"] / f32(3.0), y / f32(H)).astype(f32).reshape(H * W, spp)
        total = np.zeros(H * W, f32)
        for k in range(spp):
            total = total + col[:, k]
        g = np.sqrt(total / f32(spp))
        ch = np.where(g > f32(1.0), 255, np.trunc(g * f32(255.0))).astype(np.uint32) & 255
    return (ch << 16) | (ch << 8) | ch


def vertex_box(tris):
    """(vmin f32 [3], vmax f32 [3], scene_scale f32) of a mesh whose every vertex is a triangle corner."""
    v = np.ascontiguousarray(tris, f32).reshape(-1, 3)
    return v.min(0), v.max(0), f32(np.abs(v).max())


def stop_condition(o, d, pos, vmin, vmax, scale, min_dist):
    """The receding-miss stop of k_march_rays at a step's position, csrc/rt_march.hip's float operations in their
    order -> bool [n]."""
    o, d, pos = (np.ascontiguousarray(x, f32) for x in (o, d, pos))
    md = f32(min_dist)
    with np.errstate(all="ignore"):
        pmax = np.fmax(np.fmax(np.abs(pos[:, 0]), np.abs(pos[:, 1])), np.abs(pos[:, 2]))
        margin = f32(1e-5) * (pmax + f32(scale))
        w = pos - np.fmin(np.fmax(pos, vmin[None, :]), vmax[None, :])
        db = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        rate = (d[:, 0] * w[:, 0] + d[:, 1] * w[:, 1]) + d[:, 2] * w[:, 2]
        thr = (f32(2e-5) * ((np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2]))) * db
        omax = np.fmax(np.fmax(np.abs(o[:, 0]), np.abs(o[:, 1])), np.abs(o[:, 2]))
        err = f32(2.5e-7) * (omax + f32(2.0) * pmax)
        return ((db > f32(1.00001) * ((margin + md) + err)) & (db <= FLT_MAX) & (rate >= thr) & (rate <= FLT_MAX) &
                (thr >= FLT_MIN))


def frame_stop_condition(d, pos, vmin, vmax, scale):
    """The receding-miss stop of the FRAME march (ray_march's culled arm, csrc/rt_frame_isect.h) at a step's position, its
    float operations in their order -> bool [n].  Unlike the query's (stop_condition) it has neither the |dir|_1 factor
    nor the E term: min_dist is 0.001, the rate threshold 2e-5 db whatever the direction's length.

        margin = 1e-5 (|p|_inf + scene_scale)
        w      = p - clamp(p, smin, smax)
        db     = sqrtf(wx wx + wy wy + wz wz)       every product and sum one rounding, summed left to right
        rate   = dx wx + dy wy + dz wz
        fire iff db > 1.00001 (margin + 0.001) && rate >= 2e-5 db"""
    d, pos = (np.ascontiguousarray(x, f32) for x in (d, pos))
    with np.errstate(all="ignore"):
        pmax = np.fmax(np.fmax(np.abs(pos[:, 0]), np.abs(pos[:, 1])), np.abs(pos[:, 2]))
        margin = f32(1e-5) * (pmax + f32(scale))
        w = pos - np.fmin(np.fmax(pos, np.asarray(vmin, f32)[None, :]), np.asarray(vmax, f32)[None, :])
        db = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        rate = (d[:, 0] * w[:, 0] + d[:, 1] * w[:, 1]) + d[:, 2] * w[:, 2]
        return (db > f32(1.00001) * (margin + f32(0.001))) & (rate >= f32(2e-5) * db)


def idle_share(steps, max_steps, wave=64):
    """Share of lane-steps idle in waves of `wave` consecutive rays when every ray marches to its hit and a miss to
    max_steps (the arm without the early stop): 1 - sum(lane steps) / (wave x sum(the wave's longest lane))."""
    s = np.where(np.asarray(steps) == 0, max_steps, np.asarray(steps)).astype(np.int64)
    pad = (-s.size) % wave
    lanes = np.concatenate([s, np.zeros(pad, np.int64)]).reshape(-1, wave)
    return 1.0 - float(s.sum()) / float((lanes.max(1) * wave).sum())
