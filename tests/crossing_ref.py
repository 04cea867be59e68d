"""A numpy float32 restatement of the walk rt_crossing_rays_device is defined by (include/rt_tracer.h), shared by
tests/test_crossing_cpu.py (which anchors it to the oracle's IntersectRayTri and to the occlusion restatement) and
tests/test_gpu_crossings.py (which holds the kernel to it, byte for byte).  A plain module, numpy only; the scene,
the triangle test, the box entry and the float -> int conversion are tests/occlusion_ref.py's, unedited.

The walk is occlusion_ref.walk's Grid::Intersect (grid.cpp:159-281) with these points:
  0. t_in = -inf before the first cell; count = front = 0;
  1. a test counts iff hit && t_in <= cur_t && cur_t < next_crossing_t[step_axis] && tmin < cur_t && cur_t < tmax;
  2. a counted test does count += 1, and front += 1 when det > 0 (triangle.h:48's f32 det); nothing ends the list
     or the walk;
  3. after the cell's list, before the advance: next_crossing_t[step_axis] >= tmax ends the walk; otherwise
     t_in = next_crossing_t[step_axis] (the value before += delta_t), then the reference's advance.
{0, 0} without a walk: a ray with a non-finite component, a NaN bound, !(tmin < tmax), a ray that misses the box.
"""
import numpy as np

from occlusion_ref import F, FLT_MAX, PAIRS_PER_SLICE, box_entry, cvt_i32, ray_tri


def tri_det(d, v0, v1, v2):
    """triangle.h:41-48: det = DOT(edge1, CROSS(dir, edge2)), the operations of occlusion_ref.ray_tri in its order
    (the same bits as the det ray_tri gates on)."""
    e1, e2 = v1 - v0, v2 - v0
    px = d[:, 1] * e2[:, 2] - d[:, 2] * e2[:, 1]
    py = d[:, 2] * e2[:, 0] - d[:, 0] * e2[:, 2]
    pz = d[:, 0] * e2[:, 1] - d[:, 1] * e2[:, 0]
    return (e1[:, 0] * px + e1[:, 1] * py) + e1[:, 2] * pz


def intervals_of(n, tminmax):
    if tminmax is None:
        return np.full(n, -np.inf, F), np.full(n, np.inf, F)
    tmm = np.ascontiguousarray(tminmax, F)
    return tmm[:, 0].copy(), tmm[:, 1].copy()


def walk_count(sc, rays, tminmax=None, pairs=False):
    """rays [n, 6] f32 (origin, direction as passed); tminmax [n, 2] f32 or None = (-inf, +inf).  Returns a dict of
    per-ray arrays count, front (u32) and crossings (bool [n]: the walk's crossing times never decreased); with
    pairs=True also pairs, an int64 [m, 2] array of the counted (ray, mesh triangle) tests in walk order."""
    rays = np.ascontiguousarray(rays, F)
    n = rays.shape[0]
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    tmin, tmax = intervals_of(n, tminmax)
    valid = np.isfinite(rays).all(1) & (tmin < tmax)          # (false for a NaN bound)
    count, front = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    monotone = np.ones(n, bool)
    counted_pairs = []

    with np.errstate(all="ignore"):
        inside, ok, enter, g = box_entry(sc, o, d)
        # ---- grid.cpp:187-216: per-axis setup, as occlusion_ref.walk
        pos = np.clip(cvt_i32((g - sc.bmin) * sc.icw), 0, sc.dims - 1)
        up, zero = d > F(0), d == F(0)
        face = sc.bmin + (pos + up).astype(F) * sc.cw
        nct = np.where(zero, FLT_MAX, enter[:, None] + (face - g) / d).astype(F)
        dt = np.where(zero, F(0), np.where(up, sc.cw / d, (-sc.cw) / d)).astype(F)
        step = np.where(zero, 0, np.where(up, 1, -1)).astype(np.int64)
        out = np.where(zero, pos, np.where(up, sc.dims, -1)).astype(np.int64)
        t_in = np.full(n, -np.inf, F)                                                   # point 0

        act = np.flatnonzero(valid & (inside | ok))
        D0, D02 = int(sc.dims[0]), int(sc.dims[0] * sc.dims[2])
        while act.size:
            n0, n1, n2 = nct[act, 0], nct[act, 1], nct[act, 2]
            ax = np.where(n0 < n1, np.where(n0 < n2, 0, 2), np.where(n1 < n2, 1, 2))     # grid.cpp:236-239
            nax = nct[act, ax]
            monotone[act] &= ~(nax < t_in[act])
            cell = pos[act, 0] + pos[act, 2] * D0 + pos[act, 1] * D02                   # GridIdx
            kb = sc.offs[cell]
            ln = sc.offs[cell + 1] - kb
            csum = np.cumsum(ln)
            lo_row = 0
            while lo_row < act.size:
                base = int(csum[lo_row - 1]) if lo_row else 0
                hi_row = max(lo_row + 1, int(np.searchsorted(csum, base + PAIRS_PER_SLICE, side="right")))
                rows_of = np.arange(lo_row, hi_row)
                lo_row = hi_row
                sl = ln[rows_of]
                m = int(sl.sum())
                if m == 0:
                    continue
                first_pair = np.cumsum(sl) - sl
                rows = np.repeat(rows_of, sl)
                k = np.arange(m) - np.repeat(first_pair, sl)
                r = act[rows]
                ti = sc.cell_tris[kb[rows] + k]
                h, ct, _, _ = ray_tri(o[r], d[r], sc.v0[ti], sc.v1[ti], sc.v2[ti])
                det = tri_det(d[r], sc.v0[ti], sc.v1[ti], sc.v2[ti])
                cnt = h & (t_in[r] <= ct) & (ct < nax[rows]) & (tmin[r] < ct) & (ct < tmax[r])   # point 1
                np.add.at(count, r[cnt], 1)                                                      # point 2
                np.add.at(front, r[cnt & (det > F(0))], 1)
                if pairs:
                    counted_pairs.append(np.stack([r[cnt], ti[cnt]], axis=1))
            go = ~(nax >= tmax[act])                                                    # point 3
            t_in[act[go]] = nax[go]
            # ---- grid.cpp:274-277: advance
            a, axg = act[go], ax[go]
            pos[a, axg] += step[a, axg]
            stay = pos[a, axg] != out[a, axg]
            a, axg = a[stay], axg[stay]
            nct[a, axg] = nct[a, axg] + dt[a, axg]
            act = a
    res = {"count": count, "front": front, "crossings": monotone}
    if pairs:
        res["pairs"] = (np.concatenate(counted_pairs) if counted_pairs else np.zeros((0, 2), np.int64)).astype(np.int64)
    return res


def brute_count(sc, rays, tminmax=None, chunk=1 << 20):
    """B and B_front of include/rt_tracer.h: per ray, the mesh triangles whose IntersectRayTri hit lies in
    (tmin, tmax), and those of them with det > 0 -- over every (ray, triangle) pair, with occlusion_ref.ray_tri."""
    rays = np.ascontiguousarray(rays, F)
    n, nt = rays.shape[0], sc.v0.shape[0]
    tmin, tmax = intervals_of(n, tminmax)
    valid = np.isfinite(rays).all(1) & (tmin < tmax)
    B, Bf = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    per = max(1, chunk // max(1, nt))
    with np.errstate(all="ignore"):
        for lo in range(0, n, per):
            r = np.repeat(np.arange(lo, min(n, lo + per)), nt)
            ti = np.tile(np.arange(nt), r.size // nt)
            o, d = rays[r, :3], rays[r, 3:]
            h, ct, _, _ = ray_tri(o, d, sc.v0[ti], sc.v1[ti], sc.v2[ti])
            det = tri_det(d, sc.v0[ti], sc.v1[ti], sc.v2[ti])
            ok = h & valid[r] & (tmin[r] < ct) & (ct < tmax[r])
            np.add.at(B, r[ok], 1)
            np.add.at(Bf, r[ok & (det > F(0))], 1)
    return B, Bf


# ------------------------------------------------------------------ two closed, outward-oriented meshes
CUBE_CENTRE, CUBE_HALF = np.array([0.125, -0.25, 0.375], F), F(1.0)
SPHERE_CENTRE, SPHERE_RADIUS = np.array([-0.25, 0.125, 0.5], F), F(1.0)
CUBE_SHELL, SPHERE_SHELL = 1e-3, 0.02          # points nearer the surface than this are not classified


def cube_tris():
    """The 12 triangles [12, 3, 3] of the cube CUBE_CENTRE +- CUBE_HALF, e1 x e2 pointing outwards."""
    out = []
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for s in (-1.0, 1.0):
            def p(x, y):
                v = np.zeros(3)
                v[axis], v[a], v[b] = s, x, y
                return v
            q = [p(-1, -1), p(1, -1), p(1, 1), p(-1, 1)]
            if s < 0:
                q.reverse()
            out += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return (np.array(out) * float(CUBE_HALF) + CUBE_CENTRE.astype(np.float64)).astype(F)


def sphere_tris(levels=4):
    """An octahedron subdivided `levels` times, its vertices on the sphere: 8 x 4^levels = 2,048 triangles
    [n, 3, 3], e1 x e2 pointing outwards.  The polyhedron lies within 0.002 of the sphere."""
    t = []
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                a, b, c = np.array([sx, 0, 0.0]), np.array([0, sy, 0.0]), np.array([0, 0, sz * 1.0])
                t.append([a, b, c] if sx * sy * sz > 0 else [a, c, b])
    t = np.array(t)
    for _ in range(levels):
        a, b, c = t[:, 0], t[:, 1], t[:, 2]
        ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
        t = np.concatenate([np.stack(x, axis=1) for x in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    t = t / np.sqrt((t * t).sum(2, keepdims=True))
    return (t * float(SPHERE_RADIUS) + SPHERE_CENTRE.astype(np.float64)).astype(F)


def closed_mesh_points(name, n, seed):
    """(points f32 [n, 3] within 1.6 of the mesh's centre and outside its shell, analytic inside bool [n])."""
    r = np.random.Generator(np.random.PCG64(seed))
    centre = (CUBE_CENTRE if name == "cube" else SPHERE_CENTRE).astype(np.float64)
    pts = np.zeros((0, 3), F)
    while pts.shape[0] < n:
        p = (centre + r.uniform(-1.6, 1.6, (2 * n, 3))).astype(F)
        q = p.astype(np.float64) - centre
        if name == "cube":
            off = np.abs(np.abs(q) - float(CUBE_HALF)).min(1)     # >= the distance to the nearest face plane
            keep = off > CUBE_SHELL
        else:
            keep = np.abs(np.sqrt((q * q).sum(1)) - float(SPHERE_RADIUS)) > SPHERE_SHELL
        pts = np.concatenate([pts, p[keep]])
    pts = np.ascontiguousarray(pts[:n])
    q = pts.astype(np.float64) - centre
    inside = (np.abs(q) < float(CUBE_HALF)).all(1) if name == "cube" else np.sqrt((q * q).sum(1)) < float(SPHERE_RADIUS)
    return pts, inside


def inside_vote(sc, points, dirs, rule="winding"):
    """GpuScene.inside restated: per point the majority, over the directions, of count - 2 front > 0 (winding) or
    count odd (parity) for the ray (point, direction) over (0, +inf)."""
    points, dirs = np.ascontiguousarray(points, F), np.ascontiguousarray(dirs, F)
    n, k = points.shape[0], dirs.shape[0]
    rays = np.empty((k, n, 6), F)
    rays[:, :, :3] = points
    rays[:, :, 3:] = dirs[:, None, :]
    tmm = np.tile(np.array([0.0, np.inf], F), (n * k, 1))
    res = walk_count(sc, rays.reshape(n * k, 6), tmm)
    c, f = res["count"].astype(np.int64).reshape(k, n), res["front"].astype(np.int64).reshape(k, n)
    yes = (c - 2 * f) > 0 if rule == "winding" else (c & 1) != 0
    return yes.sum(0) * 2 > k
