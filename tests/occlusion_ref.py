"""A numpy float32 restatement of the walk rt_occluded_rays_device is defined by (include/rt_tracer.h), and of
Grid::Intersect itself, shared by tests/test_occlusion_cpu.py and tests/test_ray_sets_cpu.py (which pin it to the
reference's records, on camera rays and on rays no camera makes) and tests/test_gpu_occlusion.py and
tests/test_gpu_ray_sets.py (which hold the kernel to it, byte for byte).  A plain module, numpy only.

Restated from the reference, one float32 operation per reference operation, in its order, nothing fused (two
numpy ufunc calls cannot contract into an FMA):
  IntersectPointAABB, IntersectRayAABB (aabb.h:9-13, 34-83), ToVoxel / ToPos (grid.h:44-51), the 3D-DDA of
  Grid::Intersect (grid.cpp:159-281), IntersectRayTri's non-culling branch (triangle.h:15-107).
Vectorised over rays: every ray carries its own walk state, and one outer iteration is one cell of every ray
still walking; a cell's list is tested as a whole and the outcome taken that testing it in order gives.

mode "closest": Grid::Intersect -> hit, tri, voxel (GridIdx of the accepted cell / the last cell walked;
0xFFFFFFFF when the ray misses the grid box), t, u, v, and the counts steps (cells visited) and tests (triangles
tested), as the fixtures of tests/golden/synth record them.
mode "any": the occlusion walk over (tmin, tmax) -> occluded (and steps, tests of that walk):
  1. a test counts iff hit && cur_t < next_crossing_t[step_axis] && tmin < cur_t && cur_t < tmax;
  2. the first counted test ends the walk with true;
  3. after a cell with no counted test, before the advance: next_crossing_t[step_axis] >= tmax ends it with false.
In both modes a ray with a non-finite component is a miss without a walk (rt_trace_rays_device's definition), and
in mode "any" so is a ray with a NaN bound or !(tmin < tmax).
"""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
EPS = F(0.00000001)                      # triangle.h:26
NOTRI = 0xFFFFFFFF
INT_MIN = -(2 ** 31)
PAIRS_PER_SLICE = 1 << 19                 # (ray, triangle) tests evaluated at once by walk()


class RefScene:
    """A scene's grid (CSR) and mesh as the restatement reads them."""

    def __init__(self, meta, offsets, cell_tris, vertices, triangles):
        self.dims = np.array([int(x) for x in meta["dims"]], np.int64)
        self.bmin = np.asarray(meta["aabb_min"], F).copy()
        self.bmax = np.asarray(meta["aabb_max"], F).copy()
        self.cw = F(meta["cell_wdh"])
        self.icw = F(meta["inv_cell_wdh"])
        self.offs = np.asarray(offsets).astype(np.int64)
        self.cell_tris = np.asarray(cell_tris).astype(np.int64)
        p = np.ascontiguousarray(np.asarray(vertices)[:, :3], F)
        idx = np.asarray(triangles)[:, :3].astype(np.int64)
        self.v0, self.v1, self.v2 = p[idx[:, 0]], p[idx[:, 1]], p[idx[:, 2]]

    @classmethod
    def from_host(cls, hs):
        """hs: the package's HostScene (grid() and mesh() return copies of the reference-pinned builder's arrays)."""
        meta, offs, tris = hs.grid()
        v, t = hs.mesh()
        return cls(meta, offs, tris, v, t)

    def diagonal(self):
        e = (self.bmax - self.bmin).astype(np.float64)
        return F(np.sqrt((e * e).sum()))


def cvt_i32(x):
    """int(float) as the reference's x86 build converts (cvttss2si): truncation, INT_MIN when out of range or NaN."""
    ok = np.isfinite(x) & (np.abs(x) < F(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, x, F(0))), INT_MIN).astype(np.int64)


def ray_tri(o, d, v0, v1, v2):
    """IntersectRayTri, non-culling branch, on [m, 3] arrays -> (hit, t, u, v); t, u, v are only meaningful on a
    hit (the early returns of triangle.h:77-101 as one predicate over the same operations)."""
    e1, e2 = v1 - v0, v2 - v0                                             # SUB :41-42
    px = d[:, 1] * e2[:, 2] - d[:, 2] * e2[:, 1]                          # CROSS(pvec, dir, edge2) :45
    py = d[:, 2] * e2[:, 0] - d[:, 0] * e2[:, 2]
    pz = d[:, 0] * e2[:, 1] - d[:, 1] * e2[:, 0]
    det = (e1[:, 0] * px + e1[:, 1] * py) + e1[:, 2] * pz                 # DOT :48
    inv = F(1.0) / det                                                    # :79
    tv = o - v0                                                           # SUB :82
    u = ((tv[:, 0] * px + tv[:, 1] * py) + tv[:, 2] * pz) * inv           # :85
    qx = tv[:, 1] * e1[:, 2] - tv[:, 2] * e1[:, 1]                        # CROSS(qvec, tvec, edge1) :90
    qy = tv[:, 2] * e1[:, 0] - tv[:, 0] * e1[:, 2]
    qz = tv[:, 0] * e1[:, 1] - tv[:, 1] * e1[:, 0]
    v = ((d[:, 0] * qx + d[:, 1] * qy) + d[:, 2] * qz) * inv              # :93
    t = ((e2[:, 0] * qx + e2[:, 1] * qy) + e2[:, 2] * qz) * inv           # :98
    hit = ~((det > -EPS) & (det < EPS)) & ~((u < F(0)) | (u > F(1))) & ~((v < F(0)) | (u + v > F(1))) & (t >= F(0))
    return hit, t, u, v


def box_entry(sc, o, d):
    """grid.cpp:174-185, the on-grid origin, on [n, 3] arrays -> (inside, ok, enter_t, grid_intersection):
    IntersectPointAABB, else IntersectRayAABB's tmin (ok = the slab test's verdict, only meaningful where not inside)."""
    with np.errstate(all="ignore"):
        inside = ((o >= sc.bmin) & (o <= sc.bmax)).all(1)                 # IntersectPointAABB
        inv = F(1.0) / d                                                  # aabb.h:49
        sign = inv < F(0)
        lo, hi = np.where(sign, sc.bmax, sc.bmin), np.where(sign, sc.bmin, sc.bmax)
        t0 = (lo[:, 0] - o[:, 0]) * inv[:, 0]
        t1 = (hi[:, 0] - o[:, 0]) * inv[:, 0]
        ty0 = (lo[:, 1] - o[:, 1]) * inv[:, 1]
        ty1 = (hi[:, 1] - o[:, 1]) * inv[:, 1]
        ok = ~((t0 > ty1) | (ty0 > t1))
        t0 = np.where(ty0 > t0, ty0, t0)
        t1 = np.where(ty1 < t1, ty1, t1)
        tz0 = (lo[:, 2] - o[:, 2]) * inv[:, 2]
        tz1 = (hi[:, 2] - o[:, 2]) * inv[:, 2]
        ok &= ~((t0 > tz1) | (tz0 > t1))
        t0 = np.where(tz0 > t0, tz0, t0)
        enter = np.where(inside, F(0), t0).astype(F)
        g = np.where(inside[:, None], o, o + d * enter[:, None]).astype(F)
    return inside, ok, enter, g


def walk(sc, rays, tminmax=None, mode="closest"):
    """rays [n, 6] f32 (origin, direction as passed); tminmax [n, 2] f32 or None = (-inf, +inf).  Returns a dict of
    per-ray arrays: mode "closest": hit (bool), tri, voxel (u32), t, u, v (f32), steps, tests (u32);
    mode "any": occluded (bool), steps, tests."""
    assert mode in ("closest", "any")
    anyhit = mode == "any"
    rays = np.ascontiguousarray(rays, F)
    n = rays.shape[0]
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    valid = np.isfinite(rays).all(1)
    if anyhit:
        if tminmax is None:
            tmin, tmax = np.full(n, -np.inf, F), np.full(n, np.inf, F)
        else:
            tmm = np.ascontiguousarray(tminmax, F)
            tmin, tmax = tmm[:, 0].copy(), tmm[:, 1].copy()
        valid &= tmin < tmax                   # false for a NaN bound
    hit = np.zeros(n, bool)
    tri = np.full(n, NOTRI, np.uint32)
    voxel = np.full(n, NOTRI, np.uint32)
    tt, uu, vv = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
    steps, tests = np.zeros(n, np.uint32), np.zeros(n, np.uint32)

    with np.errstate(all="ignore"):
        inside, ok, enter, g = box_entry(sc, o, d)

        # ---- grid.cpp:187-216: per-axis setup
        pos = np.clip(cvt_i32((g - sc.bmin) * sc.icw), 0, sc.dims - 1)    # ToVoxel
        up, zero = d > F(0), d == F(0)
        face = sc.bmin + (pos + up).astype(F) * sc.cw                     # ToPos(pos + 1) / ToPos(pos)
        nct = np.where(zero, FLT_MAX, enter[:, None] + (face - g) / d).astype(F)
        dt = np.where(zero, F(0), np.where(up, sc.cw / d, (-sc.cw) / d)).astype(F)
        step = np.where(zero, 0, np.where(up, 1, -1)).astype(np.int64)
        out = np.where(zero, pos, np.where(up, sc.dims, -1)).astype(np.int64)   # (a still axis: its step ends the walk)

        act = np.flatnonzero(valid & (inside | ok))
        D0, D02 = int(sc.dims[0]), int(sc.dims[0] * sc.dims[2])
        while act.size:
            n0, n1, n2 = nct[act, 0], nct[act, 1], nct[act, 2]
            ax = np.where(n0 < n1, np.where(n0 < n2, 0, 2), np.where(n1 < n2, 1, 2))     # grid.cpp:236-239
            nax = nct[act, ax]
            cell = pos[act, 0] + pos[act, 2] * D0 + pos[act, 1] * D02                   # GridIdx
            steps[act] += 1
            voxel[act] = cell
            kb = sc.offs[cell]
            ln = sc.offs[cell + 1] - kb
            # ---- grid.cpp:243-267: the cells' lists as one array of (ray, list position) pairs, a slice of rays at
            # a time.  The list is tested in order, so a closest walk keeps the FIRST position that holds the least
            # accepted cur_t (the strict "cur_t < t" never replaces an equal one), and an any-hit walk stops at the
            # first counted position.
            best = np.full(act.size, FLT_MAX, F)             # closest: t (FLT_MAX at every cell's start)
            done = np.zeros(act.size, bool)                  # any: a test counted
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
                seg = first_pair[sl > 0]                     # reduceat boundaries: the non-empty lists
                srow = rows_of[sl > 0]
                r = act[rows]
                ti = sc.cell_tris[kb[rows] + k]
                h, ct, cu, cv = ray_tri(o[r], d[r], sc.v0[ti], sc.v1[ti], sc.v2[ti])
                if anyhit:
                    cnt = h & (ct < nax[rows]) & (tmin[r] < ct) & (ct < tmax[r])
                    first = np.minimum.reduceat(np.where(cnt, k, m), seg)
                    found = first < m
                    done[srow[found]] = True
                    tests[act[srow]] += np.where(found, first + 1, sl[sl > 0]).astype(np.uint32)
                else:
                    ok_t = h & (ct < FLT_MAX) & (ct < nax[rows])
                    val = np.where(ok_t, ct, F(np.inf)).astype(F)
                    least = np.minimum.reduceat(val, seg)
                    found = least < F(np.inf)
                    at = np.minimum.reduceat(np.where(ok_t & (val == np.repeat(least, sl[sl > 0])), np.arange(m), m), seg)
                    w, at = srow[found], at[found]
                    best[w] = ct[at]
                    rw = act[w]
                    tt[rw], uu[rw], vv[rw], tri[rw] = ct[at], cu[at], cv[at], ti[at]
                    tests[act[srow]] += sl[sl > 0].astype(np.uint32)
            if anyhit:
                hit[act[done]] = True
                go = ~done & ~(nax >= tmax[act])             # rule 3
            else:
                done = best != FLT_MAX                       # grid.cpp:270
                hit[act[done]] = True
                go = ~done
            # ---- grid.cpp:274-277: advance
            a, axg = act[go], ax[go]
            pos[a, axg] += step[a, axg]
            stay = pos[a, axg] != out[a, axg]
            a, axg = a[stay], axg[stay]
            nct[a, axg] = nct[a, axg] + dt[a, axg]
            act = a
    if anyhit:
        return {"occluded": hit, "steps": steps, "tests": tests}
    return {"hit": hit, "tri": tri, "voxel": voxel, "t": tt, "u": uu, "v": vv, "steps": steps, "tests": tests}


def rec11(res):
    """A closest-mode result as the reference's 11-word records (tests/synth_scenes.py COLS): hit, tri, t, u, v,
    r, g, b (0 here), voxel, steps, tests; tri 0xFFFFFFFF and t = u = v = 0 on a miss, voxel 0xFFFFFFFF on a hit."""
    n = res["hit"].shape[0]
    out = np.zeros((n, 11), np.uint32)
    h = res["hit"]
    out[:, 0] = h
    out[:, 1] = np.where(h, res["tri"], np.uint32(NOTRI))
    for j, k in ((2, "t"), (3, "u"), (4, "v")):
        out[:, j] = np.where(h, res[k], F(0)).astype(F).view(np.uint32)
    out[:, 8] = res["voxel"]
    out[:, 9] = res["steps"]
    out[:, 10] = res["tests"]
    return out
