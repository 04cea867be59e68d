"""The reference of rt_distance_points_device (GpuScene.distance): Renderer::DistanceBruteForce (renderer.cpp:138-155)
by the oracle's orc_kat_dist, which tests/golden/kat_dist.f32.gz pins to the reference's DistancePointTri.

    d[i, j]  = DistancePointTri(p_i, v0_j, v1_j, v2_j)
    dist_i   = np.fmin.reduce(d[i], initial=FLT_MAX)      the reference's loop exactly: std::min(dist, d) is
                                                          (d < dist) ? d : dist, which never selects a NaN (fmin drops
                                                          it) nor anything at or above FLT_MAX
    tri_i    = the first j with d[i, j] == dist_i, else 0xFFFFFFFF

No point is excluded from any comparison: the reference is defined for every float.
"""
import numpy as np

NOTRI = 0xFFFFFFFF
FLT_MAX = np.finfo(np.float32).max
CHUNK = 1 << 21                 # (point, triangle) pairs per oracle call


def triangles_of(vertices, triangles):
    """(vertices f32 [nv, 6], triangles u32 [nt, 6]) -> corner positions f32 [nt, 3, 3]."""
    p = np.ascontiguousarray(vertices, np.float32)[:, :3]
    return np.ascontiguousarray(p[np.ascontiguousarray(triangles).view(np.uint32)[:, :3].astype(np.int64)], np.float32)


def all_distances(oracle, points, tris):
    """d f32 [np, nt], in chunks of whole points."""
    points = np.ascontiguousarray(points, np.float32)
    t9 = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    n, nt = points.shape[0], t9.shape[0]
    d = np.empty((n, nt), np.float32)
    step = max(1, CHUNK // max(nt, 1))
    for i0 in range(0, n, step):
        m = min(step, n - i0)
        rin = np.empty((m, nt, 12), np.float32)
        rin[:, :, :3] = points[i0:i0 + m, None, :]
        rin[:, :, 3:] = t9[None, :, :]
        d[i0:i0 + m] = oracle.kat("dist", rin.reshape(m * nt, 12), 1).reshape(m, nt)
    return d


def reduce_rule(d):
    """(dist f32 [np], tri u32 [np]) of a distance matrix: the reference's loop and the lowest-index rule."""
    d = np.asarray(d, np.float32)
    n = d.shape[0]
    if d.shape[1] == 0:
        return np.full(n, FLT_MAX, np.float32), np.full(n, NOTRI, np.uint32)
    with np.errstate(invalid="ignore"):
        dist = np.fmin.reduce(d, axis=1, initial=FLT_MAX).astype(np.float32)
        eq = d == dist[:, None]
    tri = np.where(eq.any(1), eq.argmax(1), NOTRI).astype(np.uint32)
    return dist, tri


def reference(oracle, points, tris):
    return reduce_rule(all_distances(oracle, points, tris))


def closest_identity(points, closest):
    """sqrtf((dx*dx + dy*dy) + dz*dz) with d = p - q, every operation one f32 rounding."""
    p = np.ascontiguousarray(points, np.float32)
    q = np.ascontiguousarray(closest, np.float32)
    with np.errstate(all="ignore"):
        d = (p - q).astype(np.float32)
        s = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float32) + d[:, 2] * d[:, 2]).astype(np.float32)
        return np.sqrt(s, dtype=np.float32)


def families(tris, n_each, seed):
    """Five point families of a mesh, n_each points of each, f32 [5 n_each, 3]: inside the vertex box, 1e-3 of the
    box diagonal off the surface, on vertices, 1,024 diagonals away, 2^20 diagonals away."""
    r = np.random.Generator(np.random.PCG64(seed))
    tris = np.ascontiguousarray(tris, np.float32)
    v = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    diag = float(np.sqrt(((hi - lo) ** 2).sum())) or 1.0
    inside = r.uniform(lo, hi, (n_each, 3))
    pick = tris[r.integers(0, tris.shape[0], n_each)].astype(np.float64)
    b = r.dirichlet((1.0, 1.0, 1.0), n_each)
    on = (pick * b[:, :, None]).sum(1)
    u = r.normal(size=(n_each, 3))
    u /= np.sqrt((u * u).sum(1))[:, None]
    near = on + 1e-3 * diag * u
    verts = v[r.integers(0, v.shape[0], n_each)]
    w = r.normal(size=(2 * n_each, 3))
    w /= np.sqrt((w * w).sum(1))[:, None]
    mid = 0.5 * (lo + hi)
    far = mid + 1024.0 * diag * w[:n_each]
    vfar = mid + float(2 ** 20) * diag * w[n_each:]
    return np.ascontiguousarray(np.concatenate([inside, near, verts, far, vfar]), np.float32)
