"""Meshes that sit on the edges of the grid builders (host/rt_host.cpp build_grid, csrc/rt_grid_build.hip),
shared by oracle/gen_golden_grid.py (which pins each one to the reference's own Grid::Grid),
tests/test_grid_adversarial.py and tests/test_gpu_grid_edges.py.  A plain module, not a conftest.

The ten shipped scenes are normalised, centred, 64-cell meshes.  These are not: vertices exactly on cell
planes, all-negative coordinates (the reference seeds the AABB max with float::min(), so the grid reaches
to 0 and every triangle's cell range runs to the far corner), offsets on either side of where the 0.0001
pad rounds away, single triangles, needles, other resolutions -- and sizes that put the device build's
triangle count and key count on the edges of its 1,024-element scan and sort tiles.

Every mesh comes from a fixed seed through numpy's PCG64 and float32 arithmetic; tests/golden/grid.json
carries the SHA-256 of each mesh's bytes, so a changed generator cannot silently move a mesh off its edge.
Meshes are built on demand (mesh(name)): the largest has 1,048,577 triangles.
"""
import hashlib
import json
import os
import struct

import numpy as np

from conftest import GOLD
from synth_scenes import anchors, mesh_of

FIXTURE = os.path.join(GOLD, "grid.json")
F = np.float32


# ------------------------------------------------------------------ the reference's cell planes
def box_grid(lo, hi, res):
    """(aabb_min, cell_wdh) in float32 as grid.cpp:29-36 forms them for a mesh whose AABB is [lo, hi]^3
    (hi > 0: the float::min() seed of the maximum plays no part)."""
    bmin = F(F(lo) - F(0.0001))
    bmax = F(F(hi) + F(0.0001))
    return bmin, F(F(bmax - bmin) / F(res))


def plane(bmin, cw, i):
    """Cell plane i as grid.cpp:101-108 forms it: aabb_min + float(i) * cell_wdh, each step in float32."""
    return F(bmin + F(F(i) * cw))


def inner_planes(res, limit=0.8):
    """The planes of the res-cell grid over [-1, 1]^3 that lie within [-limit, limit]."""
    bmin, cw = box_grid(-1.0, 1.0, res)
    p = np.array([plane(bmin, cw, i) for i in range(res + 1)], F)
    return p[np.abs(p) <= limit]


# ------------------------------------------------------------------ geometry
def tiny(r, n, half=0.004, span=0.95, centre=0.0):
    """n triangles of about 2 * half around random centres.  A triangle with a negative maximum on an axis gets
    the float::min() seed there (triangle.h:116-131), so its candidate cells run on to the plane of 0; with
    centre >= span + half every coordinate is positive and a tiny triangle has at most 8 candidates."""
    c = centre + r.uniform(-span, span, (n, 1, 3))
    return (c + r.uniform(-half, half, (n, 3, 3))).astype(F)


def planes(res, seed=101):
    """300 triangles of about 0.2 around a vertex that sits exactly on a cell plane of the res-cell grid over
    [-1, 1]^3: 100 with a vertex on an x plane, 100 with an edge in a y plane, 100 with a vertex on a cell
    corner; plus the corner anchors that fix the box."""
    r = np.random.Generator(np.random.PCG64(seed))
    pl = inner_planes(res)
    n = 300
    p = r.uniform(-0.8, 0.8, (n, 3)).astype(F)
    pick = pl[r.integers(0, len(pl), (n, 3))]
    p[:100, 0] = pick[:100, 0]                       # vertex on an x plane
    p[100:200, 1] = pick[100:200, 1]                 # edge in a y plane (below: v1.y = v0.y)
    p[200:] = pick[200:]                             # vertex on a cell corner
    tris = np.repeat(p[:, None, :], 3, axis=1)
    tris[:, 1:] += r.uniform(-0.2, 0.2, (n, 2, 3)).astype(F)
    tris[100:200, 1, 1] = tris[100:200, 0, 1]
    return np.concatenate([tris, anchors()])


# z planes of the 64-cell grid over [-1, 1]^3 on which a triangle lying in the plane is claimed by neither
# neighbouring cell (the float centre / half-size conversion of aabb.h:19-26 leaves it just outside both): the
# reference aborts on such a triangle (grid.cpp:125).  Found by building each inner plane's triangle alone.
UNCLAIMED_Z_PLANES = (12,)


def inplane_z(which=None, seed=102, unclaimed=False):
    """40 triangles lying in z cell planes of the 64-cell grid over [-1, 1]^3 (all three vertices on the
    plane), or only triangle `which` of them; plus the anchors.  The planes are drawn from the inner ones that
    are not UNCLAIMED_Z_PLANES, or with unclaimed=True from those alone."""
    r = np.random.Generator(np.random.PCG64(seed))
    bmin, cw = box_grid(-1.0, 1.0, 64)
    idx = [i for i in range(65) if abs(plane(bmin, cw, i)) <= 0.8 and (i in UNCLAIMED_Z_PLANES) == unclaimed]
    pl = np.array([plane(bmin, cw, i) for i in idx], F)
    n = 40
    c = r.uniform(-0.75, 0.75, (n, 1, 3))
    tris = (c + r.uniform(-0.2, 0.2, (n, 3, 3))).astype(F)
    tris[:, :, 2] = pl[r.integers(0, len(pl), n)][:, None]
    if which is not None:
        tris = tris[which:which + 1]
    return np.concatenate([tris, anchors()])


def degenerate(seed=103):
    """50 point triangles, 50 collinear ones, 20 triangles that each appear twice; no anchors."""
    r = np.random.Generator(np.random.PCG64(seed))
    pt = np.repeat(r.uniform(-1, 1, (50, 1, 3)).astype(F), 3, axis=1)
    a = r.uniform(-1, 1, (50, 3)).astype(F)
    d = r.uniform(-0.1, 0.1, (50, 3)).astype(F)
    col = np.stack([a, a + d, a + d + d], axis=1).astype(F)
    dup = (r.uniform(-0.9, 0.9, (20, 1, 3)) + r.uniform(-0.1, 0.1, (20, 3, 3))).astype(F)
    return np.concatenate([pt[:25], dup, col, pt[25:], dup])


def corner_points(seed=104):
    """30 point triangles exactly on cell corners of the 64-cell grid over [-1, 1]^3, plus the anchors."""
    r = np.random.Generator(np.random.PCG64(seed))
    pl = inner_planes(64)
    p = pl[r.integers(0, len(pl), (30, 3))]
    return np.concatenate([np.repeat(p[:, None, :], 3, axis=1), anchors()])


def cloud(seed=105, n=200, size=0.3):
    """n random triangles of about `size` in [-1, 1]^3 plus the anchors."""
    r = np.random.Generator(np.random.PCG64(seed))
    c = r.uniform(-0.7, 0.7, (n, 1, 3))
    tris = np.clip(c + r.uniform(-size, size, (n, 3, 3)), -0.98, 0.98).astype(F)
    return np.concatenate([tris, anchors()])


def shifted(offset):
    return (cloud() + F(offset)).astype(F)


def scaled(scale):
    return (cloud() * F(scale)).astype(F)


def single(kind):
    t = {"flat_z": [[-1, -1, 0.3], [1, -1, 0.3], [0, 1, 0.3]],
         "tilted": [[-1, -1, 0.1], [1, -0.5, 0.8], [0, 1, 1.5]],
         "point": [[0.3, 0.2, 0.5]] * 3,
         "needle": [[0, 0, 0], [1000, 0.001, 0], [500, 0, 0.001]]}[kind]
    return np.array([t], F)


def span2(seed=106):
    """2,000 tiny triangles plus two that span the grid."""
    r = np.random.Generator(np.random.PCG64(seed))
    big = np.array([[[-1, -1, -1], [1, 1, -1], [1, -1, 1]], [[-1, 1, 1], [1, -1, 1], [-1, -1, -1]]], F)
    return np.concatenate([tiny(r, 2000), big])


def skew(seed=107):
    """One triangle whose candidate range is the whole 64^3 grid between 2 x 1,000 tiny ones, all in positive
    coordinates: one lane of k_tri_ranges counts 262,144 candidates, its neighbours at most 8."""
    r = np.random.Generator(np.random.PCG64(seed))
    big = np.array([[[0, 0, 0], [2, 2, 0], [1, 1, 2]]], F)
    return np.concatenate([tiny(r, 1000, centre=1.0), big, tiny(r, 1000, centre=1.0)])


def all_negative(seed=108, n=300):
    """n triangles of about 0.08 with every coordinate below 0, denser towards the minimum corner.  The grid
    reaches from about -2 to 0.0001 and every triangle's cell range runs to the far corner: tens of millions
    of candidate cells for a few thousand references."""
    r = np.random.Generator(np.random.PCG64(seed))
    u = r.uniform(0.0, 1.0, (n, 1, 3))
    c = -2.0 + 1.9 * u * u
    tris = (c + r.uniform(-0.04, 0.04, (n, 3, 3))).astype(F)
    tris[0, 0] = (-2.0, -2.0, -2.0)
    assert (tris < 0).all()
    return tris


def big(seed=109, n=1048577):
    """n - 2 small proper triangles (about half a cell of the 128-cell grid) plus the anchors, in [0, 2]^3 (in
    negative coordinates the candidate count would pass the device build's limit): more than 1,048,576
    elements, the scan's third level, and 21 + 22 key bits."""
    r = np.random.Generator(np.random.PCG64(seed))
    return np.concatenate([tiny(r, n - 2, half=0.004, span=0.99, centre=1.0), anchors(0.0, 2.0)])


def points(nt, seed):
    """nt point triangles in (-1, 1)^3, the first at (-1, -1, -1) and (from two on) the last at (1, 1, 1): a
    point strictly inside a cell touches that cell alone, so the key count equals nt."""
    r = np.random.Generator(np.random.PCG64(seed))
    p = r.uniform(-0.999, 0.999, (nt, 3)).astype(F)
    p[0] = -1.0
    if nt > 1:
        p[-1] = 1.0
    return np.repeat(p[:, None, :], 3, axis=1)


def candidate_limit_mesh(seed=110, n=8300):
    """n small triangles inside the minimum-corner cell of an all-negative mesh: each one's candidate range is
    the whole 64^3 grid, n * 262,144 >= 2^31 candidates.  NOT a catalogue case: the reference accepts it,
    but its build (and the host's) takes minutes; only the device build's limit is tested on it."""
    r = np.random.Generator(np.random.PCG64(seed))
    tris = (-1.0 + r.uniform(0.0, 0.012, (n, 3, 3))).astype(F)
    tris[0, 0] = (-1.0, -1.0, -1.0)
    return tris


# ------------------------------------------------------------------ the catalogue
SIZES = [(nt, 64) for nt in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)] + \
        [(4097, 7), (5000, 1), (100, 1)]          # (100, 1): 7 + 1 key bits, the one-pass sort


def _catalogue():
    c = {}

    def add(name, fn, args=(), res=64, accept=True, kind="geometry"):
        c[name] = dict(fn=fn, args=tuple(args), res=res, accept=accept, kind=kind)

    add("planes", planes, (64,))
    for res in (1, 7, 200):
        add(f"planes_res{res}", planes, (64,), res=res)          # the same mesh at other resolutions
    add("planes7_res7", planes, (7,), res=7)                     # on the planes of their own grids
    add("planes200_res200", planes, (200,), res=200)
    add("inplane_z", inplane_z)
    for i in range(6):
        add(f"inplane_z_one{i}", inplane_z, (i,))
    add("inplane_z_unclaimed", inplane_z, (0, 102, True), accept=False)
    add("degenerate", degenerate)
    add("corner_points", corner_points, accept=False)
    for off, ok in ((1024, True), (2048, False), (4096, False), (65536, False),
                    (-3, True), (-1024, True), (-4096, True), (-65536, True)):
        add(f"shift_{off:+d}", shifted, (off,), accept=ok)
    for k in ("flat_z", "tilted", "point", "needle"):
        add(f"single_{k}", single, (k,))
    add("extent_1e-3", scaled, (1e-3,))
    add("extent_1e-6", scaled, (1e-6,))
    add("span2", span2)
    add("skew", skew, kind="skew")
    add("all_negative", all_negative, kind="all_negative")
    add("big", big, res=128, kind="big")
    for nt, res in SIZES:
        add(f"points_{nt}_res{res}", points, (nt, 1000 + nt), res=res, kind="size")
    return c


CASES = _catalogue()
ACCEPTED = [n for n, c in CASES.items() if c["accept"]]
REJECTED = [n for n, c in CASES.items() if not c["accept"]]
THREADED = ("planes", "degenerate", "all_negative", "skew")      # host build at nthreads 1, 3, 8
_cache = {}


def mesh(name):
    """(vertices f32 [nv, 6], triangles u32 [nt, 6]) of a catalogue case; built once per process, read-only."""
    if name not in _cache:
        c = CASES[name]
        v, t = mesh_of(c["fn"](*c["args"]))
        v.setflags(write=False)
        t.setflags(write=False)
        if c["kind"] == "big":
            return v, t                                          # 50 MB: not kept
        _cache[name] = (v, t)
    return _cache[name]


def mesh_sha(v, t):
    return hashlib.sha256(np.ascontiguousarray(v).tobytes() + np.ascontiguousarray(t).tobytes()).hexdigest()


def write_rtscene(path, v, t, fov=45.0, cam=None):
    """The .rtscene layout (oracle/ref_driver.cpp ReadScene, host read_scene)."""
    cam = np.eye(4, dtype=F).reshape(16) if cam is None else np.asarray(cam, F).reshape(16)
    with open(path, "wb") as f:
        f.write(b"RTSCENE1" + struct.pack("<If", 0xFFFFFFFF, fov) + cam.astype("<f4").tobytes() +
                struct.pack("<II", v.shape[0], t.shape[0]))
        f.write(np.ascontiguousarray(v, "<f4").tobytes())
        f.write(np.ascontiguousarray(t, "<u4").tobytes())


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def bits(x):
    return [f"{w:08x}" for w in np.asarray(x, F).reshape(-1).view(np.uint32)]


def meta_bits(meta):
    """The eight metadata words (aabb_min, aabb_max, cell_wdh, inv_cell_wdh) of a grid() / gpu_grid_build meta."""
    return bits(meta["aabb_min"]) + bits(meta["aabb_max"]) + bits([meta["cell_wdh"]]) + bits([meta["inv_cell_wdh"]])


def csr_sha(offs, tris):
    """The CSR hash of tests/test_host_grid.py: offsets || refs."""
    return hashlib.sha256(np.ascontiguousarray(offs, "<u4").tobytes() +
                          np.ascontiguousarray(tris, "<u4").tobytes()).hexdigest()


def check_against_fixture(e, meta, offs, tris, what):
    """dims, metadata bits, reference count, fullest cell and CSR SHA-256 of a build against a fixture entry."""
    assert meta["dims"] == e["dims"], what
    assert meta_bits(meta) == e["meta_bits"], what
    assert int(offs[-1]) == e["num_refs"] == len(tris), what
    assert int(np.diff(offs).max()) == e["max_refs_per_cell"], what
    assert csr_sha(offs, tris) == e["csr_sha256"], what


def sort_passes(nt, dims):
    """Passes of the device build's radix sort, as build() of rt_grid_build.hip computes them: 8 bits a pass
    over tb + cb key bits (tb: bits of nt - 1, at least 1; cb: bits of the cell count)."""
    tb = max(1, int(nt - 1).bit_length())
    cb = int(dims[0] * dims[1] * dims[2]).bit_length()
    return (tb + cb + 7) // 8
