"""Rays that no camera makes, and the reference's answers for them (tests/golden/rays), shared by
oracle/gen_golden_rays.py (which builds the sets here and has the reference's own Grid::Intersect answer them),
tests/test_ray_sets_cpu.py and tests/test_gpu_ray_sets.py.  A plain module, not a conftest.

Seven scenes, eight families per scene, in this order (sizes in FAMILIES; A-F are multiples of 64, so in family order a wave
holds one family up to G; the total is no multiple of 64, so the last wave is partly masked):

  A bounce     origins o + t d (f32) at closest hits of the scene's own 62x46x4 camera rays, 4 seeded unit directions
               each, unrestricted by hemisphere
  B interior   origins uniform inside the grid box; half seeded unit directions, half aimed: d = q - o (f32, not
               normalised) for a random barycentric point q of a random triangle
  C exterior   origins uniform in 3x the box, outside it; half aimed, a quarter random, a quarter aimed and negated
  D zeros      exact +-axis directions and directions with one or two components exactly +0.0 / -0.0; half of the
               origins lie on a line through a triangle point (so sparse scenes are hit too); in a quarter the origin's
               coordinate on a zeroed axis is exactly lo, hi or a ToPos(k): the 0 * inf case of the slab test
  E lattice    origins with one, two or three coordinates exactly lo, hi or ToPos(k) (faces, edges, corners, cell
               planes / edges / corners), the others interior; +-diagonal, +-axis and aimed directions; a quarter with
               the component on a lattice axis exactly zero, half of the rest negative there, half positive
  F ties       exterior origins with d = target - o (f32) for the 8 corners, the 12 edge midpoints and cell-lattice
               points (three lattice coordinates, or two and one free); and origins displaced from a cell-lattice point
               by a power-of-two multiple of (+-1, +-1, +-1) or (+-1, +-1, 0), walking back along that diagonal
  G lengths    48 rays of A-C per factor, directions times 2^-20, 2^-10, 2^-1, 7.9, 8, 8.5, 2^4, 2^10, 2^20: the first
               24 of each in blocks of one factor, the second 24 interleaved ray by ray
  H far        origins 2^6, 2^10, 2^14, 2^20 box diagonals from the centre, aimed at a triangle point or a box point
               with a jitter of a few cells

ToPos(k) = lo + float(k) * cell_wdh in float32 (grid.h:50).  Every generator is numpy's PCG64 seeded by
(SEED, scene, family); the rays are committed all the same, so the tests do not depend on numpy's random streams.
"""
import gzip
import hashlib
import json
import os

import numpy as np

from conftest import GOLD, ROOT

F = np.float32
RAYS = os.path.join(GOLD, "rays")
SEED = 20261020
SCENES = ("inside", "stack1500", "stack2100", "negative_octant", "flat_front", "scene1", "scene8")
# the scenes of tests/ray_variant_scenes.py (tests/golden/ray_variants): the same families, seeded by indices of
# their own after SCENES', so the seven sets above keep their seeds
VARIANT_SCENES = ("ribbon_x513", "ribbon_y513", "ribbon_z513", "ribbon_z512", "sheets16", "huge_axis_z", "huge_stack2100")
THIN_SCENE = "flat_front"                     # 64 x 64 x 1 cells
FAMILIES = (("A", 512), ("B", 384), ("C", 384), ("D", 256), ("E", 384), ("F", 192), ("G", 432), ("H", 200))
NAMES = tuple(n for n, _ in FAMILIES)
TOTAL = sum(k for _, k in FAMILIES)
CAM_FRAME = (62, 46, 4)                       # family A's camera rays (synth_scenes.W, H, SPP)
G_FACTORS = (2.0 ** -20, 2.0 ** -10, 0.5, 7.9, 8.0, 8.5, 16.0, 2.0 ** 10, 2.0 ** 20)
H_DISTANCES = (2.0 ** 6, 2.0 ** 10, 2.0 ** 14, 2.0 ** 20)
REC_COLS = ("hit", "tri", "t", "u", "v", "voxel", "steps", "tests")     # the 8-word record of `refdriver rays`
NOTRI = 0xFFFFFFFF
# non-vacuity, conditions on the reference's own records (hits, misses)
MIN_SHARE = 0.2                               # per scene, over all families: at least this share hits, and misses
MIN_PER_SCENE = {"A": 32, "B": 32, "E": 32, "G": 32, "D": 16}
MIN_ACROSS = {"C": 200, "F": 200, "H": 200}
MAX_EXCLUDED_SHARE = 0.005

# A-F are whole waves of 64, so in family order a wave up to there holds one family; G is 48 rays x 9 factors
assert all(k % 64 == 0 for _, k in FAMILIES[:6]) and TOTAL % 64 != 0 and len(G_FACTORS) * 48 == dict(FAMILIES)["G"]


def bounds():
    """{family: (first, past-the-end)} in the per-scene ray array."""
    out, o = {}, 0
    for n, k in FAMILIES:
        out[n] = (o, o + k)
        o += k
    return out


def scene_file(name, tmp_path):
    """The .rtscene of a scene of SCENES: a shipped one, or a synthetic one gunzipped under tmp_path."""
    if name.startswith("scene") and name[5:].isdigit():
        return os.path.join(ROOT, "data", "scenes", name + ".rtscene")
    out = os.path.join(str(tmp_path), name + ".rtscene")
    if not os.path.exists(out):
        with gzip.open(os.path.join(GOLD, "synth", name + ".rtscene.gz"), "rb") as f, open(out, "wb") as o:
            o.write(f.read())
    return out


# ------------------------------------------------------------------ fixtures
def meta():
    with open(os.path.join(RAYS, "rays.json")) as f:
        return json.load(f)


def read_fixture(name):
    with gzip.open(os.path.join(RAYS, name), "rb") as f:
        return f.read()


def load(scene):
    """(rays f32 [n, 6], records u32 [n, 8]) of a scene, as committed."""
    rays = np.frombuffer(read_fixture(scene + ".rays.gz"), "<f4").reshape(-1, 6)
    rec = np.frombuffer(read_fixture(scene + ".rec.gz"), "<u4").reshape(-1, 8)
    assert rays.shape[0] == rec.shape[0] == TOTAL, (scene, rays.shape, rec.shape)
    return rays, rec


def pinned(entry):
    """bool [TOTAL]: False at the rays rays.json lists as resting on undefined behaviour of the reference."""
    keep = np.ones(TOTAL, bool)
    keep[[x["index"] for x in entry["excluded"]]] = False
    return keep


def sha256(data):
    return hashlib.sha256(data).hexdigest()


def counts(rec, keep=None):
    """{family: [hits, misses]} of 8-word records (rays outside `keep` are not counted)."""
    keep = np.ones(rec.shape[0], bool) if keep is None else keep
    return {n: [int(((rec[a:b, 0] == 1) & keep[a:b]).sum()), int(((rec[a:b, 0] == 0) & keep[a:b]).sum())]
            for n, (a, b) in bounds().items()}


def check_non_vacuity(per_scene, waived=()):
    """per_scene {scene: counts()}; waived: (scene, family) pairs rays.json names.  Returns the list of failures."""
    bad = []
    for sc, c in per_scene.items():
        h, m = sum(v[0] for v in c.values()), sum(v[1] for v in c.values())
        if min(h, m) < MIN_SHARE * (h + m):
            bad.append((sc, "all", h, m))
        for fam, k in MIN_PER_SCENE.items():
            if min(c[fam]) < k and (sc, fam) not in waived:
                bad.append((sc, fam, c[fam]))
    for fam, k in MIN_ACROSS.items():
        tot = [sum(c[fam][j] for c in per_scene.values()) for j in (0, 1)]
        if min(tot) < k:
            bad.append(("across", fam, tot))
    return bad


# ------------------------------------------------------------------ the grid box
class Box:
    """The grid box as the reference holds it: lo, hi (m_aabb_min / max), cw (m_cell_wdh), dims."""

    def __init__(self, grid_meta):
        self.lo = np.asarray(grid_meta["aabb_min"], F).copy()
        self.hi = np.asarray(grid_meta["aabb_max"], F).copy()
        self.cw = F(grid_meta["cell_wdh"])
        self.dims = [int(x) for x in grid_meta["dims"]]
        self.ext = self.hi - self.lo
        self.ctr = (self.lo + self.hi) * F(0.5)
        e = self.ext.astype(np.float64)
        self.diag = F(np.sqrt((e * e).sum()))

    def topos(self, axis, k):
        """grid.h:50-51 in float32: m_aabb_min[axis] + vox * m_cell_wdh."""
        return (self.lo[axis] + np.asarray(k, np.int64).astype(F) * self.cw).astype(F)

    def lattice(self, r, axis, n, faces=True):
        """n lattice values of an axis: lo, hi, or ToPos(k) with 1 <= k <= dims - 1, in turn (an axis one cell thick
        has no interior plane: lo and hi only)."""
        d = self.dims[axis]
        k = r.integers(1, max(d, 2), n)
        plane = self.topos(axis, k)
        kind = np.arange(n) % 4 if faces else np.full(n, 2)
        if d < 2:
            kind = kind % 2
        return np.where(kind == 0, self.lo[axis], np.where(kind == 1, self.hi[axis], plane)).astype(F)

    def interior(self, r, n):
        p = (self.lo + self.ext * r.uniform(0.02, 0.98, (n, 3)).astype(F)).astype(F)
        return np.clip(p, self.lo, self.hi).astype(F)

    def exterior(self, r, n):
        """Uniform in 3x the box, outside the box."""
        p = (self.ctr + F(1.5) * self.ext * r.uniform(-1, 1, (8 * n + 64, 3)).astype(F)).astype(F)
        p = p[~((p >= self.lo) & (p <= self.hi)).all(1)]
        assert p.shape[0] >= n
        return np.ascontiguousarray(p[:n])


def rng(scene, fam):
    return np.random.Generator(np.random.PCG64([SEED, (SCENES + VARIANT_SCENES).index(scene), NAMES.index(fam)]))


def unit_dirs(r, n):
    d = r.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def tri_points(r, p0, p1, p2, n):
    """n random barycentric points of random triangles, float32."""
    i = r.integers(0, p0.shape[0], n)
    a, b = r.uniform(0, 1, n), r.uniform(0, 1, n)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a)[:, None], np.where(flip, 1 - b, b)[:, None]
    q = p0[i].astype(np.float64) * (1 - a - b) + p1[i].astype(np.float64) * a + p2[i].astype(np.float64) * b
    return q.astype(F)


def join(o, d):
    return np.ascontiguousarray(np.concatenate([np.asarray(o, F), np.asarray(d, F)], axis=1), F)


def zero_of(sign):
    return np.where(sign, F(-0.0), F(0.0)).astype(F)


# ------------------------------------------------------------------ the families
def family_a(scene, box, tri, cam_rays, cam_hit, cam_t):
    r = rng(scene, "A")
    idx = np.flatnonzero(cam_hit)
    assert idx.size >= 16, (scene, idx.size)
    pick = np.sort(r.choice(idx, 128, replace=idx.size < 128))
    o, d, t = cam_rays[pick, :3], cam_rays[pick, 3:], np.asarray(cam_t, F)[pick]
    p = (o + d * t[:, None]).astype(F)
    return join(np.repeat(p, 4, axis=0), unit_dirs(r, 512))


def family_b(scene, box, tri):
    r = rng(scene, "B")
    o = box.interior(r, 384)
    d = unit_dirs(r, 192)
    q = tri_points(r, *tri, 192)
    return join(o, np.concatenate([d, (q - o[192:]).astype(F)]))


def family_c(scene, box, tri):
    r = rng(scene, "C")
    o = box.exterior(r, 384)
    q = tri_points(r, *tri, 288)
    aimed = (q[:192] - o[:192]).astype(F)
    rand = unit_dirs(r, 96)
    away = (-(q[192:] - o[288:])).astype(F)
    return join(o, np.concatenate([aimed, rand, away]))


def family_d(scene, box, tri):
    n = 256
    r = rng(scene, "D")
    i = np.arange(n)
    d = unit_dirs(r, n)
    neg = r.integers(0, 2, (n, 3)).astype(bool)
    # rays 0-127: exact +-axis directions (the two other components +-0); 128-255: one or two zero components
    ax = r.integers(0, 3, n)
    nz = np.ones((n, 3), bool)                         # True where the component is zeroed
    nz[i[:128], ax[:128]] = False
    for k in range(128, n):
        nz[k] = False
        nz[k, r.permutation(3)[: 1 + k % 2]] = True
    d = np.where(nz, zero_of(neg), d).astype(F)
    d[i[:128], ax[:128]] = np.where(neg[i[:128], ax[:128]], F(-1), F(1))
    # origins: even rays on a line through a triangle point (o = q - L d), odd rays anywhere in 1.5x the box
    q = tri_points(r, *tri, n)
    L = (box.diag * r.uniform(0.05, 1.2, n).astype(F)).astype(F)
    dn = (d / np.abs(d).max(1, keepdims=True)).astype(F)
    o_line = (q - dn * L[:, None]).astype(F)
    o_any = (box.ctr + F(0.75) * box.ext * r.uniform(-1, 1, (n, 3)).astype(F)).astype(F)
    o = np.where((i % 2 == 0)[:, None], o_line, o_any).astype(F)
    # every fourth ray: the origin's coordinate on a zeroed axis exactly lo, hi or ToPos(k)
    for k in range(3, n, 4):
        a = int(np.flatnonzero(nz[k])[(k // 4) % int(nz[k].sum())])
        o[k, a] = box.lattice(r, a, 4)[(k // 4) % 4]
    assert (nz.sum(1) >= 1).all() and (nz.sum(1) <= 2).all() and (d[nz] == 0).all() and (d[~nz] != 0).all()
    return join(o, d)


def family_e(scene, box, tri):
    n = 384
    r = rng(scene, "E")
    i = np.arange(n)
    o = box.interior(r, n)
    nlat = 1 + i % 3                                   # one, two, three lattice coordinates
    first = r.integers(0, 3, n)                        # the first lattice axis; the others follow it cyclically
    lat = np.zeros((n, 3), bool)
    for a in range(3):
        vals = box.lattice(r, a, n)
        on = ((a - first) % 3) < nlat
        lat[:, a] = on
        o[on, a] = vals[on]
    kind = (i // 3) % 3                                # 0 +-diagonal, 1 +-axis, 2 aimed
    sg = np.where(r.integers(0, 2, (n, 3)) == 1, F(-1), F(1)).astype(F)
    axd = np.zeros((n, 3), F)
    ax = r.integers(0, 3, n)
    axd[i, ax] = sg[i, ax]
    aimed = (tri_points(r, *tri, n) - o).astype(F)
    d = np.where((kind == 0)[:, None], sg, np.where((kind == 1)[:, None], axd, aimed)).astype(F)
    # on the first lattice axis: a quarter exactly zero, half of the rest negative, half positive
    mode = (i // 9) % 8                                # 0, 1: zero (+0, -0); 2-4: negative; 5-7: positive
    c = d[i, first]
    mag = np.where(c == 0, F(1), np.abs(c)).astype(F)
    d[i, first] = np.where(mode == 0, F(0.0), np.where(mode == 1, F(-0.0), np.where(mode < 5, -mag, mag))).astype(F)
    dead = (d == 0).all(1)                             # an axis direction whose only component was zeroed
    d[dead, (first[dead] + 1) % 3] = sg[dead, (first[dead] + 1) % 3]
    assert not (d == 0).all(1).any()
    return join(o, d), lat


def family_f(scene, box, tri):
    r = rng(scene, "F")
    lo, hi = box.lo, box.hi
    corners = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] for k in range(8)], F)
    mids = []
    for a in range(3):                                 # the 12 edges: along axis a, the two others at lo / hi
        b, c = (a + 1) % 3, (a + 2) % 3
        for k in range(4):
            p = np.zeros(3, F)
            p[a] = box.ctr[a]
            p[b] = (hi if k & 1 else lo)[b]
            p[c] = (hi if k & 2 else lo)[c]
            mids.append(p)
    n3, n2 = 38, 38
    lat3 = np.stack([box.lattice(r, a, n3, faces=False) for a in range(3)], axis=1)
    lat2 = np.stack([box.lattice(r, a, n2, faces=False) for a in range(3)], axis=1)
    free = r.integers(0, 3, n2)
    lat2[np.arange(n2), free] = box.interior(r, n2)[np.arange(n2), free]
    targets = np.concatenate([corners, np.array(mids, F), lat3, lat2]).astype(F)
    assert targets.shape[0] == 96
    o = box.exterior(r, 96)
    part1 = join(o, (targets - o).astype(F))
    # displaced: o = p + 2^m s, d = -2^m s exactly, s in (+-1, +-1, +-1) / (+-1, +-1, 0); 2^m at least the box's extent
    p = np.stack([box.lattice(r, a, 96, faces=False) for a in range(3)], axis=1)
    s = np.where(r.integers(0, 2, (96, 3)) == 1, F(-1), F(1)).astype(F)
    flat = np.arange(96) % 2 == 1
    s[flat, r.integers(0, 3, 96)[flat]] = F(0)
    m = np.ceil(np.log2(float(box.ext.max()))) + (np.arange(96) // 2) % 3
    step = (s * np.exp2(m).astype(F)[:, None]).astype(F)
    o2 = (p + step).astype(F)
    assert not ((o2 >= lo) & (o2 <= hi)).all(1).any()
    return np.concatenate([part1, join(o2, -step)])


def family_g(scene, abc):
    r = rng(scene, "G")
    pick = r.choice(abc.shape[0], (len(G_FACTORS), 48), replace=False)
    fac = np.array(G_FACTORS, F)
    blocks, inter = [], []
    for k in range(len(G_FACTORS)):
        g = abc[pick[k, :24]].copy()
        g[:, 3:] = (g[:, 3:] * fac[k]).astype(F)
        blocks.append(g)
    tail = abc[pick[:, 24:].T.reshape(-1)].copy()       # ray j of the interleaved half has factor j % 9
    tail[:, 3:] = (tail[:, 3:] * fac[np.arange(tail.shape[0]) % len(G_FACTORS)][:, None]).astype(F)
    return np.concatenate(blocks + [tail])


def family_h(scene, box, tri):
    n = dict(FAMILIES)["H"]
    r = rng(scene, "H")
    dist = (np.array(H_DISTANCES, F)[np.arange(n) % 4] * box.diag).astype(F)
    o = (box.ctr + unit_dirs(r, n) * dist[:, None]).astype(F)
    q_tri = tri_points(r, *tri, n)
    q_box = box.interior(r, n)
    q = np.where((np.arange(n) // 4 % 2 == 0)[:, None], q_tri, q_box)
    q = (q + (F(3) * box.cw * r.normal(size=(n, 3))).astype(F)).astype(F)
    return join(o, (q - o).astype(F))


def build(scene, grid_meta, vertices, triangles, cam_rays, cam_hit, cam_t):
    """The scene's rays f32 [TOTAL, 6] and family E's lattice mask bool [384, 3].  grid_meta: HostScene.grid()'s;
    vertices, triangles: HostScene.mesh()'s; cam_rays [n, 6]: the reference's GenerateRay rays of CAM_FRAME;
    cam_hit, cam_t: the reference's closest hits for them."""
    box = Box(grid_meta)
    p = np.ascontiguousarray(np.asarray(vertices)[:, :3], F)
    idx = np.asarray(triangles)[:, :3].astype(np.int64)
    tri = (p[idx[:, 0]], p[idx[:, 1]], p[idx[:, 2]])
    a = family_a(scene, box, tri, np.asarray(cam_rays, F), np.asarray(cam_hit, bool), cam_t)
    b, c = family_b(scene, box, tri), family_c(scene, box, tri)
    e, lat = family_e(scene, box, tri)
    parts = [a, b, c, family_d(scene, box, tri), e, family_f(scene, box, tri),
             family_g(scene, np.concatenate([a, b, c])), family_h(scene, box, tri)]
    for (name, k), part in zip(FAMILIES, parts):
        assert part.shape == (k, 6) and part.dtype == F, (name, part.shape)
    return np.ascontiguousarray(np.concatenate(parts), F), lat


def lattice_values(box, axis):
    """Every float32 an E origin's lattice coordinate may hold on an axis: lo, hi and ToPos(1 .. dims - 1)."""
    return np.concatenate([[box.lo[axis], box.hi[axis]], box.topos(axis, np.arange(1, max(box.dims[axis], 1)))]).astype(F)


# ------------------------------------------------------------------ what the GPU calls must return
def expected_rec12(rec8):
    """The reference's 8-word records as rt_sample_rec words [n, 12] of the counting arm: hit, tri, voxel, steps,
    tests, t, u, v, and r = g = b = pad = 0."""
    rec8 = np.asarray(rec8, np.uint32)
    out = np.zeros((rec8.shape[0], 12), np.uint32)
    out[:, [0, 1, 5, 6, 7, 2, 3, 4]] = rec8
    return out


def expected_hits(rec8):
    """... and as rt_ray_hit words [n, 4]: tri, t, u, v (0xFFFFFFFF, 0, 0, 0 on a miss, as the records hold it)."""
    return np.ascontiguousarray(np.asarray(rec8, np.uint32)[:, 1:5])


def assert_words(got, want, float_cols, keep, what):
    """Word arrays [n, w] equal on the rows of `keep`, column by column; a NaN in a float column equals any NaN (x86
    writes the negative default NaN, gfx950 the positive one)."""
    got, want = np.array(got, np.uint32), np.array(want, np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for j in float_cols:
        for a in (got, want):
            a[np.isnan(a[:, j].view(F)), j] = 0x7FC00000
    rows = np.flatnonzero(keep)
    for j in range(got.shape[1]):
        bad = rows[got[rows, j] != want[rows, j]]
        assert bad.size == 0, (f"{what}: word {j} differs on {bad.size} rays; first ray {int(bad[0])}: "
                               f"got {got[bad[0]]}, the reference {want[bad[0]]}")


def intervals(rays, rec8, diag):
    """Per-ray (tmin, tmax) f32 [n, 2] around the reference's own t.  In units of t a length L is L / |d|:
    tmin cycles through -inf, 0 and 1e-4 diagonals; tmax of a hit ray through nextafter(t, 0), t, nextafter(t, +inf),
    2 t, t / 2 and +inf, of a miss ray through 0.05 diagonals, 0.5 diagonals and +inf."""
    n = rays.shape[0]
    i = np.arange(n)
    inf = F(np.inf)
    dl = np.sqrt((rays[:, 3:].astype(np.float64) ** 2).sum(1))
    unit = (float(diag) / dl).astype(F)                      # one diagonal, in units of t
    t = np.asarray(rec8, np.uint32)[:, 2].view(F)
    hit = np.asarray(rec8, np.uint32)[:, 0] == 1
    tmin = np.choose(i % 3, [np.full(n, -inf), np.zeros(n, F), (F(1e-4) * unit).astype(F)]).astype(F)
    on_hit = np.choose((i // 3) % 6, [np.nextafter(t, F(0)), t, np.nextafter(t, inf), (F(2) * t).astype(F),
                                      (t / F(2)).astype(F), np.full(n, inf)])
    on_miss = np.choose((i // 3) % 3, [(F(0.05) * unit).astype(F), (F(0.5) * unit).astype(F), np.full(n, inf)])
    return np.ascontiguousarray(np.stack([tmin, np.where(hit, on_hit, on_miss).astype(F)], axis=1), F)
