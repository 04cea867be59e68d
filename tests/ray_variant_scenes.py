"""The scenes that reach the ray, occlusion and AO kernels' other instantiations, and their fixtures
(tests/golden/ray_variants), shared by oracle/gen_golden_ray_variants.py, tests/test_ray_variants_cpu.py,
tests/test_gpu_ray_variants.py and tests/test_gpu_variants.py (CallerBuilt).  A plain module, not a conftest.

rt_trace_rays_device, rt_occluded_rays_device and rt_render_ao_device each ship four instantiations, picked by
scene_traversal_bits() (rt_launch.hip) from rt_scene_info.  The scenes of tests/ray_sets.py all have
rcp_safe = pack_ok = 1 and box words (stack2100: no cell words at all).  These seven do not:

  name              mesh, grid                                          rt_scene_info               kernel variant
  ribbon_[xyz]513   S.ribbon(axis, 50 + axis), 513 x 3 x 3 cells         pack_ok 0, packed_cells 1,  kRaysBase | kVarFastRcp over the
                                                                        rcp_safe 1                  cell words (the distance-skip walk,
                                                                                                    RT_DDA_ADVANCE_ADD); sort shift 1
  ribbon_z512       the same mesh at 512                                pack_ok 1, box_words 1      the packable side: kRaysBox at the
                                                                                                    9-bit z count of a box word; shift 0
  sheets16          S.sheets(7000, 41), 16^3 cells                      packed_cells 1, box_words   kRaysBase | kVarFastRcp; reference
                                                                        0, rcp_safe 1, num_refs in  indices of 2^20 and more in the cell
                                                                        [2^20, 2^21)                words' 21-bit start field
  huge_axis_z       CallerBuilt(axis_z): a triangle with edges of 2^62  rcp_safe 0, box_words 1,    kRaysBase | kRaysBox: the exact
                                                                        pack_ok 1                   reciprocal inside the box-run walk
  huge_stack2100    CallerBuilt(stack2100)                              rcp_safe 0, packed_cells 0  kRaysBase: ... over the plain CSR walk

The meshes come from their seeds at test time; ray_variants.json carries the SHA-256 of each scene's vertex and
triangle arrays, and a mismatch fails.  The rays are ray_sets.build()'s eight families (2,744 per scene, the last wave
partial), committed.  Expected records: the reference's own Grid::Intersect for the ribbons and sheets16
(`refdriver_instr rays <scene> <in> <out> <grid_res>`); for the two huge scenes, whose grids the reference cannot build
(the appended triangle is listed by hand), tests/occlusion_ref.py's walk over CallerBuilt's arrays, with the ray/triangle
half anchored to the reference: `refdriver tri` answers every (ray, appended triangle) pair (huge_tri.out.gz).
"""
import ctypes
import gzip
import json
import os

import numpy as np

import occlusion_ref as R
import ray_sets as RS
import synth_scenes as S
from conftest import GOLD, load_package

rtm = load_package()
DIR = os.path.join(GOLD, "ray_variants")
SCENES = RS.VARIANT_SCENES
RIBBONS = ("ribbon_x513", "ribbon_y513", "ribbon_z513", "ribbon_z512")
REFERENCE_SCENES = RIBBONS + ("sheets16",)           # records: the reference's Grid::Intersect
HUGE_SCENES = ("huge_axis_z", "huge_stack2100")      # records: occlusion_ref.walk over CallerBuilt's arrays
GRID_RES = {"ribbon_x513": 513, "ribbon_y513": 513, "ribbon_z513": 513, "ribbon_z512": 512, "sheets16": 16}
# rt_scene_info, asserted before anything is compared: the kernel variant is a pure function of these
INFO = {"ribbon_x513": dict(pack_ok=0, packed_cells=1, rcp_safe=1),
        "ribbon_y513": dict(pack_ok=0, packed_cells=1, rcp_safe=1),
        "ribbon_z513": dict(pack_ok=0, packed_cells=1, rcp_safe=1),
        "ribbon_z512": dict(pack_ok=1, box_words=1),
        "sheets16": dict(packed_cells=1, box_words=0, rcp_safe=1),
        "huge_axis_z": dict(rcp_safe=0, box_words=1, pack_ok=1),
        "huge_stack2100": dict(rcp_safe=0, packed_cells=0)}
WAIVED = (("sheets16", "B"),)                        # every interior ray hits one of 7,000 sheets
MIN_BIG_TRI_HITS = 100                               # closest hits on the appended triangle, per huge scene
MIN_NONFINITE_UV = {"huge_axis_z": 32}               # pairs IntersectRayTri accepts with a non-finite u or v
MAX_FILE = 100_000
AO_FRAME = (62, 46, 4)
assert RS.CAM_FRAME == AO_FRAME


# ------------------------------------------------------------------ B5's caller-built scene
class CallerBuilt:
    """A caller-built rt_scene_desc, which rt_scene_create accepts (it validates indices and offsets only):
    a host scene's arrays plus one triangle with edges of 2^62, listed by hand at the end of some cells' lists.
    Has what GpuScene and VScene use of a HostScene: desc(), cam, fov, save()."""

    def __init__(self, hs, layer=20, lo=20, hi=45, big=2.0 ** 61):
        v, t = hs.mesh()
        g, offs, refs = hs.grid()
        self.g = g
        nv, nt = v.shape[0], t.shape[0]
        z = np.float32(g["aabb_min"][2] + np.float32(layer + 0.5) * g["cell_wdh"])
        big = np.float32(big)
        # big = 2^61: e1 = (2^62, 0, 0), e2 = (2^61, 2^62, 0): |e1|_1 |e2|_1 = 1.5 * 2^124 >= 2^120; the plane z = const
        # crosses every listed cell, behind the scene's own triangles as the -z cameras see them
        pts = np.array([[-big, -big, z], [big, -big, z], [0.0, big, z]], np.float32)
        ev = np.zeros((3, 6), np.float32)
        ev[:, :3], ev[:, 5] = pts, 1.0
        et = np.zeros((1, 6), np.uint32)
        et[0, :3] = (nv, nv + 1, nv + 2)
        et[0, 5] = np.float32(1.0).view(np.uint32)
        self.v = np.ascontiguousarray(np.concatenate([v, ev]))
        self.t = np.ascontiguousarray(np.concatenate([t, et]))
        dx, dy, dz = g["dims"]
        xs, ys = np.meshgrid(np.arange(lo, hi), np.arange(lo, hi))
        cells = np.sort((xs + layer * dx + ys * dx * dz).reshape(-1)).astype(np.int64)        # grid.h:41-42
        add = np.zeros(offs.size - 1, np.int64)
        add[cells] = 1
        self.refs = np.ascontiguousarray(np.insert(refs, offs[cells + 1].astype(np.int64), nt).astype(np.uint32))
        self.offs = np.ascontiguousarray(np.concatenate([[0], np.cumsum(np.diff(offs.astype(np.int64)) + add)])
                                         .astype(np.uint32))
        self.listed = cells.size
        self.cam, self.fov = hs.cam.copy(), hs.fov

    def desc(self):
        d = rtm.SceneDesc()
        d.num_vertices, d.num_triangles = self.v.shape[0], self.t.shape[0]
        d.vertices = self.v.ctypes.data_as(ctypes.POINTER(rtm.Vertex))
        d.triangles = self.t.ctypes.data_as(ctypes.POINTER(rtm.Triangle))
        for a in range(3):
            d.grid.dims[a] = int(self.g["dims"][a])
            d.grid.aabb_min[a] = float(self.g["aabb_min"][a])
            d.grid.aabb_max[a] = float(self.g["aabb_max"][a])
        d.grid.cell_wdh, d.grid.inv_cell_wdh = float(self.g["cell_wdh"]), float(self.g["inv_cell_wdh"])
        d.grid.cell_offsets = self.offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        d.grid.cell_tris = self.refs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        return d


# ------------------------------------------------------------------ the seven scenes
def ribbon_camera(axis):
    """The second (oblique, fov 45) view of test_gpu_variants.test_b3_pack_ok_boundary."""
    thin = [k for k in range(3) if k != axis]
    eye = np.full(3, 0.005, np.float32)
    eye[axis] = 0.3
    eye[thin[0]] = 0.12
    at = eye.copy()
    at[thin[0]] = 0.0
    at[axis] = 0.25
    return S.look(eye, at)


class Scene:
    """One scene, regenerated: .host is what rtm.GpuScene takes (a HostScene, or a CallerBuilt), .ref the restatement's
    RefScene over the same arrays, .gm the grid meta, .v / .t the mesh as the device gets it, .ray_mesh the mesh
    ray_sets.build() aims at (the huge scenes: without the appended triangle, whose points lie 2^61 away), .big the
    appended triangle's index (None elsewhere), .num_refs the grid's reference count."""

    def __init__(self, name, tmp_path):
        self.name, self.big, self._hs = name, None, None
        if name in GRID_RES:
            if name in RIBBONS:
                axis = "xyz".index(name[7])
                tris, cam = S.ribbon(axis, 50 + axis), ribbon_camera(axis)
            else:
                tris, cam = S.sheets(7000, 41), S.look((2.5, 1.8, 3.0), (0.0, 0.0, 0.0))
            v, t = S.mesh_of(tris)
            hs = rtm.HostScene.from_mesh(v, t, 45.0, cam, grid_res=GRID_RES[name])
            self.host = self._hs = hs
            self.gm, offs, refs = hs.grid()
            self.v, self.t = hs.mesh()
            self.ray_mesh = (self.v, self.t)
        else:
            hs = S.build_host(S.cases()["axis_z"]) if name == "huge_axis_z" else \
                rtm.HostScene.load(S.gunzip_scene("stack2100", tmp_path))
            try:
                cb = CallerBuilt(hs)
                self.ray_mesh = hs.mesh()
            finally:
                hs.close()
            self.host, self.gm, offs, refs, self.v, self.t = cb, cb.g, cb.offs, cb.refs, cb.v, cb.t
            self.big = cb.t.shape[0] - 1
        self.num_refs = int(offs[-1])
        self.ref = R.RefScene(self.gm, offs, refs, self.v, self.t)
        self.cam, self.fov = np.asarray(self.host.cam, np.float32).copy(), float(self.host.fov)

    def mesh_shas(self):
        return {"vertices_sha256": RS.sha256(np.ascontiguousarray(self.v, "<f4").tobytes()),
                "triangles_sha256": RS.sha256(np.ascontiguousarray(self.t, "<u4").tobytes())}

    def check_static(self):
        """What the scene must be before a GPU exists: the grid's dims and reference count."""
        d = [int(x) for x in self.gm["dims"]]
        if self.name in RIBBONS:
            axis, want = "xyz".index(self.name[7]), [3, 3, 3]
            want[axis] = GRID_RES[self.name]
            assert d == want, (self.name, d)
        if self.name == "sheets16":
            assert (1 << 20) <= self.num_refs < (1 << 21), self.num_refs

    def save(self, path):
        """The .rtscene the reference drivers read (the ribbons and sheets16 only)."""
        self._hs.save(path)

    def big_pairs(self, rays):
        """Every ray paired with the appended triangle: f32 [n, 15] (o, d, v0, v1, v2), `refdriver tri`'s input."""
        k = self.big
        tri = np.concatenate([self.ref.v0[k], self.ref.v1[k], self.ref.v2[k]]).astype(np.float32)
        return np.ascontiguousarray(np.concatenate([rays, np.tile(tri, (rays.shape[0], 1))], axis=1), np.float32)

    def close(self):
        if self._hs is not None:
            self._hs.close()
            self._hs = None


def assert_info(name, info):
    """rt_scene_info against INFO[name] (GpuScene.info()); returns the observed values of the five properties."""
    seen = {k: int(info[k]) for k in ("rcp_safe", "pack_ok", "box_words", "packed_cells", "octant_words", "max_cell_refs")}
    print(f"{name}: rt_scene_info {seen}")
    assert {k: seen[k] for k in INFO[name]} == INFO[name], (name, seen)
    return seen


# ------------------------------------------------------------------ fixtures
def meta():
    with open(os.path.join(DIR, "ray_variants.json")) as f:
        return json.load(f)


def read_fixture(name):
    with gzip.open(os.path.join(DIR, name), "rb") as f:
        return f.read()


def load(scene):
    """(rays f32 [n, 6], records u32 [n, 8]) of a scene, as committed."""
    rays = np.frombuffer(read_fixture(scene + ".rays.gz"), "<f4").reshape(-1, 6)
    rec = np.frombuffer(read_fixture(scene + ".rec.gz"), "<u4").reshape(-1, 8)
    assert rays.shape[0] == rec.shape[0] == RS.TOTAL, (scene, rays.shape, rec.shape)
    return rays, rec


def load_huge_tri():
    """{scene: u32 [n, 4]}: `refdriver tri`'s hit, t, u, v for every ray of a huge scene against its appended triangle."""
    a = np.frombuffer(read_fixture("huge_tri.out.gz"), "<u4").reshape(len(HUGE_SCENES), RS.TOTAL, 4)
    return {s: a[i] for i, s in enumerate(HUGE_SCENES)}


def check_non_vacuity(name, counts):
    """ray_sets' per-scene conditions on one scene's {family: [hits, misses]} (no across-scene conditions: a ribbon is
    hit by 2 of the 200 far rays).  Returns the list of failures."""
    bad = []
    h, m = sum(v[0] for v in counts.values()), sum(v[1] for v in counts.values())
    if min(h, m) < RS.MIN_SHARE * (h + m):
        bad.append((name, "all", h, m))
    for fam, k in RS.MIN_PER_SCENE.items():
        if min(counts[fam]) < k and (name, fam) not in WAIVED:
            bad.append((name, fam, counts[fam]))
    return bad


def rec8(res):
    """occlusion_ref's closest-mode result as the 8-word record of `refdriver rays`."""
    return np.ascontiguousarray(R.rec11(res)[:, [0, 1, 2, 3, 4, 8, 9, 10]])
