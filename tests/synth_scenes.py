"""Synthetic scenes that sit on the edges of the kernels' scene-dependent choices, shared by
oracle/gen_golden_synth.py (which pins them to the reference's own code), tests/test_oracle_synth.py,
tests/test_gpu_synth.py and tests/test_gpu_variants.py.  A plain module, not a conftest.

The ten shipped scenes all have rcp_safe = pack_ok = box_words = packed_cells = octant_words = 1 and
a 64-cell grid, so without these only k_render_lanes<MT, kVarAuto> is ever compared with anything.

Every mesh comes from a fixed seed through numpy's PCG64 and float32 arithmetic, so the generator
reproduces the committed .rtscene files byte for byte.
"""
import ctypes
import gzip
import hashlib
import json
import os

import numpy as np

from conftest import GOLD, load_package

rtm = load_package()
SYNTH = os.path.join(GOLD, "synth")
W, H, SPP = 62, 46, 4            # ragged 16-pixel tiles (4 x 3, the last column and row 14 wide)
# The first Hammersley sample is (-0.5, -0.5), not (0, 0) (rt_sample_table): a sample looks exactly down the
# camera axis only where pixel + offset = size / 2 on both axes (GenerateRay, camera.h:20), i.e. at ODD
# sizes with sample 0.  At 62 x 46 only one component vanishes (sample 1, offset (-0.25, 0), on row 23;
# sample 2, offset (0, -0.25), on column 31).  So the cases whose point is the axis ray are pinned at
# 63 x 47 as well, where pixel (32, 24) sample 0 has two exactly-zero direction components.
AXIS_FRAME = (63, 47, 4)
AXIS_PIXEL = (32, 24)            # (32 - 0.5) / 63 * 2 - 1 = 0 and (24 - 0.5) / 47 * 2 - 1 = 0
AXIS_CASES = ("fan_axis", "axis_x", "axis_y", "axis_z")
CAM_FRAME = (96, 54, 4)          # the seeded cameras' frame
BIG_FRAME = (1920, 1080, 2)      # 16,200 workgroups: above wg64_min_blocks and hf_min_blocks
WIDE_FRAME = (256, 144, 4)       # the wide-section test's frame: 2,304 work items (waves)
REC_WORDS = 12                   # rt_sample_rec
# fixture column (11-word refdriver_instr record) -> rt_sample_rec word
COLS = {"hit": (0, 0), "tri": (1, 1), "t": (2, 5), "u": (3, 6), "v": (4, 7), "r": (5, 8), "g": (6, 9), "b": (7, 10),
        "voxel": (8, 2), "steps": (9, 3), "tests": (10, 4)}
PRODUCT_COLS = ("hit", "tri", "voxel", "t", "u", "v", "r", "g", "b")   # the product kernels count no steps / tests
FLOAT_COLS = ("t", "u", "v", "r", "g", "b")
SENTINEL = 0x5A5A5A5A


# ------------------------------------------------------------------ meshes
def mesh_of(tris, zero_normals=()):
    """tris [nt, 3, 3] -> (vertices f32 [3 nt, 6], triangles u32 [nt, 6]).  Vertex and face normals are
    the normalised e1 x e2 (float32), (0, 1, 0) where that is not finite; the triangles listed in
    zero_normals get (0, 0, 0) vertex normals (the reference's Normalize then yields NaN colours)."""
    p = np.ascontiguousarray(tris, np.float32)
    nt = p.shape[0]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(np.float32)
    ln = np.sqrt((n * n).sum(1, dtype=np.float32), dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = (n / ln[:, None]).astype(np.float32)
    n[~np.isfinite(n).all(1)] = (0.0, 1.0, 0.0)
    v = np.zeros((nt * 3, 6), np.float32)
    v[:, :3] = p.reshape(-1, 3)
    v[:, 3:] = np.repeat(n, 3, axis=0)
    for i in zero_normals:
        v[3 * i:3 * i + 3, 3:] = 0.0
    t = np.zeros((nt, 6), np.uint32)
    t[:, :3] = np.arange(nt * 3, dtype=np.uint32).reshape(nt, 3)
    t[:, 3:] = n.view(np.uint32)
    return v, t


def anchors(lo=-1.0, hi=1.0):
    """Two small triangles in opposite corners: they fix the grid's box to [lo, hi]^3."""
    d = np.float32(0.02) * np.float32(hi - lo)
    a = np.array([[lo, lo, lo], [lo + d, lo, lo + d / 2], [lo + d / 2, lo + d, lo]], np.float32)
    b = np.array([[hi, hi, hi], [hi - d, hi, hi - d / 2], [hi - d / 2, hi - d, hi]], np.float32)
    return np.stack([a, b])


# the 64^3 grid over [-1, 1]^3 (+- the builder's 0.0001 pad): cell 32 spans about [0.0000, 0.0313]
STACK_LO, STACK_HI = 0.004, 0.027


def stack(n, seed):
    """n small triangles strictly inside one cell of the 64^3 grid, facing +z, z ascending with the index:
    from a camera on the +z side the nearest triangle is the LAST of the cell's list."""
    r = np.random.Generator(np.random.PCG64(seed))
    c = r.uniform(STACK_LO + 0.006, STACK_HI - 0.006, (n, 2)).astype(np.float32)
    ang = r.uniform(0.0, 2.0 * np.pi, n)
    rad = r.uniform(0.003, 0.006, (n, 3))
    z = np.linspace(STACK_LO, STACK_HI, n).astype(np.float32)
    tris = np.zeros((n, 3, 3), np.float32)
    for k in range(3):
        a = ang + 2.0 * np.pi * k / 3.0
        tris[:, k, 0] = c[:, 0] + (rad[:, k] * np.cos(a)).astype(np.float32)
        tris[:, k, 1] = c[:, 1] + (rad[:, k] * np.sin(a)).astype(np.float32)
        tris[:, k, 2] = z
    return np.concatenate([tris, anchors()])


def sparse(seed, n=60, size=0.3):
    """n random triangles of about `size` in [-1, 1]^3 plus the corner anchors: long empty runs."""
    r = np.random.Generator(np.random.PCG64(seed))
    c = r.uniform(-0.7, 0.7, (n, 1, 3))
    tris = np.clip(c + r.uniform(-size, size, (n, 3, 3)), -0.98, 0.98).astype(np.float32)
    return np.concatenate([tris, anchors()])


def fan(apex):
    """Eight triangles around a shared vertex, rim points at slightly different depths."""
    ax, ay, az = apex
    rim = [(ax + 0.5 * np.cos(k * np.pi / 4), ay + 0.5 * np.sin(k * np.pi / 4), az - 0.05 * (k % 3)) for k in range(8)]
    tris = [[apex, rim[k], rim[(k + 1) % 8]] for k in range(8)]
    return np.concatenate([np.array(tris, np.float32), anchors()])


def slab(seed, thin_axes, n=160, thick=0.02):
    """Random triangles spanning [-1, 1] on the other axes and [0, thick] on thin_axes (tilted, so none
    lies in a cell plane): dims 64 on the long axes, 1 on the thin ones."""
    r = np.random.Generator(np.random.PCG64(seed))
    c = r.uniform(-0.85, 0.85, (n, 1, 3))
    tris = np.clip(c + r.uniform(-0.15, 0.15, (n, 3, 3)), -1.0, 1.0)
    for a in thin_axes:
        tris[:, :, a] = r.uniform(0.0, thick, (n, 3))
    ends = np.array(tris[:2])
    for a in range(3):                     # the two ends of the long axes, so dims there are exactly 64
        if a not in thin_axes:
            ends[0, :, a] = (-1.0, -0.97, -0.98)
            ends[1, :, a] = (1.0, 0.97, 0.98)
    return np.concatenate([tris, ends]).astype(np.float32)


def degenerate(seed):
    """The sparse mesh with zero-area (collinear), all-equal-vertex and exactly duplicated triangles mixed in."""
    base = sparse(seed, n=80)
    extra = []
    for i in range(0, 24, 3):
        p = base[i]
        extra.append([p[0], (p[0] + p[1]) * np.float32(0.5), p[1]])     # collinear
        extra.append([p[2], p[2], p[2]])                               # a point
        extra.append(p.copy())                                         # duplicate of triangle i
    out = np.concatenate([base[:40], np.array(extra, np.float32), base[40:]])
    return out


# ------------------------------------------------------------------ meshes of tests/test_gpu_variants.py
def sheets(n, seed):
    """n large tilted triangles, each half of the [-1, 1]^2 square at its own height: on a grid_res = 16 grid
    every one overlaps a few hundred cells, so the grid holds about 150 references per triangle and a few
    hundred per cell -- num_refs in [2^20, 2^21) at n = 7000 with every cell under 2,048."""
    r = np.random.Generator(np.random.PCG64(seed))
    z = r.uniform(-0.95, 0.95, (n, 1)) + r.uniform(-0.04, 0.04, (n, 3))
    corners = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float64)
    tris = np.zeros((n, 3, 3))
    for i in range(n):
        k = i % 4
        tris[i, :, :2] = corners[[k, (k + 1) % 4, (k + 2) % 4]] * r.uniform(0.9, 1.0)
    tris[:, :, 2] = z
    return np.concatenate([tris.astype(np.float32), anchors()])


def ribbon(axis, seed, n=14):
    """Small triangles strung along `axis` from -1 to 1, within [0, 0.01] on the other two: with grid_res = R
    the grid is R cells long and 3 x 3 across."""
    r = np.random.Generator(np.random.PCG64(seed))
    tris = r.uniform(0.0, 0.01, (n, 3, 3))
    c = np.linspace(-0.95, 0.95, n)[:, None]
    tris[:, :, axis] = c + r.uniform(-0.04, 0.04, (n, 3))
    tris[0, :, axis] = (-1.0, -0.97, -0.99)
    tris[-1, :, axis] = (1.0, 0.97, 0.99)
    tris[0, 0, :] = np.where(np.arange(3) == axis, -1.0, 0.0)        # the box's two corners, exactly
    tris[-1, 0, :] = np.where(np.arange(3) == axis, 1.0, 0.01)
    return tris.astype(np.float32)


def big_grid_mesh(seed, res=512, ny=129, nz=128, n=40):
    """A sparse mesh whose grid_res = 512 grid is 512 x ny x nz cells: just over 2^23 of them at 129 x 128,
    the fewest with every axis <= 512 (so pack_ok holds and only the octant words are missing)."""
    r = np.random.Generator(np.random.PCG64(seed))
    cw = 2.0002 / res
    # (y and z start at 0: the builder seeds the box's maximum with float::min(), so a negative one becomes 0)
    hi = np.array([1.0, (ny - 0.5) * cw, (nz - 0.5) * cw])
    lo = np.array([-1.0, 0.0, 0.0])
    c = lo + (hi - lo) * r.uniform(0.1, 0.9, (n, 1, 3))
    tris = c + r.uniform(-0.04, 0.04, (n, 3, 3))
    tris[0, 0] = lo
    tris[1, 0] = hi
    return np.clip(tris, lo, hi).astype(np.float32)


# ------------------------------------------------------------------ cameras
def axis_cam(axis, sign, eye):
    """The view matrix (rows: right, up, back, eye -- Matrix44f as Scene::GetCameraParameters returns it)
    of a camera at eye looking exactly along sign * axis: every basis component is 0 or +-1, so the
    centre ray has two exactly-zero direction components."""
    back = np.zeros(3, np.float32)
    back[axis] = -sign
    up = np.array([0, 0, -sign] if axis == 1 else [0, 1, 0], np.float32)
    right = np.cross(up, back).astype(np.float32)
    m = np.eye(4, dtype=np.float32)
    m[0, :3], m[1, :3], m[2, :3], m[3, :3] = right, up, back, np.asarray(eye, np.float32)
    return m.reshape(16)


def look(eye, at):
    return rtm.look_at(np.asarray(eye, np.float32), np.asarray(at, np.float32))


# ------------------------------------------------------------------ the A1 cases
def grid_of(tris, grid_res=64):
    """The builder's grid for a mesh (no camera needed): meta dict of HostScene.grid()."""
    v, t = mesh_of(tris)
    hs = rtm.HostScene.from_mesh(v, t, 45.0, np.eye(4, dtype=np.float32).reshape(16), grid_res=grid_res)
    try:
        return hs.grid()[0]
    finally:
        hs.close()


def cases():
    """{name: dict(tris, cam, fov, all_miss, zero_normals, dims)}: one .rtscene per entry (a view is part
    of the file: save() writes the camera from_mesh was given)."""
    out = {}

    def add(name, tris, cam, fov=45.0, all_miss=False, zero_normals=(), dims=(64, 64, 64)):
        out[name] = dict(tris=np.asarray(tris, np.float32), cam=np.asarray(cam, np.float32), fov=float(fov),
                         all_miss=all_miss, zero_normals=tuple(zero_normals), dims=None if dims is None else list(dims))

    mid = 0.5 * (STACK_LO + STACK_HI)
    add("stack1500", stack(1500, 11), axis_cam(2, -1, (mid, mid, 1.5)), fov=2.0)
    add("stack2100", stack(2100, 12), axis_cam(2, -1, (mid, mid, 1.5)), fov=2.0)
    add("fan_axis", fan((0.2, 0.1, 0.0)), axis_cam(2, -1, (0.2, 0.1, 3.0)))
    sp = sparse(21)
    add("axis_x", sp, axis_cam(0, -1, (3.0, 0.013, -0.02)))
    add("axis_y", sp, axis_cam(1, 1, (0.02, -3.0, 0.01)))
    add("axis_z", sp, axis_cam(2, -1, (-0.015, 0.03, 3.0)))
    g = grid_of(sp)
    add("eye_on_face", sp, axis_cam(2, -1, (0.1, 0.05, g["aabb_max"][2])))
    plane = np.float32(g["aabb_min"][0] + np.float32(40.0) * g["cell_wdh"])       # as grid.cpp:101 forms it
    add("eye_on_plane", sp, look((plane, 0.21, 2.5), (plane, -0.1, 0.0)))
    dense = sparse(22, n=200)
    add("inside", dense, look((0.11, -0.07, 0.23), (-0.6, 0.3, -0.8)))
    add("away", sp, axis_cam(2, 1, (0.0, 0.0, 3.0)), all_miss=True)
    fl = slab(23, (2,))
    add("flat_front", fl, look((0.1, 0.1, 3.0), (0.0, 0.05, 0.0)), dims=(64, 64, 1))
    add("flat_inplane", fl, axis_cam(0, -1, (1.2, 0.0, 0.01)), dims=(64, 64, 1))
    for a, name in enumerate(("thin_x", "thin_y", "thin_z")):
        thin = tuple(k for k in range(3) if k != a)
        eye = np.full(3, 0.01, np.float32)
        eye[a] = 0.1
        eye[thin[0]] = 0.6
        dims = [1, 1, 1]
        dims[a] = 64
        at = np.full(3, 0.01, np.float32)
        at[a] = -0.1
        add(name, slab(24 + a, thin, n=120), look(eye, at), fov=30.0, dims=dims)
    neg = sparse(27)
    neg[:-2] = neg[:-2] - np.float32(2.0)
    neg = neg[:-2]                                     # no anchors: the mesh alone, all coordinates < 0
    add("negative_octant", neg, look((-2.0, -2.1, 1.5), (-2.0, -2.0, -2.0)), dims=None)
    add("scale_1500", sp * np.float32(1500.0), axis_cam(2, -1, (30.0, -45.0, 4500.0)))
    add("scale_2e-2", sp * np.float32(2e-2), axis_cam(2, -1, (4e-4, -6e-4, 6e-2)))
    add("degenerate", degenerate(28), look((0.3, 0.2, 3.0), (0.0, 0.0, 0.0)))
    add("zero_normals", sp, look((-0.4, 0.3, 3.0), (0.0, 0.0, 0.0)), zero_normals=range(0, 60, 7))
    add("far_eye", sp, look((120.0, 90.0, 259.0), (0.0, 0.0, 0.0)), fov=1.0)
    return out


BARY_ALT = ("stack1500", "fan_axis", "inside")         # A2: second triangle test, brute force, march
BIG = ("stack1500", "inside")                          # A2: 1920x1080x2 frames
ALT_CROPS = {"brute": (23, 15, 16, 16), "march": (27, 19, 8, 8)}     # (x0, y0, w, h) around the frame centre


def build_host(case, grid_res=64):
    v, t = mesh_of(case["tris"], case["zero_normals"])
    return rtm.HostScene.from_mesh(v, t, case["fov"], case["cam"], grid_res=grid_res)


# ------------------------------------------------------------------ A3: seeded cameras
CAM_SCENES = ("scene1", "scene8", "inside")
CAM_SEED = 31


def seeded_cameras(lo, hi, fov):
    """Sixteen (name, cam16, fov) for a grid box [lo, hi]: the six exact axis directions from outside, two
    eyes inside the grid, two exactly on a grid face, one looking away, five random look-ats from one seed."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    ctr, ext = (lo + hi) * np.float32(0.5), hi - lo
    r = np.random.Generator(np.random.PCG64(CAM_SEED))
    out = []
    for axis in range(3):
        for sign in (-1, 1):
            eye = ctr + np.float32(0.07) * ext * r.uniform(-1, 1, 3).astype(np.float32)
            eye[axis] = ctr[axis] - sign * np.float32(1.6) * ext.max()
            out.append((f"axis{'xyz'[axis]}{'+' if sign > 0 else '-'}", axis_cam(axis, sign, eye), fov))
    for k in range(2):
        eye = ctr + np.float32(0.3) * ext * r.uniform(-1, 1, 3).astype(np.float32)
        at = ctr + np.float32(0.5) * ext * r.uniform(-1, 1, 3).astype(np.float32)
        out.append((f"inside{k}", look(eye, at), fov))
    for k, (axis, side) in enumerate(((0, hi), (1, lo))):
        eye = ctr + np.float32(0.2) * ext * r.uniform(-1, 1, 3).astype(np.float32)
        eye[axis] = side[axis]
        out.append((f"face{k}", look(eye, ctr), fov))
    eye = ctr + np.array([0.0, 0.0, 2.0], np.float32) * ext.max()
    out.append(("away", axis_cam(2, 1, eye), fov))
    for k in range(5):
        d = r.normal(size=3)
        eye = ctr + (d / np.linalg.norm(d) * r.uniform(0.9, 2.2)).astype(np.float32) * ext.max()
        at = ctr + np.float32(0.2) * ext * r.uniform(-1, 1, 3).astype(np.float32)
        out.append((f"random{k}", look(eye, at), fov))
    return out


# ------------------------------------------------------------------ fixtures
def meta():
    with open(os.path.join(GOLD, "synth.json")) as f:
        return json.load(f)


def gunzip_scene(name, tmp_path):
    """tests/golden/synth/<name>.rtscene.gz -> a plain file under tmp_path; its path."""
    out = os.path.join(str(tmp_path), name + ".rtscene")
    if not os.path.exists(out):
        with gzip.open(os.path.join(SYNTH, name + ".rtscene.gz"), "rb") as f, open(out, "wb") as o:
            o.write(f.read())
    return out


def scene_file(e, tmp_path):
    """The scene a fixture entry renders: a shipped one ("scene1") or a synthetic one."""
    if e["scene"].startswith("scene") and e["scene"][5:].isdigit():
        return rtm.scene_path(int(e["scene"][5:]))
    return gunzip_scene(e["scene"], tmp_path)


def read_synth(name, dtype):
    with gzip.open(os.path.join(SYNTH, name), "rb") as f:
        return np.frombuffer(f.read(), dtype=dtype)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits_f32(hexes):
    return np.array([int(x, 16) for x in hexes], np.uint32).view(np.float32)


def rec_shas(rec11, cols=("hit_tri", "tuv", "voxel", "rgb", "steps", "tests")):
    """Column SHA-256s of 11-word reference records, the names of oracle/gen_golden.py rec_shas."""
    sel = {"hit_tri": lambda: np.where(rec11[:, 0] == 1, rec11[:, 1], np.uint32(0xFFFFFFFF)).astype("<u4"),
           "tuv": lambda: rec11[:, 2:5], "voxel": lambda: rec11[:, 8], "rgb": lambda: rec11[:, 5:8],
           "steps": lambda: rec11[:, 9], "tests": lambda: rec11[:, 10]}
    return {f"{c}_sha256": sha(sel[c]()) for c in cols}


def to_rec11(rec12):
    """rt_sample_rec / orc_rec words [n, 12] -> the reference's 11-word order; t, u, v are 0 on a miss there."""
    rec12 = np.ascontiguousarray(rec12).view(np.uint32).reshape(-1, REC_WORDS)
    out = np.zeros((rec12.shape[0], 11), np.uint32)
    for _, (j, w) in COLS.items():
        out[:, j] = rec12[:, w]
    return out


def nan_canonical(words):
    """u32 words of floats with every NaN replaced by one pattern: x86 gives the negative default NaN,
    gfx950 the positive one (conftest.nan_equal_bits), so columns that may hold NaN are hashed and compared
    through this."""
    w = np.array(words, np.uint32)
    w[np.isnan(w.view(np.float32))] = 0x7FC00000
    return w


def check_rec11(got11, e, cols=tuple(COLS), what=""):
    """got11 [n, 11] against fixture entry e: per column against the stored array when the entry has one
    (a mismatch is then printed per sample), else against the column SHA-256s.  NaN (zero_normals) compares
    equal to NaN whatever its payload."""
    if e.get("rec"):
        ref = read_synth(e["rec"], "<u4").reshape(-1, 11)
        assert got11.shape == ref.shape, (what, got11.shape, ref.shape)
        for c in cols:
            j = COLS[c][0]
            a, b = got11[:, j], ref[:, j]
            if c in FLOAT_COLS:
                a, b = nan_canonical(a), nan_canonical(b)
            np.testing.assert_array_equal(a, b, err_msg=f"{what} {e['name']} column {c}")
        return
    groups = {"hit_tri": ("hit", "tri"), "tuv": ("t", "u", "v"), "voxel": ("voxel",), "rgb": ("r", "g", "b"),
              "steps": ("steps",), "tests": ("tests",)}
    g = got11.copy()
    g[:, 2:8] = nan_canonical(g[:, 2:8])
    got = rec_shas(g, [k for k, v in groups.items() if all(c in cols for c in v)])
    bad = [k for k, v in got.items() if e["nan_canonical_shas"][k] != v]
    assert not bad, (what, e["name"], bad)


def check_alt(got, exp, mode, what):
    """Records of the brute-force / ray-march intersectors (rt_sample_rec layout) against the reference's
    alt-samples records (conftest.ALT_REC_DTYPE), as tests/test_gpu_alt.py compares them."""
    np.testing.assert_array_equal(got["hit"], exp["hit"], err_msg=what)
    np.testing.assert_array_equal(np.where(got["hit"] == 1, got["tri"], np.uint32(0xFFFFFFFF)), exp["tri"], err_msg=what)
    for k in ("t", "u", "v", "r", "g", "b"):
        np.testing.assert_array_equal(nan_canonical(got[k].view(np.uint32)), nan_canonical(exp[k].view(np.uint32)),
                                      err_msg=f"{what} {k}")
    if mode == "march":
        np.testing.assert_array_equal(got["steps"], exp["steps"], err_msg=what)


def camera_box(scene, golden_scenes, m):
    """(aabb_min, aabb_max) of the grid the seeded cameras of `scene` are placed around."""
    g = golden_scenes[scene[5:]] if scene.startswith("scene") else m["cases"][scene]
    return bits_f32(g["aabb_min_bits"]), bits_f32(g["aabb_max_bits"])


class OracleScene:
    """The CPU restatement (oracle/liboracle_tracer.so) on a scene FILE (conftest.Oracle takes scene ids)."""

    def __init__(self, oracle, path):
        self.L = oracle.L
        self.h = ctypes.c_void_p(self.L.orc_scene_load(path.encode()))
        assert self.h, f"oracle failed to load {path}"

    def records(self, Wd, Ht, spp, rect=None, tri_test=0):
        x0, y0, w, h = rect or (0, 0, Wd, Ht)
        out = np.zeros(w * h * spp, rtm.SAMPLE_REC_DTYPE)
        assert self.L.orc_trace_samples(self.h, Wd, Ht, spp, tri_test, x0, y0, w, h, ctypes.c_void_p(out.ctypes.data)) == 0
        return out

    def render(self, Wd, Ht, spp, tri_test=0, cam=None, fov=None):
        """(frame [H, W] u32, hit ids [W H spp] u32); cam / fov: another view (orc_render_cam)."""
        out, hid = np.zeros(Wd * Ht, np.uint32), np.zeros(Wd * Ht * spp, np.uint32)
        if cam is None:
            sec = ctypes.c_double()
            rc = self.L.orc_render(self.h, Wd, Ht, spp, tri_test, 0, ctypes.c_void_p(out.ctypes.data),
                                   ctypes.c_void_p(hid.ctypes.data), ctypes.byref(sec))
        else:
            c = np.ascontiguousarray(cam, np.float32)
            rc = self.L.orc_render_cam(self.h, Wd, Ht, spp, ctypes.c_void_p(c.ctypes.data), float(fov),
                                       ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(hid.ctypes.data))
        assert rc == 0
        return out.reshape(Ht, Wd), hid

    def close(self):
        if self.h:
            self.L.orc_scene_free(self.h)
            self.h = None
