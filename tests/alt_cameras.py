"""The brute-force and ray-march intersectors of rt_render_frame_device / rt_trace_samples under odd cameras, odd eyes
and degenerate meshes, shared by oracle/gen_golden_alt_cameras.py (which pins the cases to the reference's own code),
tests/test_alt_cameras_cpu.py and tests/test_gpu_alt_cameras.py.  A plain module, not a conftest.

Three groups of cases (specs()):

  A1  scenes `scene1`, `inside`, `stack1500` under every factor of camera_matrices.factors(), `scene8` under six of
      them, and `scene1` x `scale_3` at 3 and 5 samples a pixel (the pixel loop);
  A2  `scene1` and `inside` from ten eyes (inside the vertex box, on a vertex, either side of min_dist off a triangle,
      on a face and a corner of the box, just outside a face, 1,024 and 2^20 box diagonals away), march only;
  A3  meshes whose Morton-first records have NaN distances (a point triangle, an (a, a, b) triangle, a whole first
      block of them, nothing else), synth_scenes.degenerate, meshes of exactly 1 ... 1,025 triangles around the block
      size of 32, and a floor of half-extent 2,047 seen from 0.0012 below it (margin = 1e-5 scene_scale is twenty
      times min_dist there).  Grid::Grid pads the vertex box by 0.0001 and aborts when that is absorbed, from 2,048 on:
      the floor of half-extent 4,096 exists for the stop checker of tests/test_alt_cameras_cpu.py only.

A brute case is a whole frame plus its records; a march case a small frame plus the records of one window of a larger
one.  The fixture (tests/golden/alt_cameras.json) holds, per case, the camera's bits and the reference's SHA-256 of the
frame and of every record column, the hit count and the sum of the march steps.  Float columns are hashed with every
NaN replaced by one pattern (synth_scenes.nan_canonical).  No sample is left out of any comparison.
"""
import ctypes
import hashlib
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import camera_matrices as C
import distance_ref as D
import synth_scenes as S
from conftest import GOLD, ISECT, load_package

rtm = load_package()
F = np.float32
FIXTURE = os.path.join(GOLD, "alt_cameras.json")
NOTRI = 0xFFFFFFFF
SENTINEL = 0x5A5A5A5A
MARCH_STEPS = 128                        # renderer.cpp:30 / kMarchSteps
FULL = C.CAM_FRAME                       # 96 x 54 x 4: the brute frame, and the frame the march windows are cut from
MARCH_FRAME = (48, 27, 1)
# (x0, y0) of the 16 x 8 window of FULL per scene: under the scene's own camera it holds hits and misses
# (oracle/gen_golden_alt_cameras.py checks that before it writes anything)
WINDOW = {"scene1": (8, 20), "inside": (20, 22), "stack1500": (24, 20), "nan_first_point": (40, 20),
          "nan_first_pair": (40, 20), "nan_block0": (40, 20), "nan_only": (40, 20), "degenerate": (40, 20),
          "floor2047": (40, 30)}
A1_SCENES = ("scene1", "inside", "stack1500")
SCENE8_FACTORS = ("identity", "scale_2^-1", "scale_2^1", "scale_3", C.S1024, "shear")
SCENE8_MARCH = (44, 23, 8, 8)            # windows of FULL around the frame centre
SCENE8_BRUTE = (40, 19, 16, 16)
A2_SCENES = ("scene1", "inside")
A2_FACTORS = ("identity", "scale_2^4")
FAR_EYES = ("far_1024", "far_2^20")
BLOCK_SIZES = (1, 31, 32, 33, 64, 65, 1025)
FLOOR_HALF = 2047.0                      # the largest whole half-extent whose 0.0001 pad survives in float32
FLOOR_FACTORS = ("identity", C.S1024, "scale_2^20")
MESH_CAM_EYE, MESH_CAM_AT, MESH_FOV = (0.3, 0.2, 3.0), (0.0, 0.0, 0.0), 45.0
COLUMNS = {"march": ("hit", "steps", "t", "rgb"), "brute": ("hit", "steps", "t", "rgb", "tri", "u", "v")}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------ meshes
def nan_point(base, k=0):
    """A point of cell (0, 0, 0) of the 1,024^3 Morton lattice over base's vertex box, off its corner."""
    v = base.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    return (lo + F(2.0 ** -12) * F(1.0 + k / 64.0) * (hi - lo)).astype(F)


def floor(half):
    """Two triangles: the square [-half, half]^2 at y = 0."""
    h = F(half)
    return np.array([[[-h, 0, -h], [h, 0, -h], [h, 0, h]], [[-h, 0, -h], [h, 0, h], [-h, 0, h]]], F)


def meshes():
    """{name: tris f32 [nt, 3, 3]} of the A3 cases."""
    base = S.sparse(7, n=30)
    a = nan_point(base)
    b = (a + F(2.0 ** -12) * (base.reshape(-1, 3).max(0) - base.reshape(-1, 3).min(0))).astype(F)
    out = {"nan_first_point": np.concatenate([np.stack([a, a, a])[None], base]),
           "nan_first_pair": np.concatenate([np.stack([a, a, b])[None], base]),
           "nan_block0": np.concatenate([np.stack([np.stack([nan_point(base, k)] * 3) for k in range(33)]), base]),
           "nan_only": np.stack([np.stack([p] * 3) for p in np.array([[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5],
                                                                      [0.1, 0.2, 0.3]], F)]),
           "degenerate": S.degenerate(28),
           "floor2047": floor(FLOOR_HALF)}
    for n in BLOCK_SIZES:
        out[f"sparse_{n}"] = S.sparse(40 + n, n=n)[:n] if n < 3 else S.sparse(40 + n, n=n - 2)
    return {k: np.ascontiguousarray(v, F) for k, v in out.items()}


NAN_FIRST = {"nan_first_point": 1, "nan_first_pair": 1, "nan_block0": 33, "nan_only": 3}     # leading NaN records


def morton_order(tris):
    """csrc/rt_dist_tree.h:70-87 in numpy: sorted record -> mesh triangle (centroids in double, 10 bits an axis in
    the vertex box, x the highest bit of each triple, ties by ascending triangle index)."""
    p = np.ascontiguousarray(tris, F).astype(np.float64)
    v = p.reshape(-1, 3)
    mn, mx = v.min(0), v.max(0)
    c = ((p[:, 0] + p[:, 1]) + p[:, 2]) / 3.0
    ext = mx - mn
    with np.errstate(all="ignore"):
        f = np.where(ext > 0.0, (c - mn) / np.where(ext > 0.0, ext, 1.0), 0.0)
    q = np.minimum(1023.0, np.maximum(0.0, f * 1024.0)).astype(np.uint64)
    code = np.zeros(p.shape[0], np.uint64)
    for bit in range(9, -1, -1):
        for a in range(3):
            code = (code << np.uint64(1)) | ((q[:, a] >> np.uint64(bit)) & np.uint64(1))
    return np.lexsort((np.arange(p.shape[0]), code)).astype(np.uint32)


def scene_file(scene, tmp):
    """The .rtscene a case's scene is loaded from: a shipped one, one of tests/golden/synth, or an A3 mesh saved with
    the A3 camera."""
    tmp = str(tmp)
    if scene in ("scene1", "scene8", "inside", "stack1500"):
        return S.scene_file({"scene": scene}, tmp)
    path = os.path.join(tmp, scene + ".rtscene")
    if not os.path.exists(path):
        v, t = S.mesh_of(meshes()[scene])
        hs = rtm.HostScene.from_mesh(v, t, MESH_FOV, S.look(MESH_CAM_EYE, MESH_CAM_AT))
        try:
            hs.save(path)
        finally:
            hs.close()
    return path


def scene_tris(path):
    hs = rtm.HostScene.load(path)
    try:
        v, t = hs.mesh()
        return D.triangles_of(v, t), hs.cam.copy(), F(hs.fov)
    finally:
        hs.close()


# ------------------------------------------------------------------ eyes
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum())


def eyes(tris):
    """[(name, eye f32 [3], at f32 [3], fov or None)] of the A2 cases for a mesh (float64 arithmetic, one rounding)."""
    p = np.ascontiguousarray(tris, F).astype(np.float64)
    v = p.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    ctr, ext = 0.5 * (lo + hi), hi - lo
    diag = float(np.sqrt((ext * ext).sum()))
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    k = int(np.argmax((nrm * nrm).sum(1)))                         # the largest triangle
    n, e1 = unit(nrm[k]), unit(p[k, 1] - p[k, 0])
    q = 0.5 * p[k, 0] + 0.3 * p[k, 1] + 0.2 * p[k, 2]
    face = ctr + np.array([0.0, -0.07, 0.13]) * ext
    face[0] = hi[0]
    out_eye = face + np.array([0.002, 0.0, 0.0])
    far_dir = unit([0.5, 0.3, 0.8])
    out = [("inside_box", ctr + np.array([0.13, -0.07, 0.11]) * ext, lo + 0.2 * ext, None),
           ("on_vertex", p[k, 0], ctr, None),
           ("off_0.0005", q + 0.0005 * n, q - n + 0.3 * e1, None),
           ("off_0.0015", q + 0.0015 * n, q - n + 0.3 * e1, None),
           ("on_face", face, ctr, None),
           ("on_corner", hi, ctr, None),
           ("out_away", out_eye, out_eye + np.array([1.0, 0.1, 0.05]), None),
           ("out_along", out_eye, out_eye + np.array([0.0, 1.0, 0.2]), None)]
    for name, m in zip(FAR_EYES, (1024.0, float(2 ** 20))):
        # the box about fills the frame: half the field of view spans 0.6 diagonals at m diagonals
        out.append((name, ctr + m * diag * far_dir, ctr, float(np.degrees(2.0 * np.arctan(0.6 / m)))))
    return [(nm, np.asarray(e, np.float64).astype(F), np.asarray(a, np.float64).astype(F), fv) for nm, e, a, fv in out]


# ------------------------------------------------------------------ the case list
def _case(group, scene, what, mode, cam, fov, frame, window):
    return {"key": f"{group}|{scene}|{what}|{mode}", "group": group, "scene": scene, "what": what, "mode": mode,
            "cam": np.asarray(cam, F).reshape(16), "fov": F(fov), "frame": frame, "window": window}


def _pair(group, scene, what, cam, fov, modes=("brute", "march")):
    x0, y0 = WINDOW.get(scene, (40, 20))
    out = []
    if "brute" in modes:
        out.append(_case(group, scene, what, "brute", cam, fov, FULL, FULL + (0, 0, FULL[0], FULL[1])))
    if "march" in modes:
        out.append(_case(group, scene, what, "march", cam, fov, MARCH_FRAME, FULL + (x0, y0, 16, 8)))
    return out


def specs(tmp):
    """Every case, built from the scene files and meshes (the generator's list; the tests read the fixture's)."""
    fac = dict(C.factors())
    out = []
    base = {}
    for scene in A1_SCENES + ("scene8",):
        base[scene] = scene_tris(scene_file(scene, tmp))
    for scene in A1_SCENES:
        _, cam0, fov = base[scene]
        for name in C.FACTOR_NAMES:
            out += _pair("A1", scene, name, C.apply_factor(cam0, fac[name]), fov)
    _, cam0, fov = base["scene8"]
    for name in SCENE8_FACTORS:
        cam = C.apply_factor(cam0, fac[name])
        out.append(_case("A1", "scene8", name, "brute", cam, fov, None, FULL + SCENE8_BRUTE))
        out.append(_case("A1", "scene8", name, "march", cam, fov, None, FULL + SCENE8_MARCH))
    _, cam0, fov = base["scene1"]
    x0, y0 = WINDOW["scene1"]
    for spp in (3, 5):
        cam = C.apply_factor(cam0, fac["scale_3"])
        out.append(_case("A1", "scene1", f"scale_3_spp{spp}", "brute", cam, fov, (96, 54, spp), (96, 54, spp, 0, 0, 96, 54)))
        out.append(_case("A1", "scene1", f"scale_3_spp{spp}", "march", cam, fov, (48, 27, spp), (96, 54, spp, x0, y0, 16, 8)))
    for scene in A2_SCENES:
        tris, _, fov0 = base[scene]
        for ename, eye, at, fov in eyes(tris):
            for name in A2_FACTORS:
                cam = C.apply_factor(S.look(eye, at), fac[name])
                out += _pair("A2", scene, f"{ename}@{name}", cam, fov0 if fov is None else fov, modes=("march",))
    mcam = S.look(MESH_CAM_EYE, MESH_CAM_AT)
    for scene in meshes():
        if scene == "floor2047":
            cam0 = S.look((0.3, -0.0012, 0.2), (1.3, -0.0012, 0.45))
            for name in FLOOR_FACTORS:
                out += _pair("A3", scene, name, C.apply_factor(cam0, fac[name]), 2.0)
        else:
            out += _pair("A3", scene, "identity", mcam, MESH_FOV)
    assert len({c["key"] for c in out}) == len(out)
    return out


# ------------------------------------------------------------------ records and their hashes
def columns(rec, mode):
    """{column: u32 words} of per-sample records (rt_sample_rec / orc_rec fields, or the reference's alt-samples
    records): what the fixture hashes.  A miss carries tri = 0xFFFFFFFF and t = u = v = 0; a march carries no
    triangle, u or v at all; floats NaN-canonical."""
    hit = np.ascontiguousarray(rec["hit"]).astype(np.uint32)
    out = {"hit": hit, "steps": np.ascontiguousarray(rec["steps"]).astype(np.uint32) if mode == "march" else np.zeros_like(hit),
           "t": S.nan_canonical(np.ascontiguousarray(rec["t"], F).view(np.uint32)),
           "rgb": S.nan_canonical(np.stack([np.ascontiguousarray(rec[k], F) for k in "rgb"], 1).view(np.uint32))}
    if mode == "brute":
        out["tri"] = np.where(hit == 1, rec["tri"], np.uint32(NOTRI)).astype(np.uint32)
        for k in "uv":
            out[k] = S.nan_canonical(np.ascontiguousarray(rec[k], F).view(np.uint32))
    return out


def entry(cols, frame_img):
    e = {"sha": {k: sha(v.astype("<u4")) for k, v in cols.items()}, "hits": int(cols["hit"].sum()),
         "steps": int(cols["steps"].astype(np.int64).sum())}
    if frame_img is not None:
        e["frame_sha"] = sha(np.ascontiguousarray(frame_img).astype("<u4"))
    return e


def check_columns(got, want, what):
    """Column by column, so that a mismatch is printed per sample."""
    assert sorted(got) == sorted(want), what
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: column {k}")


def check_entry(cols, frame_img, e, what):
    got = entry(cols, frame_img)
    assert got["hits"] == e["hits"] and got["steps"] == e["steps"], (what, got["hits"], e["hits"], got["steps"], e["steps"])
    bad = [k for k in e["sha"] if got["sha"][k] != e["sha"][k]]
    assert not bad, (what, "columns differ from the reference's", bad)
    if "frame_sha" in e:
        assert got["frame_sha"] == e["frame_sha"], (what, "the frame differs from the reference's")


# ------------------------------------------------------------------ the fixture
def fixture_text(generator, mesh_shas, cases):
    head = json.dumps({"generator": generator, "meshes": mesh_shas}, sort_keys=True, indent=1)
    body = ",\n".join(f"  {json.dumps(k)}: {json.dumps(cases[k], sort_keys=True)}" for k in sorted(cases))
    return head[:-2] + ',\n "cases": {\n' + body + "\n }\n}\n"


def to_json(c, e):
    """A case and its expected values as the fixture stores them."""
    d = {"cam": "".join(C.bits(c["cam"])), "fov": C.bits([c["fov"]])[0], "frame": c["frame"], "window": c["window"]}
    d.update(e)
    return d


def fixture():
    """{key: case} with the expected values under "exp" (cases as specs() builds them, cameras from the stored bits)."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    out = {}
    for key, d in fx["cases"].items():
        group, scene, what, mode = key.split("|")
        cam = C.from_bits([d["cam"][8 * i:8 * i + 8] for i in range(16)])
        c = _case(group, scene, what, mode, cam, C.from_bits([d["fov"]])[0],
                  tuple(d["frame"]) if d["frame"] else None, tuple(d["window"]))
        c["exp"] = {k: d[k] for k in ("sha", "hits", "steps", "frame_sha") if k in d}
        out[key] = c
    return out, fx["meshes"]


# ------------------------------------------------------------------ the live CPU restatement
class Live:
    """oracle/liboracle_tracer.so on a case: the restated IntersectBruteForce / RayMarch loops under the case's view
    (orc_scene_set_view), records of the window and the frame.  One scene handle per scene, results cached per case."""

    def __init__(self, oracle, tmp):
        self.oracle, self.tmp, self.scenes, self.cache = oracle, str(tmp), {}, {}
        self.pool = ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0))))
        oracle.L.orc_scene_set_view.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float]

    def scene(self, name):
        if name not in self.scenes:
            path = scene_file(name, self.tmp)
            self.scenes[name] = (path, S.OracleScene(self.oracle, path), scene_tris(path)[0])
        return self.scenes[name]

    def expect(self, c):
        """(columns of the window's records, frame u32 [H, W] or None)."""
        if c["key"] not in self.cache:
            _, osc, _ = self.scene(c["scene"])
            cam = np.ascontiguousarray(c["cam"], F)
            assert self.oracle.L.orc_scene_set_view(osc.h, ctypes.c_void_p(cam.ctypes.data), float(c["fov"])) == 0
            tt = ISECT[c["mode"]] << 8
            Wd, Ht, spp, x0, y0, w, h = c["window"]
            # (row by row on the pool: orc_trace_samples is one thread, and ctypes releases the GIL)
            rec = np.concatenate(list(self.pool.map(lambda y: osc.records(Wd, Ht, spp, (x0, y, w, 1), tri_test=tt),
                                                    range(y0, y0 + h))))
            img = osc.render(*c["frame"], tri_test=tt)[0] if c["frame"] else None
            self.cache[c["key"]] = (columns(rec, c["mode"]), img)
        return self.cache[c["key"]]

    def close(self):
        for _, osc, _ in self.scenes.values():
            osc.close()
        self.scenes = {}
        self.pool.shutdown()
