"""Cameras whose 3x3 is not orthonormal, shared by oracle/gen_golden_cameras.py (which pins them to the
reference's own code), tests/test_oracle_cameras.py, tests/test_record_gate.py and
tests/test_gpu_camera_matrices.py.  A plain module, not a conftest.

rt_frame.cam is the caller's matrix.  GenerateRay (camera.h:39-46, rtd::dir_from_xy) normalises the camera-space
direction first and multiplies by the 3x3 afterwards, so a ray's direction is as long as the matrix makes it.
Two proofs of the benchmarked path hold for |D_i| <= 1.0001 (the record gate, csrc/rt_record_gate.h) and for
|D|_inf <= 8 (kVarFastRcp, csrc/rt_ray_common.h); the library bounds |D_i| per frame from the matrix
(csrc/rt_cam_bound.h) and drops the gate / the fast reciprocal for frames above.  Every camera of the other
test files is orthonormal; the ones here are the 3x3 of a rotation (a scene's own camera, or the frozen
rotation of the sliver scene) times a FACTOR, applied from the left: it scales, mixes or drops the camera's
right / up / back rows.
"""
import json
import math
import os

import numpy as np

from conftest import GOLD, load_package

rtm = load_package()
F = np.float32
W, H, SPP = 64, 64, 4                        # the single-cell scenes' frame (test_gpu_uniform_lists.py's)
OFFSETS = np.array([0.0, 0.0, 0.25, 0.5, 0.5, 0.25, 0.75, 0.75], F)       # ... and its sample table
CAM_FRAME = (96, 54, 4)                      # the 64-cell scenes' frame (Hammersley samples)
SENTINEL = 0x5A5A5A5A
NOTRI = 0xFFFFFFFF
FIXTURE = os.path.join(GOLD, "cameras.json")


# ------------------------------------------------------------------ the factors
def factors():
    """[(name, 3x3 float64)] in fixture order.  uniform 2^k: k = +-45 put every lane outside rt_setup_div.h's
    window (whole waves take the division), and at 2^-45 every det is below 1e-8: a background frame.
    1 + 2^-14 and 1 + 2^-13 lie either side of kGateDmax = 1.0001 (1 + 2^-12 is above as well)."""
    out = [("identity", np.eye(3))]
    for k in (-45, -20, -10, -1, 1, 4, 10, 20, 45):
        out.append((f"scale_2^{k}", np.eye(3) * 2.0 ** k))
    out.append(("scale_3", np.eye(3) * 3.0))
    out.append(("scale_1/3", np.eye(3) / 3.0))
    for k in (14, 13, 12):
        out.append((f"scale_1+2^-{k}", np.eye(3) * (1.0 + 2.0 ** -k)))
    out.append(("diag_1_4_1/4", np.diag([1.0, 4.0, 0.25])))
    shear = np.eye(3)
    shear[0, 1] = 0.75                       # row 0 += 0.75 * row 1
    out.append(("shear", shear))
    out.append(("mirror", np.diag([-1.0, 1.0, 1.0])))                    # det -1
    out.append(("rank2", np.diag([1.0, 0.0, 1.0])))                      # row 1 (up) zero: every ray in one plane
    return out


FACTOR_NAMES = [n for n, _ in factors()]
UNIFORM = [n for n in FACTOR_NAMES if n == "identity" or n.startswith("scale_")]
# no sample of these may be left out of a comparison (the others: at most 0.5 % of a case's samples)
NO_SKIP = UNIFORM + ["mirror"]
S1024 = "scale_2^10"


def apply_factor(cam16, factor):
    """cam16 with its 3x3 replaced by float32(factor @ 3x3) (float64 product, one rounding); eye and the fourth
    column unchanged."""
    m = np.array(cam16, F).reshape(4, 4).copy()
    f, r = np.asarray(factor, np.float64), m[:3, :3].astype(np.float64)
    # (explicit sums, no BLAS: the same bits wherever this runs)
    m[:3, :3] = np.stack([(f[i, 0] * r[0] + f[i, 1] * r[1]) + f[i, 2] * r[2] for i in range(3)]).astype(F)
    return m.reshape(16)


def m9_of(cam16):
    return np.asarray(cam16, F).reshape(4, 4)[:3, :3].reshape(9)


def hexf(values):
    """float32 values as C hex-float strings (exact; strtof reads them)."""
    return [float(F(x)).hex() for x in np.asarray(values, F).reshape(-1)]


def bits(values):
    return [f"{int(x):08x}" for x in np.asarray(values, F).reshape(-1).view(np.uint32)]


def from_bits(hexes):
    return np.array([int(x, 16) for x in hexes], np.uint32).view(F)


# ------------------------------------------------------------------ GenerateRay in numpy float32
def fov_xs_of(fov):
    hfov = F(fov) * F(0.0174532925)                              # lin_alg.h:232
    return F(math.tan(float(hfov / F(2.0))))                     # camera.h:42, double tan


def generate_rays(cam16, fov, Wd, Ht, smp):
    """camera.h:8-47, perspective branch, for every (y, x, sample) of a frame: [n, 6] float32 (origin,
    direction).  One rounding per reference operation, in its order; two ufunc calls never fuse."""
    m = np.asarray(cam16, F).reshape(4, 4)
    smp = np.asarray(smp, F).reshape(-1, 2)
    y, x, s = [a.reshape(-1) for a in np.meshgrid(np.arange(Ht), np.arange(Wd), np.arange(smp.shape[0]), indexing="ij")]
    fxs, aspect = fov_xs_of(fov), F(Wd) / F(Ht)
    with np.errstate(all="ignore"):
        cx = ((x.astype(F) + smp[s, 0]) / F(Wd) * F(2.0) - F(1.0)) * fxs
        cy = ((y.astype(F) + smp[s, 1]) / F(Ht) * F(2.0) - F(1.0)) * fxs / aspect
        cz = np.full_like(cx, F(-1.0))
        d = F(0.0) + cx * cx                                     # lin_alg.h:138-156 Dot from T() = 0, Normalize
        d = d + cy * cy
        d = d + cz * cz
        ln = F(1.0) / np.sqrt(d)
        px, py, pz = cx * ln, cy * ln, cz * ln
        rays = np.zeros((x.size, 6), F)
        for k in range(3):
            rays[:, k] = F(0.0) * m[0, k] + F(0.0) * m[1, k] + F(0.0) * m[2, k] + m[3, k]       # lin_alg.h:518-535
            rays[:, 3 + k] = px * m[0, k] + py * m[1, k] + pz * m[2, k]                         # lin_alg.h:495-509
    return rays


# ------------------------------------------------------------------ single-cell scenes (grid_res = 1)
def mesh_of(tris):
    """tris [nt, 3, 3] -> (vertices [3 nt, 6], triangles [nt, 6]) as test_gpu_uniform_lists.mesh_of."""
    p = np.asarray(tris, F)
    nt = p.shape[0]
    v = np.zeros((nt * 3, 6), F)
    v[:, :3] = p.reshape(-1, 3)
    v[:, 4] = 1.0
    t = np.zeros((nt, 6), np.uint32)
    t[:, :3] = np.arange(nt * 3, dtype=np.uint32).reshape(nt, 3)
    t[:, 4] = F(1.0).view(np.uint32)
    return v, t


def rotation(seed):
    """A seeded rotation (float64, det +1): rows right, up, back."""
    r = np.random.Generator(np.random.PCG64(seed))
    w, x, y, z = r.uniform(-1.0, 1.0, 4)                         # a quaternion, explicit arithmetic (no LAPACK)
    n = w * w + x * x + y * y + z * z
    s = 2.0 / n
    return np.array([[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                     [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                     [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]])


SLIVER_COLUMN = 20
SLIVER_DIST = 4.0


def sliver_camera(seed):
    """The sliver scene's camera: a seeded rotation, the eye SLIVER_DIST along its back row (looking at 0)."""
    R = rotation(seed)
    m = np.eye(4)
    m[:3, :3] = R
    m[3, :3] = SLIVER_DIST * R[2]
    return m.astype(F).reshape(16)


def to_world(cam16, pts_cam):
    """Points in camera coordinates (x right, y up, z back; in front of the eye z < 0) -> world, float64."""
    m = np.asarray(cam16, F).reshape(4, 4).astype(np.float64)
    p = np.asarray(pts_cam, np.float64)
    return m[3, :3] + ((p[:, 0:1] * m[0, :3] + p[:, 1:2] * m[1, :3]) + p[:, 2:3] * m[2, :3])


def sliver_triangle(cam16, width):
    """The sliver, in world coordinates (float64, rounded to float32 by the caller): its u = 0 edge v0 -> v2
    lies in the plane of the rays of pixel column SLIVER_COLUMN, sample 0 of the W x H frame at 45 degrees
    (OFFSETS' first sample is the pixel corner), and v1 = v0 + width * right + 0.1 * up.  Rays of that column
    meet the edge to within rounding: u is 0 give or take, ok1 holds for about half of them -- and |g_z| is
    |g_h| give or take for all of them, which is where a gate bound computed for shorter directions fails.
    Every other lane of a wave (4 x 4 pixels x 4 samples) is at least a quarter pixel away: u > 1 or < 0."""
    cx = float((F(SLIVER_COLUMN) / F(W) * F(2.0) - F(1.0)) * fov_xs_of(45.0))
    ylim = 1.2 * float(fov_xs_of(45.0))
    v0 = SLIVER_DIST * np.array([cx, -ylim, -1.0])
    v2 = (SLIVER_DIST + 0.3) * np.array([cx, ylim, -1.0])
    v1 = v0 + np.array([width, 0.1, 0.0])
    return to_world(cam16, np.stack([v0, v1, v2]))


def pad_triangle(cam16, i):
    """A triangle off to one side of everything the frame sees (|x| < 1.7 at the sliver's depth), e1 along the
    camera's right: u lies outside [0, 1] for every ray, so every lane's first half -- and the gate -- rejects
    it.  Tall enough (|y| <= 3) that the grid box covers the whole frame: every lane walks the one cell."""
    x0 = 5.0 + 0.25 * (i % 4) if i % 2 else -7.0 - 0.25 * (i % 3)
    z = -SLIVER_DIST + 0.03 * i
    return to_world(cam16, [[x0, -3.0, z], [x0 + 1.0, -3.0 + 0.01 * (i % 5), z], [x0 + 0.1, 3.0, z]])


def sliver_scene(cam16, width, nt, pos):
    """nt triangles [nt, 3, 3] float32: pad triangles with the sliver at list position pos."""
    tris = [pad_triangle(cam16, i) for i in range(nt)]
    tris[pos] = sliver_triangle(cam16, width)
    return np.asarray(tris, np.float64).astype(F)


SLIVER_LISTS = [(8, 0), (8, 4), (8, 7), (9, 0), (9, 4), (9, 8), (17, 0), (17, 8), (17, 16)]     # (records, sliver at)


def facing_stack(zs):
    """test_gpu_uniform_lists.facing_stack: one big triangle per z around the z axis."""
    out = []
    for i, z in enumerate(zs):
        s = 1.0 + 0.03 * (i % 5)
        out.append([[-s, -0.9, z], [s, -0.8, z], [0.05 * (i % 3), s, z]])
    return np.asarray(out, F)


def edge_on(nt):
    """test_gpu_record_gate's nearly-edge-on scene: triangles whose plane holds the camera axis to within 1e-7."""
    tris = []
    for i in range(nt - 1):
        tilt = (i - (nt - 1) // 2) * 2.5e-8
        x = 0.01 * (i % 3 - 1)
        tris.append([[x, -1.0, 0.5], [x + tilt, 1.0, 0.6], [x - tilt, 0.1 * (i % 4), 2.5]])
    tris.insert(nt // 2, facing_stack([0.0])[0].tolist())
    return np.asarray(tris, F)


EYE, AT = (0.0, 0.0, 4.0), (0.0, 0.0, 0.0)


def cell_scenes(fx=None):
    """{name: (tris f32 [nt, 3, 3], cam16 f32)}: the grid_res = 1 scenes.  The sliver scenes come from the
    fixture's frozen bits (fx: the loaded fixture; None: without them)."""
    out = {"facing9": (facing_stack([0.05 * i for i in range(9)]), rtm.look_at(EYE, AT)),
           "edge_on17": (edge_on(17), rtm.look_at(EYE, AT))}
    if fx is not None:
        cam = from_bits(fx["sliver"]["cam_bits"])
        for nt, pos in SLIVER_LISTS:
            out[f"sliver{nt}_{pos}"] = (from_bits(fx["sliver"]["scenes"][f"{nt}_{pos}"]).reshape(nt, 3, 3), cam)
    return out


def host_scene(tris, cam16, fov=45.0, grid_res=1):
    v, t = mesh_of(tris)
    return rtm.HostScene.from_mesh(v, t, fov, np.asarray(cam16, F), grid_res=grid_res)


GRID_SCENES = ("scene1", "scene8", "stack1500", "inside")       # 64-cell grids: the reference renders them itself


def base_of(scene):
    """Whose rotation a scene's cameras are built on: its own camera's (the 64-cell scenes), the frozen seeded one
    (the sliver scenes) or look_at(EYE, AT)."""
    return scene if scene in GRID_SCENES else ("sliver" if scene.startswith("sliver") else "look_at")


def compact(fx):
    """The fixture as committed: what cannot be recomputed -- the base cameras' bits, the frozen sliver triangle, the
    checker's counts on it, and per case the reference's SHA-256s and hit count (hits, hit_samples[, bgra])."""
    sl = fx["sliver"]
    nt, pos = SLIVER_LISTS[0]
    tri = sl["scenes"][f"{nt}_{pos}"][9 * pos:9 * pos + 9]
    return {"generator": fx["generator"], "factors": fx["factors"], "bases": fx["bases"], "dropped": fx["dropped"],
            "sliver": {"seed": sl["seed"], "width": sl["width"], "cam_bits": sl["cam_bits"], "tri_bits": tri,
                       "gate_check": sl["gate_check"]},
            "cases": {k: [e["hits_sha256"], e["hit_samples"]] + ([e["bgra_sha256"]] if "bgra_sha256" in e else [])
                      for k, e in fx["cases"].items()}}


def expand(c):
    """compact()'s inverse: every camera (a base's 3x3 times each factor, apply_factor), the nine sliver lists (the
    pad triangles around the frozen sliver) and each case's frame shape, as the tests read them."""
    fac = factors()
    assert c["factors"] == [n for n, _ in fac]
    fx = {k: c[k] for k in ("generator", "factors", "bases", "dropped")}
    fx["cams"] = {}
    for base, b in c["bases"].items():
        fx["cams"][base] = {n: bits(apply_factor(from_bits(b["cam_bits"]), f)) for n, f in fac}
        if "fov_bits" in b:
            fx["cams"][base]["fov_bits"] = b["fov_bits"]
    sl = c["sliver"]
    cam = from_bits(sl["cam_bits"])
    fx["sliver"] = {k: sl[k] for k in ("seed", "width", "cam_bits", "gate_check")}
    fx["sliver"]["scenes"] = {}
    for nt, pos in SLIVER_LISTS:
        tris = np.asarray([pad_triangle(cam, i) for i in range(nt)], np.float64).astype(F)
        tris[pos] = from_bits(sl["tri_bits"]).reshape(3, 3)
        fx["sliver"]["scenes"][f"{nt}_{pos}"] = bits(tris)
    fx["cases"] = {}
    for k, v in c["cases"].items():
        scene, factor = k.split("|")
        Wd, Ht, spp = CAM_FRAME if scene in GRID_SCENES else (W, H, SPP)
        e = {"scene": scene, "factor": factor, "W": Wd, "H": Ht, "spp": spp, "grid_res": 64 if scene in GRID_SCENES else 1,
             "cam": base_of(scene), "hits_sha256": v[0], "hit_samples": v[1]}
        if len(v) > 2:
            e["bgra_sha256"] = v[2]
        fx["cases"][k] = e
    return fx


def fixture_text(fx):
    """The committed file's text: compact(), one case per line."""
    c = compact(fx)
    cases = c.pop("cases")
    head = json.dumps(c, sort_keys=True, indent=1)
    body = ",\n".join(f"  {json.dumps(k)}: {json.dumps(cases[k])}" for k in sorted(cases))
    return head[:-2] + ',\n "cases": {\n' + body + "\n }\n}\n"


def fixture():
    with open(FIXTURE) as f:
        return expand(json.load(f))
