"""The miss skip on the device at the cases the parity tests render once (tests/miss_skip_cases.py).

A key gets its mask at its SECOND request, so the camera matrices, the synthetic views, the variant table and the
shipped scenes -- each rendered once by their own tests -- never ran k_miss_mask or process_item's flagged branch.
Here every one of those cases goes through miss_skip_cases.masked_vs_reference: rendered until its mask is in use for
a second frame, then held to the reference's frame (a golden, or the CPU restatement pinned to the goldens), to
the unskipped arms and to the CPU checker's flagged count.  No case, pixel or item is left out of a comparison.

Every group asserts how many of its cases reach the skip.  The counts below were taken with the CPU checker before
any GPU run (tests/test_miss_reach_cpu.py re-derives them on the CPU); a case that is expected to flag nothing is
named with its reason, and the device must flag exactly zero there too.

  group                     cases   reach the skip (asserted)    expected zero
  camera matrices           285     39, each count: CAM_FLAGGED   the rest: no item misses entirely, or CAM_REFUSED
  synthetic views           21 + 4  6, each count: SYNTH_FLAGGED  SYNTH_ZERO, one reason per view
  variants                  10      10: VARIANT_FLAGGED           none
  shipped scenes, 256x144   10      4: SHIPPED_FLAGGED            SHIPPED_ZERO, one reason per scene
    scenes 0 and 4, 1080p   2       2: BIG
  spp 32 / 64               2 x 2   4: SPP_FLAGGED                none
  sample tables             4 x 2   8: TABLE_FLAGGED              none
"""
import hashlib
import os

import numpy as np
import pytest

import camera_matrices as cm
import miss_skip_cases as mk
import occlusion_ref as R
import synth_scenes as ss
from conftest import load_package
from ray_variant_scenes import CallerBuilt

pytestmark = pytest.mark.gpu
rtm = load_package()
FX = cm.fixture()
CAM_SCENES = sorted({k.split("|")[0] for k in FX["cases"]})
META = ss.meta()
SYNTH_CASES = sorted(META["cases"])
FOV = 45.0
CAM_A = ((1.8, 1.2, 5.0), (1.1, 0.6, 0.0))       # tests/test_gpu_miss_skip.py's: the box [-1, 1]^3 across two frame edges


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return mk.build_checker(tmp_path_factory.mktemp("missreach"))


class Pair:
    """A host scene on the device twice -- with the skip and created with RT_MISS_SKIP=0 -- and the CPU restatement on its
    scene file."""

    def __init__(self, oracle, hs, path, own_hs=True, oracle_res=64):
        self.hs, self.path, self.own_hs = hs, path, own_hs
        self.skip, self.plain = mk.gpu_scene(hs, True), mk.gpu_scene(hs, False)
        self.oracle, self.osc = oracle, (mk.oracle_scene(oracle, path, oracle_res) if path else None)

    def close(self):
        self.skip.close()
        self.plain.close()
        if self.osc:
            self.osc.close()
        if self.own_hs and hasattr(self.hs, "close"):
            self.hs.close()


# ------------------------------------------------------------------ camera matrices
# Flagged items per (scene, factor), tests/miss_mask_check.cpp on the CPU before any GPU run (the 64-cell scenes at
# 96x54x4: 336 items with a valid lane; the single-cell scenes at 64x64x4 with camera_matrices.OFFSETS: 256 items).
# U: identity, the uniform scales 2^-45 .. 2^45, 3, 1/3, 1 + 2^-14, 1 + 2^-13, 1 + 2^-12, and the mirror (16 factors:
# a uniform scale moves no ray, and bounds of 2^45 are far inside the proof's 2^100).
#   scene      U     diag_1_4_1/4   shear   rank2
#   scene1     78    295            109     0 (84 items miss entirely; the zero up row puts 0 into a direction interval)
#   facing9    82    222            88      0 (48 items miss entirely; the same refusal)
#   scene8     0     233            20      0
#   edge_on17  0     218            0       0
#   inside, stack1500 and the nine sliver scenes: 0 for all 19 factors
# Every zero except the two rank2 cases named above is a frame in which NO item misses entirely (the checker's
# all_miss == 0: the eye is inside the box -- inside -- or the box fills the frame: scene8's ground, stack1500 at a
# field of view of 2 degrees, the pad triangles of the sliver scenes, edge_on17's long triangles), which the test
# asserts from the checker's own count.  39 of the 285 cases reach the skip.
CAM_UNIFORM = tuple(cm.UNIFORM) + ("mirror",)
CAM_FLAGGED = {"scene1": dict({f: 78 for f in CAM_UNIFORM}, **{"diag_1_4_1/4": 295, "shear": 109}),
               "facing9": dict({f: 82 for f in CAM_UNIFORM}, **{"diag_1_4_1/4": 222, "shear": 88}),
               "scene8": {"diag_1_4_1/4": 233, "shear": 20},
               "edge_on17": {"diag_1_4_1/4": 218}}
CAM_REFUSED = (("scene1", "rank2"), ("facing9", "rank2"))       # items miss entirely, the proof refuses them
CAM_MIN_FLAGGING = sum(len(v) for v in CAM_FLAGGED.values())
assert CAM_MIN_FLAGGING == 39 and len(CAM_UNIFORM) == 16


class CamScene(Pair):
    """tests/test_gpu_camera_matrices.py's Sc for the miss skip: the scene file, the frame shape and sample table of its
    cases, and the reference's frame per factor -- the CPU restatement held to the fixture's SHA-256s."""

    def __init__(self, oracle, name, tmp):
        self.name, self.cell = name, name not in cm.GRID_SCENES
        if self.cell:
            tris, cam = cm.cell_scenes(FX)[name]
            hs = cm.host_scene(tris, cam)
            path = os.path.join(str(tmp), name + ".rtscene")
            hs.save(path)
            self.shape, self.offsets = (cm.W, cm.H, cm.SPP), cm.OFFSETS
        else:
            path = ss.scene_file({"scene": name}, tmp)
            hs = rtm.HostScene.load(path)
            self.shape, self.offsets = cm.CAM_FRAME, None
        super().__init__(oracle, hs, path)
        self.smp = None if self.offsets is None else mk.samples_file(tmp, name, self.offsets)

    def cam_of(self, factor):
        e = FX["cases"][f"{self.name}|{factor}"]
        cam = cm.from_bits(FX["cams"][e["cam"]][factor])
        fov = float(cm.from_bits([FX["cams"][e["cam"]]["fov_bits"]])[0]) if not self.cell else 45.0
        return cam, fov

    def expected(self, factor):
        """The restatement's frame, its hit IDs held to the reference's (tests/golden/cameras.json: `refdriver render
        --view` for the 64-cell scenes, frame and hit IDs; `refdriver rays` for the single-cell ones, hit IDs)."""
        e = FX["cases"][f"{self.name}|{factor}"]
        cam, fov = self.cam_of(factor)
        img, hid = mk.oracle_frame(self.oracle, self.osc.h, *self.shape, cam, fov, self.offsets)
        assert sha(hid) == e["hits_sha256"], "the CPU restatement differs from the reference"
        if "bgra_sha256" in e:
            assert sha(img) == e["bgra_sha256"], "the CPU restatement differs from the reference"
        return img

    def checker_cases(self):
        out = []
        for factor in cm.FACTOR_NAMES:
            cam, fov = self.cam_of(factor)
            out.append(mk.case_args(*self.shape, cam=cam, fov=fov, samples=self.smp))
        return out


@pytest.fixture(scope="module")
def cam_scenes(oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("misscams")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = CamScene(oracle, name, tmp)
        return cache[name]
    get.tmp = tmp
    yield get
    for sc in cache.values():
        sc.close()


@pytest.mark.parametrize("scene", CAM_SCENES)
def test_camera_matrices(cam_scenes, checker, scene):
    """Every case of tests/golden/cameras.json (19 factors per scene), each settled on its mask."""
    sc = cam_scenes(scene)
    cpus = mk.cpu_masks(checker, sc.path, sc.checker_cases(), cam_scenes.tmp, scene)
    for factor, cpu in zip(cm.FACTOR_NAMES, cpus):
        cam, fov = sc.cam_of(factor)
        _, flagged = mk.masked_vs_reference(sc.skip, sc.plain, *sc.shape, sc.expected(factor), cpu, cam=cam, fov=fov,
                                            offsets=sc.offsets, what=f"{scene} {factor}")
        assert flagged == CAM_FLAGGED.get(scene, {}).get(factor, 0), (scene, factor)
        if flagged == 0:
            assert cpu["all_miss"] == 0 or (scene, factor) in CAM_REFUSED, (scene, factor, cpu)


def test_camera_matrices_reach_the_skip_without_the_gate_and_without_the_fast_reciprocal(cam_scenes):
    """Over the group: every case above asserts its exact count, so the CAM_MIN_FLAGGING cases of CAM_FLAGGED ran with
    flagged items (no state is shared with them: this test stands alone).  Among them are frames above kGateDmax (no
    gate records) and above kRcpMaxDir (no kVarFastRcp), by the bound the library itself takes from the matrix.  That
    those frames do take another launch is shown as tests/test_gpu_camera_matrices.py shows it: a batch of
    [identity, factor] falls back to one launch per frame (rt_scene_info.batch_fallbacks)."""
    import torch
    bound = {(s, f): mk.cam_dir_bound(cam_scenes(s).cam_of(f)[0]) for s, fs in CAM_FLAGGED.items() for f in fs}
    assert len(bound) == CAM_MIN_FLAGGING
    ungated = [k for k, b in bound.items() if mk.GATE_DMAX < b <= mk.RCP_MAX_DIR]
    slow_rcp = [k for k, b in bound.items() if b > mk.RCP_MAX_DIR]
    print("flagging cases without gate records:", ungated, "without kVarFastRcp:", slow_rcp)
    assert len(ungated) >= 2 and len(slow_rcp) >= 2
    sc = cam_scenes("scene1")
    W, H, spp = sc.shape
    st = torch.cuda.current_stream().cuda_stream
    for factor in ("scale_1+2^-13", "scale_2^4"):
        assert ("scene1", factor) in ungated + slow_rcp
        frames = [mk.frame(sc.skip, W, H, spp, sc.cam_of(f)[0], fov=sc.cam_of(f)[1]) for f in ("identity", factor)]
        outs = [torch.zeros(W * H, dtype=torch.int32, device="cuda") for _ in frames]
        before = sc.skip.info()["batch_fallbacks"]
        rtm.render_batch_device([sc.skip, sc.skip], frames, [o.data_ptr() for o in outs], stream=st)
        torch.cuda.synchronize()
        assert sc.skip.info()["batch_fallbacks"] == before + 1, factor
        for o, f in zip(outs, ("identity", factor)):
            assert np.array_equal(o.cpu().numpy().view(np.uint32).reshape(H, W), sc.expected(f)), f


# ------------------------------------------------------------------ synthetic views
# Flagged items (CPU checker, before any GPU run) per view of tests/golden/synth, 62x46x4 (192 items):
#   far_eye 121   flat_front 22   flat_inplane 143   thin_x 168   thin_y 168   thin_z 160
# The other fifteen views (and the four 63x47 axis frames) flag nothing; one by one:
SYNTH_FLAGGED = {"far_eye": 121, "flat_front": 22, "flat_inplane": 143, "thin_x": 168, "thin_y": 168, "thin_z": 160}
FILLS = "the box fills the frame: no item misses entirely"
SYNTH_ZERO = {
    "inside": "the eye is inside the box (point_in_aabb's refusal)",
    "eye_on_face": "the eye lies on the box's face, which point_in_aabb counts as inside",
    "eye_on_plane": FILLS + " (the eye is on an interior cell plane, outside the box, 1.5 from its face)",
    "away": "the camera looks away from the box, which is behind it: RayAABB has no tmax < 0 rejection, so every "
            "ray 'hits' the box and no item misses",
    "axis_x": FILLS, "axis_y": FILLS, "axis_z": FILLS, "fan_axis": FILLS, "degenerate": FILLS, "zero_normals": FILLS,
    "negative_octant": FILLS, "scale_1500": FILLS, "scale_2e-2": FILLS,
    "stack1500": FILLS + " (fov 2 degrees)", "stack2100": FILLS + " (fov 2 degrees)",
}
assert sorted(list(SYNTH_FLAGGED) + list(SYNTH_ZERO)) == SYNTH_CASES


@pytest.fixture(scope="module")
def synth_scenes(oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("misssynth")
    cache = {}

    def get(entry):
        key = entry["scene"]
        if key not in cache:
            path = ss.scene_file(entry, tmp)
            cache[key] = Pair(oracle, rtm.HostScene.load(path), path)
        return cache[key]
    yield get
    for sc in cache.values():
        sc.close()


@pytest.mark.parametrize("name", SYNTH_CASES)
def test_synthetic_views(synth_scenes, checker, name):
    """All 21 views (and the 63x47 frames of the axis cases) against the reference's own frames."""
    e0 = META["cases"][name]
    for e in [e0] + ([e0["axis_frame"]] if "axis_frame" in e0 else []):
        sc = synth_scenes(e)
        W, H, spp = e["W"], e["H"], e["spp"]
        ref = ss.read_synth(e["bgra"], "<u4").reshape(H, W)
        assert sha(ref) == e["bgra_sha256"]
        cpu = mk.cpu_mask(checker, sc.path, W, H, spp)
        _, flagged = mk.masked_vs_reference(sc.skip, sc.plain, W, H, spp, ref, cpu, what=e["name"])
        if name in SYNTH_ZERO:
            assert flagged == 0 and cpu["all_miss"] == 0, (name, SYNTH_ZERO[name])
        elif e is e0:
            assert flagged == SYNTH_FLAGGED[name], name


# ------------------------------------------------------------------ variants
# Cameras under which the box covers only part of the frame AND the mesh is seen (all at 45 degrees).  The stack is
# 0.023 wide in the middle of [-1, 1]^3: from outside the box it is a pixel or two, next to the box's right outline.
STACK_CAM = ((0.9, 0.5, 1.8), (0.6, 0.3, 0.0))
BIG_GRID_CAM = ((2.2, 1.4, 1.9), (0.0, 0.25, 0.25))         # tests/test_gpu_variants.py B4's first view


def stack2100_mesh(tmp):
    h0 = rtm.HostScene.load(ss.gunzip_scene("stack2100", tmp))
    try:
        return h0.mesh()
    finally:
        h0.close()


def variant_host(name, tmp):
    """(host scene whose own camera leaves part of the frame outside the box, the rt_scene_info it must have, the
    resolution of the CPU restatement's grid): the meshes of tests/test_gpu_variants.py B1-B4 and
    tests/ray_variant_scenes.py, not copied -- built by their generators (stack2100: read from its fixture)."""
    from ray_variant_scenes import ribbon_camera
    ores = 64
    if name in ("stack2100", "stack2048"):
        v, t = stack2100_mesh(tmp) if name == "stack2100" else ss.mesh_of(ss.stack(2048, 13))
        res, cam = 64, rtm.look_at(*STACK_CAM)
        info = dict(packed_cells=0, box_words=0, rcp_safe=1, pack_ok=1)
    elif name == "sheets16":
        (v, t), res, cam = ss.mesh_of(ss.sheets(7000, 41)), 16, rtm.look_at(*CAM_A)
        info = dict(packed_cells=1, box_words=0, rcp_safe=1)
        ores = 16         # (a 64^3 grid of 7,000 sheets takes the restatement five seconds to build; 16^3 is the device's own)
    elif name.startswith("ribbon_"):
        axis, res = "xyz".index(name[7]), int(name[8:])
        (v, t), cam = ss.mesh_of(ss.ribbon(axis, 50 + axis)), ribbon_camera(axis)
        info = dict(pack_ok=int(res <= 512), packed_cells=1, rcp_safe=1)
    elif name == "big_grid":
        (v, t), res, cam = ss.mesh_of(ss.big_grid_mesh(60)), 512, rtm.look_at(*BIG_GRID_CAM)
        info = dict(octant_words=0, packed_cells=1, box_words=0, pack_ok=1, rcp_safe=1)
    else:
        raise KeyError(name)
    return rtm.HostScene.from_mesh(v, t, FOV, cam, grid_res=res), info, ores


# Flagged items (CPU checker before any GPU run; 64x64x4, Hammersley samples: 256 items), in brackets the items that
# miss entirely and the samples of the frame that hit a triangle:
VARIANT_FLAGGED = {"stack2100": 24,        # (29; 3)
                   "stack2048": 24,        # (29; 4)
                   "sheets16": 136,        # (169; 4,620)
                   "ribbon_x513": 205,     # (218; 71)
                   "ribbon_y513": 218,     # (219; 156)
                   "ribbon_z513": 205,     # (218; 91)
                   "ribbon_z512": 205,     # (218; 91)
                   "big_grid": 176,        # (184; 70)
                   "huge_axis_z": 136,     # (169; 1,561, 283 of them on the appended triangle)
                   "huge_stack2100": 24}   # (29; 2,565, 2,562 of them on the appended triangle)
# None is expected to flag nothing.  The two caller-built grids (B5: a triangle with edges of 2^62 listed by hand)
# keep the base scene's box [-1, 1]^3: the proof reads the BOX and the camera, never a triangle, so nothing of it
# comes near 2^100 and they flag what their base scenes flag (the count is the checker's on the base scene's file,
# which has the same box and camera).  A box of 2^62 would be refused -- but no scene here has one: a mesh with
# such a triangle cannot be given a grid by the builder at all.
FILE_VARIANTS = ("stack2100", "stack2048", "sheets16", "ribbon_x513", "ribbon_y513", "ribbon_z513", "ribbon_z512",
                 "big_grid")
HUGE_VARIANTS = ("huge_axis_z", "huge_stack2100")
VW, VH, VSPP = cm.W, cm.H, cm.SPP


@pytest.mark.parametrize("name", FILE_VARIANTS)
def test_variants(oracle, checker, tmp_path, name):
    """B1-B4 and the ray-variant scenes: the fall-back instantiations of kVarAutoCore with a mask in use, against the
    CPU restatement on the saved scene file; and the RT_TRI_BARYCENTRIC frame of the same scene, which takes no mask."""
    hs, info, ores = variant_host(name, tmp_path)
    path = os.path.join(str(tmp_path), name + ".rtscene")
    hs.save(path)
    sc = Pair(oracle, hs, path, oracle_res=ores)
    try:
        got = sc.skip.info()
        assert {k: got[k] for k in info} == info, got
        exp, hid = sc.osc.render(VW, VH, VSPP)
        assert (hid != cm.NOTRI).any(), "the mesh is not in the frame"
        cpu = mk.cpu_mask(checker, path, VW, VH, VSPP)
        assert cpu["flagged"] == VARIANT_FLAGGED[name]
        _, flagged = mk.masked_vs_reference(sc.skip, sc.plain, VW, VH, VSPP, exp, cpu, what=name)
        assert flagged > 0, name
        # the barycentric frame of the same key, between two masked frames: it must be the reference's whatever the
        # host hands the kernel (it hands no mask), and the masked frame after it is unchanged
        bary = sc.skip.render_frame(mk.frame(sc.skip, VW, VH, VSPP, tri_test=rtm.RT_TRI_BARYCENTRIC))
        assert np.array_equal(bary, sc.osc.render(VW, VH, VSPP, tri_test=1)[0]), "RT_TRI_BARYCENTRIC"
        assert sc.skip.miss_mask()[0] == 0
        again = sc.skip.render_frame(mk.frame(sc.skip, VW, VH, VSPP))
        assert np.array_equal(again, exp) and sc.skip.miss_mask()[0] == flagged
    finally:
        sc.close()


@pytest.mark.parametrize("name", HUGE_VARIANTS)
def test_variants_caller_built(oracle, checker, tmp_path, name):
    """B5: rcp_safe == 0 (kVarAutoCore | kVarPackedRem | kVarSkipRun on axis_z, kVarAutoCore alone on stack2100).  The
    reference cannot build these grids and the oracle cannot read them, so -- as tests/test_gpu_variants.py does --
    the per-sample hit IDs are held to tests/occlusion_ref.py's walk over the caller's arrays on GenerateRay's own
    rays, and the masked frame to the frame of that hit-ID launch and to the unskipped arms.  Plainly: for these two
    cases the COLOURS' reference is the library's own unmasked output (the hit-ID launch takes no mask; RT_MISS_SKIP=0
    and RT_KERNEL_LANES never do), and only the hit IDs have an independent one.  Every other case of this file has a
    reference that shares no code with the library.
    The flagged count is the checker's on the BASE scene's file: the same box and camera."""
    import torch
    if name == "huge_axis_z":
        c = ss.cases()["axis_z"]
        (v, t), cam = ss.mesh_of(c["tris"], c["zero_normals"]), rtm.look_at(*CAM_A)
    else:
        (v, t), cam = stack2100_mesh(tmp_path), rtm.look_at(*STACK_CAM)
    base = rtm.HostScene.from_mesh(v, t, FOV, cam, grid_res=64)
    path = os.path.join(str(tmp_path), name + "_base.rtscene")
    base.save(path)
    cb = CallerBuilt(base)
    base.close()
    sc = Pair(oracle, cb, None)
    try:
        info = sc.skip.info()
        pins = dict(rcp_safe=0, packed_cells=1, box_words=1, pack_ok=1, octant_words=1) if name == "huge_axis_z" else \
            dict(rcp_safe=0, packed_cells=0, box_words=0, pack_ok=1, max_cell_refs=2100)       # tests/test_gpu_variants.py B5's
        assert {k: info[k] for k in pins} == pins, info
        cpu = mk.cpu_mask(checker, path, VW, VH, VSPP)
        assert cpu["flagged"] == VARIANT_FLAGGED[name]
        rays = cm.generate_rays(cam, FOV, VW, VH, rtm.sample_table(VSPP))
        res = R.walk(R.RefScene(cb.g, cb.offs, cb.refs, cb.v, cb.t), rays)
        hid = np.where(res["hit"], res["tri"], np.uint32(cm.NOTRI)).astype(np.uint32)
        assert (hid == cb.t.shape[0] - 1).any(), "no sample reaches the appended triangle"
        out = torch.full((VW * VH,), cm.SENTINEL, dtype=torch.int32, device="cuda")
        hits = torch.full((VW * VH * VSPP,), cm.SENTINEL, dtype=torch.int32, device="cuda")
        sc.skip.render_hits_device(mk.frame(sc.skip, VW, VH, VSPP), 0, 1, out.data_ptr(), hits.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(hits.cpu().numpy().view(np.uint32), hid), "hit IDs"
        exp = out.cpu().numpy().view(np.uint32).reshape(VH, VW)
        _, flagged = mk.masked_vs_reference(sc.skip, sc.plain, VW, VH, VSPP, exp, cpu, what=name)
        assert flagged > 0, name
    finally:
        sc.close()


# ------------------------------------------------------------------ shipped scenes
# Flagged items (CPU checker, before any GPU run) at 256x144x4 (2,304 items), the scenes' own cameras:
#   0: 725 (758 miss entirely)   1: 630 (648)   4: 560 (576)   6: 204 (219)
# and zero where no item misses entirely (all_miss == 0, asserted), one by one:
SHIPPED_FLAGGED = {0: 725, 1: 630, 4: 560, 6: 204}
SHIPPED_ZERO = {2: "the box fills the frame", 3: "the box fills the frame", 5: "the camera is inside the box",
                7: "the box fills the frame", 8: "the ground's box fills the frame", 9: "the box fills the frame"}
BIG = {0: 45290, 4: 34701}          # flagged of 129,600 items at 1920x1080x4 (tests/test_miss_mask.py)


@pytest.mark.parametrize("sid", range(10))
def test_shipped_scenes(golden, oracle, checker, sid):
    """All ten at 256x144x4 against the CPU restatement; scenes 0 and 4 (never rendered with a mask before; scene 4
    keeps 256-lane workgroups for its 1,000+-reference cells) at 1920x1080x4 against the reference's golden SHA-256."""
    hs = rtm.HostScene.load(sid)
    path = rtm.scene_path(sid)
    skip, plain = mk.gpu_scene(hs, True), mk.gpu_scene(hs, False)
    try:
        W, H, spp = 256, 144, 4
        cpu = mk.cpu_mask(checker, path, W, H, spp)
        _, flagged = mk.masked_vs_reference(skip, plain, W, H, spp, oracle.render(sid, W, H, spp)[0], cpu, what=f"scene {sid}")
        if sid in SHIPPED_ZERO:
            assert flagged == 0 and cpu["all_miss"] == 0, (sid, SHIPPED_ZERO[sid])
        else:
            assert flagged == SHIPPED_FLAGGED[sid], sid
        if sid in BIG:
            W, H = 1920, 1080
            cpu = mk.cpu_mask(checker, path, W, H, spp)
            assert cpu["flagged"] == BIG[sid]
            a, flagged = mk.masked_vs_reference(skip, plain, W, H, spp, None, cpu, what=f"scene {sid} 1080p",
                                                sha256=golden["frames_1080p4"][str(sid)]["bgra_sha256"])
            assert flagged == BIG[sid]
    finally:
        skip.close()
        plain.close()
        hs.close()


# ------------------------------------------------------------------ spp 32 and 64, caller-supplied sample tables
@pytest.fixture(scope="module")
def synth(oracle, tmp_path_factory):
    """tests/test_gpu_miss_skip.py's two meshes: {name: Pair}"""
    tmp = tmp_path_factory.mktemp("missspp")
    out = {}
    for name, (tris, res) in mk.synth_meshes().items():
        hs = cm.host_scene(tris, rtm.look_at(*CAM_A), fov=FOV, grid_res=res)
        path = str(tmp / f"{name}.rtscene")
        hs.save(path)
        out[name] = Pair(oracle, hs, path)
    out["tmp"] = tmp
    yield out
    for k, sc in out.items():
        if k != "tmp":
            sc.close()


# Flagged items (CPU checker before any GPU run), 64x48, CAM_A; 1,536 items at spp 32 and 3,072 at spp 64, where an
# item is ONE pixel (and row_miss_word takes the generic resolve at both):
SPP_FLAGGED = {("cell1", 32): 867, ("cell1", 64): 1806, ("grid64", 32): 918, ("grid64", 64): 1883}


@pytest.mark.parametrize("spp", [32, 64])
@pytest.mark.parametrize("name", ["cell1", "grid64"])
def test_spp_32_and_64(synth, checker, name, spp):
    sc = synth[name]
    W, H = 64, 48
    cam = mk.cam16(CAM_A)
    cpu = mk.cpu_mask(checker, sc.path, W, H, spp, cam=cam)
    exp, _ = mk.oracle_frame(sc.oracle, sc.osc.h, W, H, spp, cam, FOV)
    _, flagged = mk.masked_vs_reference(sc.skip, sc.plain, W, H, spp, exp, cpu, cam=cam, what=f"{name} spp {spp}")
    assert flagged == SPP_FLAGGED[(name, spp)]


def sample_tables():
    """{name: [4, 2] float32}: offsets at exactly +-0.5 (the documented range's ends), all equal, seeded -- and one
    outside [-0.5, 0.5], which the ABI accepts (rt_frame.sample_offsets is not range-checked): the scan of ndcx / ndcy
    must enclose whatever the table holds."""
    r = np.random.Generator(np.random.PCG64(20261021))
    return {"corners": np.array([[-0.5, -0.5], [0.5, -0.5], [-0.5, 0.5], [0.5, 0.5]], np.float32),
            "equal": np.full((4, 2), (0.25, -0.125), np.float32),
            "seeded": r.uniform(-0.5, 0.5, (4, 2)).astype(np.float32),
            "outside": np.array([[-1.5, 0.75], [1.25, -2.0], [0.0, 0.0], [2.5, 1.5]], np.float32)}


# Flagged items (CPU checker before any GPU run), 96x54x4 (336 items with a valid lane), CAM_A, per table; cell1's
# box is a little larger than grid64's (its facing triangles reach past the anchors), which shows under the widest
# table only:
TABLE_FLAGGED = {"corners": (168, 168), "equal": (177, 177), "seeded": (169, 169), "outside": (142, 152)}   # (cell1, grid64)


@pytest.mark.parametrize("table", ["corners", "equal", "seeded", "outside"])
@pytest.mark.parametrize("name", ["cell1", "grid64"])
def test_caller_supplied_sample_offsets(synth, checker, name, table):
    sc = synth[name]
    W, H, spp = 96, 54, 4
    cam, tbl = mk.cam16(CAM_A), sample_tables()[table]
    cpu = mk.cpu_mask(checker, sc.path, W, H, spp, cam=cam, samples=mk.samples_file(synth["tmp"], table, tbl))
    exp, _ = mk.oracle_frame(sc.oracle, sc.osc.h, W, H, spp, cam, FOV, tbl)
    _, flagged = mk.masked_vs_reference(sc.skip, sc.plain, W, H, spp, exp, cpu, cam=cam, offsets=tbl,
                                        what=f"{name} {table}")
    assert flagged == TABLE_FLAGGED[table][name == "grid64"]
