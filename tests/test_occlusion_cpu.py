"""rt_occluded_rays_device without a GPU.

1. tests/occlusion_ref.py (the numpy float32 restatement the GPU tests hold the kernel to) is pinned to the
   REFERENCE: on the reference's own GenerateRay rays (oracle.kat("genray")) of all 21 synthetic views at 62x46x4 and
   the four 63x47x4 axis frames, its closest-hit mode must reproduce every geometric fixture column (hit, tri,
   voxel, t, u, v, steps, tests; tests/golden/synth, written by the reference's Grid::Intersect), and its occlusion
   mode over (-inf, +inf) must equal the fixture's hit column.
2. The implication the header states, on intervals derived from the fixtures' own t.
3. The ABI surface, the argument checks that come before any device call, the Python layer's validation.
4. The build guards of csrc/rt_occlusion.hip, by the method of tests/test_rays_cpu.py.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import occlusion_ref as R
import synth_scenes as S
from conftest import PKG_DIR, ROOT, load_package
from hip_remarks import FLAGS, HIPCC, last_error, needs_hipcc, resource_table

rtm = load_package()
META = S.meta()
CASES = sorted(META["cases"])
GEOM_COLS = ("hit", "tri", "voxel", "t", "u", "v", "steps", "tests")
OCC_SRC = os.path.join(PKG_DIR, "csrc", "rt_occlusion.hip")
FAKE = ctypes.c_void_p(1)            # a scene handle the rejected calls never dereference
# the header's cap on the converse of the implication: rays with ref.hit && ref.t < tmax that the occlusion walk
# does not report, per view and interval, as a share of the view's hit rays
CONVERSE_CAP = 0.01


def frames_of(e):
    return [e] + ([e["axis_frame"]] if "axis_frame" in e else [])


def genray(oracle, cam, fov, W, H, spp):
    """The reference's GenerateRay for every (y, x, sample) of a frame (orc_kat_genray's 23-word input, as
    tests/test_gpu_rays.py check_genray builds it)."""
    smp = rtm.sample_table(spp)
    y, x, s = [a.reshape(-1) for a in np.meshgrid(np.arange(H), np.arange(W), np.arange(spp), indexing="ij")]
    rin = np.zeros((W * H * spp, 23), np.float32)
    rin[:, :16] = np.asarray(cam, np.float32)
    bits = rin.view(np.uint32)
    bits[:, 16], bits[:, 17], bits[:, 18], bits[:, 19] = x, y, W, H
    rin[:, 20], rin[:, 21], rin[:, 22] = smp[s, 0], smp[s, 1], np.float32(fov)
    return np.ascontiguousarray(oracle.kat("genray", rin, 6), np.float32)


@pytest.fixture(scope="module")
def walked(oracle, tmp_path_factory):
    """Per fixture entry: (RefScene, rays, the restatement's closest-hit result) -- computed once, never changed."""
    tmp = tmp_path_factory.mktemp("occl")
    cache = {}

    def get(e):
        if e["name"] not in cache:
            hs = rtm.HostScene.load(S.scene_file(e, tmp))
            try:
                sc = R.RefScene.from_host(hs)
                rays = genray(oracle, hs.cam, hs.fov, e["W"], e["H"], e["spp"])
            finally:
                hs.close()
            cache[e["name"]] = (sc, rays, R.walk(sc, rays, mode="closest"))
        return cache[e["name"]]
    return get


# ------------------------------------------------------------------ 1. the restatement against the reference
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(walked, name):
    for e in frames_of(META["cases"][name]):
        sc, rays, res = walked(e)
        S.check_rec11(R.rec11(res), e, cols=GEOM_COLS, what="occlusion_ref closest mode")
        assert int(res["hit"].sum()) == e["hit_samples"]
        occ = R.walk(sc, rays, None, mode="any")["occluded"]
        np.testing.assert_array_equal(occ, res["hit"], err_msg=f"{e['name']}: occlusion over (-inf, +inf) vs the fixture's hit")
        inf = np.tile(np.array([-np.inf, np.inf], np.float32), (rays.shape[0], 1))
        np.testing.assert_array_equal(R.walk(sc, rays, inf, mode="any")["occluded"], occ)


# ------------------------------------------------------------------ 2. the implication on derived intervals
@pytest.mark.parametrize("name", CASES)
def test_occluded_implies_a_closest_hit_before_tmax(walked, name):
    """tmin = -inf, tmax in {t_ref, nextafter(t_ref, +inf), 0.5 t_ref, +inf} on every fixture ray with a hit:
    occluded => ref.hit && ref.t < tmax, so tmax = t_ref gives 0 on every ray; the converse may fail on at most 1 %
    of the view's hit rays (include/rt_tracer.h: a hit accepted in a cell the ray enters at or after tmax)."""
    for e in frames_of(META["cases"][name]):
        sc, rays, res = walked(e)
        h = res["hit"]
        if not h.any():
            continue
        r, t = rays[h], res["t"][h]
        for label, tmax in (("t_ref", t), ("nextafter", np.nextafter(t, np.float32(np.inf))),
                            ("half", (np.float32(0.5) * t).astype(np.float32)), ("inf", np.full_like(t, np.inf))):
            tmm = np.stack([np.full_like(t, -np.inf), tmax], axis=1)
            occ = R.walk(sc, r, tmm, mode="any")["occluded"]
            implied = t < tmax
            assert not (occ & ~implied).any(), (e["name"], label, int((occ & ~implied).sum()))
            conv = int((implied & ~occ).sum())
            print(f"{e['name']} tmax={label}: {int(occ.sum())} occluded of {t.size} hit rays, converse fails on {conv}")
            if label == "t_ref":
                assert not occ.any()
            assert conv <= CONVERSE_CAP * t.size, (e["name"], label, conv, t.size)


def test_restatement_interval_rules():
    """One triangle in a one-cell-thick box, by hand: the strict bounds, tmin past the only hit, rule 3, and the
    zero-without-a-walk cases."""
    tris = np.array([[[-1, -1, 0.5], [1, -1, 0.5], [0, 1, 0.5]], [[-1, -1, 0], [-0.9, -1, 0], [-1, -0.9, 0]],
                     [[1, 1, 1], [0.9, 1, 1], [1, 0.9, 1]]], np.float32)
    v, t = S.mesh_of(tris)
    hs = rtm.HostScene.from_mesh(v, t, 45.0, np.eye(4, dtype=np.float32).reshape(16), grid_res=8)
    try:
        sc = R.RefScene.from_host(hs)
    finally:
        hs.close()
    ray = np.array([[0.0, -0.5, 2.0, 0.0, 0.0, -1.0]], np.float32)
    c = R.walk(sc, ray, mode="closest")
    assert c["hit"][0] and c["tri"][0] == 0
    tr = c["t"][0]
    assert abs(tr - 1.5) < 1e-6
    inf = np.float32(np.inf)

    def occ(tmin, tmax, r=ray):
        return bool(R.walk(sc, r, np.array([[tmin, tmax]], np.float32), mode="any")["occluded"][0])

    assert occ(-inf, inf) and occ(0.0, inf) and occ(-inf, np.nextafter(tr, inf)) and occ(np.nextafter(tr, -inf), inf)
    assert not occ(-inf, tr) and not occ(tr, inf) and not occ(-inf, 0.5 * tr) and not occ(tr, tr) and not occ(2.0, 1.0)
    assert not occ(np.nan, inf) and not occ(-inf, np.nan)
    bad = ray.copy()
    bad[0, 4] = np.nan
    assert not occ(-inf, inf, bad)
    # rule 3 ends the walk: fewer cells than the closest-hit walk takes to reach the triangle
    short = R.walk(sc, ray, np.array([[-inf, 0.5 * tr]], np.float32), mode="any")
    assert 0 < short["steps"][0] < c["steps"][0]


# ------------------------------------------------------------------ 3. the ABI surface and the argument checks
def test_symbol_signature_and_python_method():
    L = ctypes.CDLL(os.path.join(PKG_DIR, "librt_tracer.so"))
    assert hasattr(L, "rt_occluded_rays_device")
    assert "rt_occluded_rays_device" in rtm.TRACER_SYMBOLS
    src = open(os.path.join(ROOT, "include", "rt_tracer.h")).read()
    assert re.search(r"int\s+rt_occluded_rays_device\(rt_scene \*scene, const rt_ray \*d_rays, const float \*d_tminmax, "
                     r"uint32_t n,\s*uint32_t flags, uint8_t \*d_occluded, void \*hip_stream\);", src)
    assert callable(getattr(rtm.GpuScene, "occluded", None))
    assert rtm.tracer_lib().rt_abi_version() == 8          # an addition bound behind hasattr: no ABI bump
    assert len(rtm.tracer_lib().rt_occluded_rays_device.argtypes) == 7


def test_occluded_rejects_bad_arguments_before_the_device():
    L = rtm.tracer_lib()
    ok = ctypes.c_void_p(0x1000)          # 8-byte aligned, never dereferenced by a rejected call

    def call(scene, rays, tmm, n, flags, occ):
        return L.rt_occluded_rays_device(scene, rays, tmm, n, flags, occ, None)

    assert call(None, ok, ok, 1, 0, ok) == 1 and "NULL" in last_error(L)
    assert call(FAKE, ok, ok, 1, rtm.RT_RAYS_COUNT, ok) == 1 and "RT_RAYS_COUNT" in last_error(L)
    assert call(FAKE, ok, ok, 1, rtm.RT_RAYS_COUNT | rtm.RT_RAYS_SORT, ok) == 1 and "RT_RAYS_COUNT" in last_error(L)
    assert call(FAKE, ok, ok, 1, 4, ok) == 1 and "unknown" in last_error(L)
    assert call(FAKE, ok, None, 1, rtm.RT_RAYS_SORT | 8, ok) == 1 and "unknown" in last_error(L)
    assert call(FAKE, ok, ok, 0x80000000, 0, ok) == 1 and "2^31" in last_error(L)
    assert call(FAKE, None, ok, 1, 0, ok) == 1 and "d_rays is NULL" in last_error(L)
    assert call(FAKE, ok, ok, 1, 0, None) == 1 and "d_occluded is NULL" in last_error(L)
    assert call(FAKE, ok, None, 1, 0, None) == 1 and "d_occluded is NULL" in last_error(L)
    for bad in (0x1004, 0x1001):
        b = ctypes.c_void_p(bad)
        assert call(FAKE, b, ok, 1, 0, ok) == 1 and "8-byte aligned" in last_error(L)
        assert call(FAKE, ok, b, 1, 0, ok) == 1 and "8-byte aligned" in last_error(L)
        assert call(FAKE, ok, b, 1, rtm.RT_RAYS_SORT, ok) == 1 and "8-byte aligned" in last_error(L)
    # n == 0: RT_OK, nothing touched (not even the scene), whatever the pointers
    assert call(FAKE, None, None, 0, 0, None) == 0
    assert call(FAKE, None, None, 0, rtm.RT_RAYS_SORT, None) == 0
    # ... but the flags are checked first
    assert call(FAKE, None, None, 0, rtm.RT_RAYS_COUNT, None) == 1


def test_python_layer_rejects_bad_inputs_before_any_launch():
    """Wrong dtype, shape, contiguity, host tensors and mixed kinds raise ValueError; the scene handle is never used."""
    import torch
    gs = object.__new__(rtm.GpuScene)
    gs._h, gs.device = None, 0
    good = np.zeros((4, 6), np.float32)
    for bad in (good.astype(np.float64), np.zeros((4, 5), np.float32), np.zeros(24, np.float32),
                np.zeros((4, 12), np.float32)[:, ::2], np.asfortranarray(good), [[0.0] * 6],
                torch.zeros((4, 6)), torch.zeros((4, 6), dtype=torch.float64), None):
        with pytest.raises(ValueError):
            gs.occluded(bad)
        with pytest.raises(ValueError):
            gs.occluded(bad, sort=True)
    tm = np.zeros((4, 2), np.float32)
    for bad in (tm.astype(np.float64), np.zeros((3, 2), np.float32), np.zeros((4, 3), np.float32), np.zeros(8, np.float32),
                np.zeros((4, 4), np.float32)[:, ::2], np.asfortranarray(tm), [[0.0, 1.0]] * 4, torch.zeros((4, 2))):
        with pytest.raises(ValueError):
            gs.occluded(good, bad)


# ------------------------------------------------------------------ 4. build guards of rt_occlusion.hip
@needs_hipcc
def test_occlusion_device_ir_has_no_contraction_or_fast_math(tmp_path):
    ll = tmp_path / "occl.ll"
    subprocess.run([HIPCC] + FLAGS + ["-emit-llvm", "-S", "-o", str(ll), OCC_SRC], check=True, capture_output=True)
    ir = ll.read_text()
    assert "k_occluded_rays" in ir
    assert "fmuladd" not in ir
    assert not re.search(r"\bllvm\.fma\.f64\b", ir)
    # no FMA of its own: the explicit ones stay in rtd::rcp_nr and box_exit_bound (test_build_guard.py counts them)
    for path in (OCC_SRC, os.path.join(PKG_DIR, "csrc", "rt_ray_common.h")):
        assert not [l for l in open(path).read().splitlines() if re.search(r"\bfmaf?\b|__builtin_fma", l)]
    for flag in (" contract ", " afn ", " arcp ", " nnan ", " ninf ", " nsz ", " reassoc ", " fast "):
        assert flag not in ir, flag
    assert "denormal-fp-math-f32" not in ir or '"denormal-fp-math-f32"="ieee' in ir


@needs_hipcc
def test_occlusion_kernels_use_no_scratch_no_lds_and_keep_8_waves(tmp_path):
    """The four k_occluded_rays instantiations (k_trace_rays' fast-arm variants | kVarAnyHit 16777216): scratch 0,
    LDS 0, 8 waves / SIMD by the compiler's estimate and by the hardware's admission rule, at most 64 VGPRs."""
    table = resource_table(OCC_SRC, ["-c", "-o", str(tmp_path / "occl.o")])
    print(table)
    # kVarAnyHit 16777216 | kVarRays 8388608 | kVarWaveGate 2 | kVarDistSkip 8 [| kVarFastRcp 2048] [| 4096 | 4]
    for key in ("k_occluded_raysILi25171982E", "k_occluded_raysILi25169934E", "k_occluded_raysILi25167882E",
                "k_occluded_raysILi25165834E"):
        assert [n for n in table if key in n], (key, sorted(table))
    assert len(table) == 4
    for n, (sg, vg, sc, oc, ld) in table.items():
        assert sc == 0 and ld == 0, (n, sc, ld)
        assert oc == 8 and 800 // (-(-sg // 16) * 16 + 16) >= 8 and vg <= 64, (n, sg, vg, oc)
