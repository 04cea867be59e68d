"""rt_march_rays_device without a GPU.

1. tests/march_ref.py against the reference's own RayMarch: the golden march crops and frames of scenes 1, 2 and 3
   (tests/golden/alt), their camera rays formed on the CPU by GenerateRay's restatement (tests/camera_matrices.py).
2. The ABI surface, and the argument checks that come before any device call.
3. The build guards of csrc/rt_march.hip, by the method of tests/test_distance_cpu.py.
4. The receding-miss stop: every ray its condition stops is a miss of march_ref run on, over five ray families.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import camera_matrices as C
import march_ref as M
import synth_scenes as S
from conftest import ALT_REC_DTYPE, PKG_DIR, ROOT, load_package, read_gz
from hip_remarks import FLAGS, HIPCC, last_error, needs_hipcc, resource_table

rtm = load_package()
MARCH_SRC = os.path.join(PKG_DIR, "csrc", "rt_march.hip")
FAKE = ctypes.c_void_p(1)            # a scene handle the rejected calls never dereference
F = np.float32


# ------------------------------------------------------------------ 1. march_ref against the reference's RayMarch
def crop_rays(cam16, fov, W, H, smp, x0, y0, w, h):
    """C.generate_rays' rays of the pixels [x0, x0 + w) x [y0, y0 + h) of a W x H frame, order (y, x, sample):
    a frame of w x h pixels has the same rays once its pixel coordinates are shifted, so the formula is restated
    here for the shifted coordinates (and compared with generate_rays below)."""
    m = np.asarray(cam16, F).reshape(4, 4)
    smp = np.asarray(smp, F).reshape(-1, 2)
    y, x, s = [a.reshape(-1) for a in np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), np.arange(smp.shape[0]),
                                                  indexing="ij")]
    fxs, aspect = C.fov_xs_of(fov), F(W) / F(H)
    with np.errstate(all="ignore"):
        cx = ((x.astype(F) + smp[s, 0]) / F(W) * F(2.0) - F(1.0)) * fxs
        cy = ((y.astype(F) + smp[s, 1]) / F(H) * F(2.0) - F(1.0)) * fxs / aspect
        cz = np.full_like(cx, F(-1.0))
        d = F(0.0) + cx * cx
        d = d + cy * cy
        d = d + cz * cz
        ln = F(1.0) / np.sqrt(d)
        px, py, pz = cx * ln, cy * ln, cz * ln
        rays = np.zeros((x.size, 6), F)
        for k in range(3):
            rays[:, k] = F(0.0) * m[0, k] + F(0.0) * m[1, k] + F(0.0) * m[2, k] + m[3, k]
            rays[:, 3 + k] = px * m[0, k] + py * m[1, k] + pz * m[2, k]
    return rays


@pytest.fixture(scope="module")
def host_scenes():
    cache = {}

    def get(sid):
        if sid not in cache:
            hs = rtm.HostScene.load(sid)
            v, t = hs.mesh()
            cache[sid] = (hs, M.D.triangles_of(v, t))
        return cache[sid]
    yield get
    for hs, _ in cache.values():
        hs.close()


def test_crop_rays_are_generate_rays():
    cam = S.look((0.3, 0.2, 3.0), (0.0, 0.1, 0.0))
    smp = rtm.sample_table(4)
    full = C.generate_rays(cam, 51.0, 24, 14, smp).reshape(14, 24, 4, 6)
    got = crop_rays(cam, 51.0, 24, 14, smp, 5, 3, 8, 6)
    np.testing.assert_array_equal(got.view(np.uint32), full[3:9, 5:13].reshape(-1, 6).view(np.uint32))


MARCH_CROPS = ["march_scene1_952_532_8x8", "march_scene2_952_532_8x8", "march_scene3_952_532_8x8",
               "march_scene1_1500_300_8x4", "march_scene3_1500_300_8x4"]


def check_against_golden_records(rec, exp, what):
    """march records against the reference's alt-samples records: hit, t bits and steps; a golden miss would carry
    t = 0 and 128 steps, which is steps = 0 here."""
    hit = exp["hit"] == 1
    np.testing.assert_array_equal(rec["steps"] != 0, hit, err_msg=what)
    np.testing.assert_array_equal(rec["t"][hit].view(np.uint32), exp["t"][hit].view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(rec["steps"][hit], exp["steps"][hit], err_msg=what)
    assert (exp["steps"][~hit] == 128).all() and (exp["t"][~hit] == 0).all(), what
    miss = rec[~hit]
    assert (miss["t"] == 0).all() and (miss["dist"] == 0).all() and (miss["tri"] == M.NOTRI).all(), what


@pytest.mark.parametrize("name", MARCH_CROPS)
def test_march_ref_on_the_golden_crops(oracle, golden_alt, host_scenes, name):
    c = next(x for x in golden_alt["crops"] if x["name"] == name)
    hs, tris = host_scenes(c["scene"])
    rays = crop_rays(hs.cam, hs.fov, c["W"], c["H"], rtm.sample_table(c["spp"]), c["x0"], c["y0"], c["w"], c["h"])
    rec = M.march(oracle, rays, tris)
    exp = read_gz(f"alt/{name}.rec.gz", ALT_REC_DTYPE)
    check_against_golden_records(rec, exp, name)
    assert (rec["dist"] < F(1e-3)).all() and (rec["tri"] < tris.shape[0]).all()


MARCH_FRAMES = ["march_scene1_48x27x1", "march_scene2_48x27x1", "march_scene3_48x27x1", "march_scene1_64x48x4",
                "march_scene3_31x19x2"]


@pytest.mark.parametrize("name", MARCH_FRAMES)
def test_march_ref_on_the_golden_frames(oracle, golden_alt, host_scenes, name):
    """The frames hold what the crops lack: misses (shaded by the row, renderer.cpp:121)."""
    f = next(x for x in golden_alt["frames"] if x["name"] == name)
    hs, tris = host_scenes(f["scene"])
    rays = C.generate_rays(hs.cam, hs.fov, f["W"], f["H"], rtm.sample_table(f["spp"]))
    rec = M.march(oracle, rays, tris)
    pix = M.frame_pixels(rec, f["W"], f["H"], f["spp"])
    gold = read_gz(f"alt/{name}.bgra.gz", "<u4")
    np.testing.assert_array_equal(pix & 0xFFFFFF, gold & 0xFFFFFF, err_msg=name)
    print(f"{name}: {int((rec['steps'] != 0).sum())} of {rec.size} samples hit, steps up to {rec['steps'].max()}")


# ------------------------------------------------------------------ 2. the interface
def test_symbols_struct_and_constants():
    L = ctypes.CDLL(os.path.join(PKG_DIR, "librt_tracer.so"))
    assert hasattr(L, "rt_march_rays_device") and "rt_march_rays_device" in rtm.TRACER_SYMBOLS
    src = open(os.path.join(ROOT, "include", "rt_tracer.h")).read()
    assert re.search(r"typedef struct rt_march_hit \{ float t; float dist; uint32_t tri; uint32_t steps; \} rt_march_hit;", src)
    assert re.search(r"typedef struct rt_march_params \{ uint32_t max_steps; float min_dist; \} rt_march_params;", src)
    assert re.search(r"RT_MARCH_EXHAUSTIVE\s*=\s*1\b", src) and re.search(r"RT_MARCH_SORT\s*=\s*2\b", src)
    assert (rtm.RT_MARCH_EXHAUSTIVE, rtm.RT_MARCH_SORT) == (1, 2)
    T = rtm.tracer_lib()
    assert T.rt_abi_version() == 8                         # additions bound behind hasattr: no ABI bump
    assert len(T.rt_march_rays_device.argtypes) == 7
    assert rtm.MARCH_HIT_DTYPE.itemsize == 16 and rtm.MARCH_HIT_DTYPE.names == ("t", "dist", "tri", "steps")
    assert [rtm.MARCH_HIT_DTYPE.fields[k][1] for k in rtm.MARCH_HIT_DTYPE.names] == [0, 4, 8, 12]
    assert rtm.MARCH_HIT_DTYPE == M.HIT_DTYPE
    assert ctypes.sizeof(rtm.MarchHitRec) == 16 and ctypes.sizeof(rtm.MarchParams) == 8
    assert [getattr(rtm.MarchHitRec, k).offset for k in ("t", "dist", "tri", "steps")] == [0, 4, 8, 12]
    assert rtm.MarchHit._fields == ("hit", "t", "dist", "tri", "steps", "raw")
    assert callable(getattr(rtm.GpuScene, "march", None))
    kp = open(os.path.join(PKG_DIR, "csrc", "rt_kparams.h")).read()
    assert int(re.search(r"constexpr uint32_t kMarchMaxSteps = (\d+);", kp).group(1)) == rtm.MARCH_MAX_STEPS == 4096
    # both kernels over the hierarchy take the sweep from the one header
    for tu in ("rt_distance.hip", "rt_march.hip"):
        text = open(os.path.join(PKG_DIR, "csrc", tu)).read()
        assert '#include "rt_dist_sweep.h"' in text and "void take(" not in text and "bool node_needed(" not in text


def test_c_abi_rejects_bad_arguments_before_the_device():
    L = rtm.tracer_lib()
    ok = ctypes.c_void_p(0x1000)

    def call(scene=FAKE, rays=ok, n=4, params=None, flags=0, out=ok):
        p = ctypes.byref(rtm.MarchParams(*params)) if params is not None else None
        return L.rt_march_rays_device(scene, rays, n, p, flags, out, None)

    assert call(scene=None) == 1 and "scene is NULL" in last_error(L)
    assert call(rays=None) == 1 and "d_rays is NULL" in last_error(L)
    assert call(out=None) == 1 and "d_out is NULL" in last_error(L)
    for bad in (0x1001, 0x1002, 0x1004):
        assert call(rays=ctypes.c_void_p(bad)) == 1 and "8-byte" in last_error(L)
        assert call(out=ctypes.c_void_p(bad)) == 1 and "8-byte" in last_error(L)
    for flags in (4, 8, 1 | 4, 0x80000000, 0xFFFFFFFF):
        assert call(flags=flags) == 1 and "unknown rt_march_flags" in last_error(L)
    for steps in (0, 4097, 0xFFFFFFFF):
        assert call(params=(steps, 1e-3)) == 1 and "max_steps" in last_error(L)
    assert call(params=(128, float("nan"))) == 1 and "min_dist is NaN" in last_error(L)
    assert call(n=0x80000000) == 1 and "2^31" in last_error(L)
    # n == 0 is RT_OK before any pointer is looked at, with every legal parameter
    assert call(n=0, rays=None, out=None) == 0
    for p in ((1, 0.0), (4096, -1.0), (128, float("inf")), (128, float("-inf"))):
        assert call(n=0, rays=None, out=None, params=p) == 0
    assert call(n=0, params=(0, 1e-3)) == 1


def test_python_layer_rejects_bad_inputs_before_any_launch():
    import torch
    gs = object.__new__(rtm.GpuScene)
    gs._h, gs.device = None, 0
    good = np.zeros((5, 6), np.float32)
    for bad in (good.astype(np.float64), good.reshape(-1), good[:, :5], np.zeros((5, 7), np.float32), good[::2],
                np.asfortranarray(np.zeros((5, 6), np.float32)), good.tolist(), None, "x",
                torch.zeros((5, 6), dtype=torch.float32), torch.zeros((5, 6), dtype=torch.float64),
                torch.zeros((5, 12), dtype=torch.float32)[:, :6], torch.zeros((30,), dtype=torch.float32)):
        with pytest.raises(ValueError):
            gs.march(bad)
    for kw in ({"max_steps": 0}, {"max_steps": 4097}, {"max_steps": -1}, {"max_steps": 1.5}, {"max_steps": True},
               {"min_dist": float("nan")}, {"min_dist": "x"}, {"min_dist": None}):
        with pytest.raises(ValueError):
            gs.march(good, **kw)


# ------------------------------------------------------------------ 3. build guards of rt_march.hip
@needs_hipcc
def test_march_device_ir_has_no_contraction_or_fast_math(tmp_path):
    ll = tmp_path / "march.ll"
    subprocess.run([HIPCC] + FLAGS + ["-emit-llvm", "-S", "-o", str(ll), MARCH_SRC], check=True, capture_output=True)
    ir = ll.read_text()
    assert "k_march_rays" in ir
    assert "fmuladd" not in ir
    assert not re.search(r"\bllvm\.fma\.", ir)
    for src in (MARCH_SRC, os.path.join(PKG_DIR, "csrc", "rt_dist_sweep.h")):
        assert not [l for l in open(src).read().splitlines() if re.search(r"\bfmaf?\b|__builtin_fma", l)]
    for flag in (" contract ", " afn ", " arcp ", " nnan ", " ninf ", " nsz ", " reassoc ", " fast "):
        assert flag not in ir, flag
    assert "denormal-fp-math-f32" not in ir or '"denormal-fp-math-f32"="ieee' in ir


# (TotalSGPRs, VGPRs, waves / SIMD by the compiler's estimate); DESIGN.md §4.35 quotes them
MARCH_KERNELS = {"k_march_raysILb0E": (94, 57, 8), "k_march_raysILb1E": (47, 23, 8)}


@needs_hipcc
def test_march_kernels_use_no_scratch_no_lds_and_keep_their_registers(tmp_path):
    table = resource_table(MARCH_SRC, ["-c", "-o", str(tmp_path / "march.o")],
                           also=(r" AGPRs: (\d+)", r"VGPRs Spill: (\d+)"))
    assert len(table) == 2
    print(table)
    for key, want in MARCH_KERNELS.items():
        hit = [n for n in table if key in n]
        assert len(hit) == 1, (key, sorted(table))
        sg, vg, sc, oc, ld, ag, vs = table[hit[0]]
        assert sc == 0 and ld == 0 and vs == 0, (key, sc, ld, vs)
        assert vg + ag <= 64 and oc >= 8, (key, vg, ag, oc)
        assert (sg, vg, oc) == want, (key, (sg, vg, oc), want)


# ------------------------------------------------------------------ 4. the receding-miss stop
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(1))[:, None]


def stop_families(tris, n_each, seed):
    """{family: rays f32 [n, 6]} around a mesh's vertex box: leaving it head-on, grazing a face, parallel to a face
    just outside it, starting 1,024 and 2^20 diagonals away, and one set of directions scaled by 2^-10 ... 2^10."""
    r = np.random.Generator(np.random.PCG64(seed))
    lo, hi, _ = M.vertex_box(tris)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    mid, ext = 0.5 * (lo + hi), hi - lo
    diag = float(np.sqrt((ext * ext).sum()))
    fam = {}
    # head-on: from a point of the box's surface (or a little outside it) along its outward direction
    p = r.uniform(lo, hi, (n_each, 3))
    ax, sg = r.integers(0, 3, n_each), r.integers(0, 2, n_each)
    p[np.arange(n_each), ax] = np.where(sg == 1, hi[ax], lo[ax]) + (2 * sg - 1) * r.uniform(0.0, 0.05, n_each) * diag
    d = unit(p - mid + 0.2 * diag * r.normal(size=(n_each, 3)))
    fam["head_on"] = np.concatenate([p, d], 1)
    # grazing: from outside towards a point of a face, nearly in the face's plane
    q = r.uniform(lo, hi, (n_each, 3))
    ax = r.integers(0, 3, n_each)
    q[np.arange(n_each), ax] = hi[ax]
    tang = r.normal(size=(n_each, 3))
    tang[np.arange(n_each), ax] = r.uniform(-0.02, 0.02, n_each)
    tang = unit(tang)
    fam["grazing"] = np.concatenate([q - 1.5 * diag * tang, tang], 1)
    # parallel: along an axis, a little outside the face of another axis
    q = r.uniform(lo - 0.5 * ext, hi, (n_each, 3))
    ax = r.integers(0, 3, n_each)
    q[np.arange(n_each), ax] = hi[ax] + r.uniform(0.01, 0.2, n_each) * diag
    d = np.zeros((n_each, 3))
    d[np.arange(n_each), (ax + 1 + r.integers(0, 2, n_each)) % 3] = 1.0
    fam["parallel"] = np.concatenate([q, d], 1)
    # far: half towards the box, half anywhere
    for name, k in (("far_1024", 1024.0), ("far_2^20", float(2 ** 20))):
        o = mid + k * diag * unit(r.normal(size=(n_each, 3)))
        aim = unit(r.uniform(lo, hi, (n_each, 3)) - o)
        anyd = unit(r.normal(size=(n_each, 3)))
        fam[name] = np.concatenate([o, np.where((np.arange(n_each) % 2 == 0)[:, None], aim, anyd)], 1)
    # scales: rays from near the box through and past it, every direction at every scale
    base = min(n_each, 8)
    o = mid + 1.2 * diag * unit(r.normal(size=(base, 3)))
    d = unit(r.uniform(lo, hi, (base, 3)) - o + 0.6 * diag * r.normal(size=(base, 3)))
    sc = 2.0 ** np.arange(-10, 11)
    fam["scales"] = np.concatenate([np.repeat(o, sc.size, 0), (d[:, None, :] * sc[None, :, None]).reshape(-1, 3)], 1)
    return {k: np.ascontiguousarray(v, np.float32) for k, v in fam.items()}


@pytest.mark.parametrize("min_dist", [1e-3, 0.05])
def test_every_ray_the_stop_condition_ends_is_a_miss(oracle, min_dist):
    """march_ref run to 512 steps with every step's positions recorded; the restated condition (march_ref.
    stop_condition: csrc/rt_march.hip's operations) evaluated at each: a ray it ends anywhere must be a miss of the
    whole run.  It must fire in every family, or the families test nothing."""
    tris = S.sparse(7, n=30)
    assert tris.shape[0] == 32
    vmin, vmax, scale = M.vertex_box(tris)
    total = 0
    for name, rays in stop_families(tris, 48, 11).items():
        trace = []
        rec = M.march(oracle, rays, tris, max_steps=512, min_dist=min_dist, trace=trace)
        stopped = np.zeros(rays.shape[0], bool)
        first = np.full(rays.shape[0], -1)
        for s, (idx, pos) in enumerate(trace):
            fire = M.stop_condition(rays[idx, :3], rays[idx, 3:], pos, vmin, vmax, scale, min_dist)
            new = idx[fire & ~stopped[idx]]
            first[new] = s
            stopped[new] = True
        bad = np.flatnonzero(stopped & (rec["steps"] != 0))
        print(f"{name} (min_dist {min_dist}): {rays.shape[0]} rays, {int((rec['steps'] != 0).sum())} hit, "
              f"{int(stopped.sum())} stopped (at steps {first[stopped].min() if stopped.any() else '-'} .. "
              f"{first.max()}), {bad.size} violations")
        assert bad.size == 0, (name, bad[:8], rays[bad[:8]], rec[bad[:8]], first[bad[:8]])
        assert stopped.any(), name
        # (every miss of these families recedes in the end: the condition finds all but those that march on the spot)
        total += int(stopped.sum())
    assert total > 100


def test_idle_share_counts_lane_steps():
    assert M.idle_share(np.full(128, 5), 128) == 0.0
    assert M.idle_share(np.array([0] * 64), 128) == 0.0
    s = np.array([1] * 63 + [0])                     # one miss keeps 63 finished lanes idle for 127 steps
    assert abs(M.idle_share(s, 128) - (1.0 - (63 + 128) / (64 * 128))) < 1e-12
