"""rt_trace_rays_device / rt_primary_rays_device without a GPU: the ABI surface, the argument checks that
come before any device call, the Python layer's input validation, and the build guards of
csrc/rt_rays.hip (in the style of tests/test_build_guard.py).

The C entry points check every argument before they touch the scene, so the rejections are exercised with
a scene handle that is never dereferenced (as test_abi.py does for rth_framebuffer_create_multi).
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT, load_package
from hip_remarks import FLAGS, HIPCC, last_error, needs_hipcc, resource_table

rtm = load_package()
RAYS_SRC = os.path.join(PKG_DIR, "csrc", "rt_rays.hip")
FAKE = ctypes.c_void_p(1)            # a scene handle the rejected calls never dereference


def test_symbols_structs_and_constants():
    L = ctypes.CDLL(os.path.join(PKG_DIR, "librt_tracer.so"))
    assert hasattr(L, "rt_trace_rays_device") and hasattr(L, "rt_primary_rays_device")
    assert {"rt_trace_rays_device", "rt_primary_rays_device"} <= set(rtm.TRACER_SYMBOLS)
    # rt_ray is 24 bytes (six floats), rt_ray_hit 16 (tri, t, u, v), as the header declares them
    src = open(os.path.join(ROOT, "include", "rt_tracer.h")).read()
    assert re.search(r"typedef struct rt_ray\s*\{\s*float o\[3\];\s*float d\[3\];\s*\}\s*rt_ray;", src)
    assert re.search(r"typedef struct rt_ray_hit\s*\{\s*uint32_t tri;\s*float t, u, v;\s*\}\s*rt_ray_hit;", src)
    # the ctypes mirrors of the two structs, field by field, and the word counts the binding allocates by
    assert ctypes.sizeof(rtm.Ray) == 24 and ctypes.sizeof(rtm.RayHit) == 16
    assert (rtm.Ray.o.offset, rtm.Ray.d.offset) == (0, 12)
    assert [getattr(rtm.RayHit, k).offset for k in ("tri", "t", "u", "v")] == [0, 4, 8, 12]
    assert [rtm.RAY_HIT_DTYPE.fields[k][1] for k in ("tri", "t", "u", "v")] == [0, 4, 8, 12]
    assert rtm.RAY_WORDS * 4 == 24 and rtm.RAY_HIT_DTYPE.itemsize == 16 and rtm.RAY_HIT_WORDS * 4 == 16
    assert rtm.RAY_HIT_DTYPE.names == ("tri", "t", "u", "v")
    assert rtm.SAMPLE_REC_WORDS * 4 == rtm.SAMPLE_REC_DTYPE.itemsize
    vals = dict(re.findall(r"\b(RT_RAYS_[A-Z]+)\s*=\s*(\d+)", src))
    assert vals == {"RT_RAYS_COUNT": "1", "RT_RAYS_SORT": "2"}
    assert rtm.RT_RAYS_COUNT == 1 and rtm.RT_RAYS_SORT == 2
    assert rtm.tracer_lib().rt_abi_version() == 8          # the new entry points do not bump the ABI


def test_compiled_struct_layout(tmp_path):
    """sizeof / offsetof of rt_ray and rt_ray_hit as the host C compiler lays the header out: 24 and 16 bytes."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no host C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_tracer.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rt_ray), offsetof(rt_ray, d),\n'
                   '    sizeof(rt_ray_hit), offsetof(rt_ray_hit, tri), offsetof(rt_ray_hit, t), offsetof(rt_ray_hit, u),\n'
                   '    offsetof(rt_ray_hit, v), sizeof(rt_sample_rec)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True,
                   capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [24, 12, 16, 0, 4, 8, 12, 48]


def test_trace_rays_rejects_bad_arguments_before_the_device():
    L = rtm.tracer_lib()
    ok = ctypes.c_void_p(0x1000)          # 8-byte aligned, never dereferenced by a rejected call

    def call(scene, rays, n, flags, hits, recs):
        return L.rt_trace_rays_device(scene, rays, n, flags, hits, recs, None)

    assert call(None, ok, 1, 0, ok, None) == 1 and "NULL" in last_error(L)
    assert call(FAKE, ok, 1, 4, ok, None) == 1 and "unknown" in last_error(L)
    assert call(FAKE, ok, 1, rtm.RT_RAYS_SORT | 8, ok, None) == 1 and "unknown" in last_error(L)
    assert call(FAKE, ok, 1, rtm.RT_RAYS_SORT, ok, ok) == 1 and "d_recs without RT_RAYS_COUNT" in last_error(L)
    assert call(FAKE, ok, 1, 0, ok, ok) == 1 and "d_recs without RT_RAYS_COUNT" in last_error(L)
    assert call(FAKE, ok, 1, rtm.RT_RAYS_COUNT, ok, None) == 1 and "needs d_recs" in last_error(L)
    assert call(FAKE, ok, 0x80000000, 0, ok, None) == 1 and "2^31" in last_error(L)
    assert call(FAKE, None, 1, 0, ok, None) == 1 and "d_rays is NULL" in last_error(L)
    assert call(FAKE, ok, 1, 0, None, None) == 1 and "d_hits is NULL" in last_error(L)
    for bad in (0x1004, 0x1001):
        b = ctypes.c_void_p(bad)
        assert call(FAKE, b, 1, 0, ok, None) == 1 and "8-byte aligned" in last_error(L)
        assert call(FAKE, ok, 1, 0, b, None) == 1 and "8-byte aligned" in last_error(L)
        assert call(FAKE, ok, 1, rtm.RT_RAYS_COUNT, None, b) == 1 and "8-byte aligned" in last_error(L)
    # n == 0: RT_OK, nothing touched (not even the scene), whatever the pointers
    assert call(FAKE, None, 0, 0, None, None) == 0
    assert call(FAKE, None, 0, rtm.RT_RAYS_COUNT, None, ok) == 0
    assert call(FAKE, None, 0, rtm.RT_RAYS_SORT, None, None) == 0


def test_primary_rays_rejects_bad_arguments_before_the_device():
    L = rtm.tracer_lib()
    f = rtm.Frame()
    f.width, f.height, f.spp, f.fov = 8, 8, 1, 45.0
    assert L.rt_primary_rays_device(None, ctypes.byref(f), ctypes.c_void_p(0x1000), None) == 1
    assert L.rt_primary_rays_device(FAKE, ctypes.byref(f), None, None) == 1
    assert L.rt_primary_rays_device(FAKE, ctypes.byref(f), ctypes.c_void_p(0x1004), None) == 1
    assert "8-byte aligned" in last_error(L)
    assert L.rt_primary_rays_device(FAKE, None, ctypes.c_void_p(0x1000), None) == 1
    f.width = 0
    assert L.rt_primary_rays_device(FAKE, ctypes.byref(f), ctypes.c_void_p(0x1000), None) == 1
    f.width, f.height, f.spp = 65536, 65536, 1          # 2^32 rays
    assert L.rt_primary_rays_device(FAKE, ctypes.byref(f), ctypes.c_void_p(0x1000), None) == 1
    assert "2^31" in last_error(L)


def test_python_layer_rejects_bad_rays_before_any_launch():
    """Wrong dtype, shape, contiguity and host tensors raise ValueError; the scene handle is never used."""
    import torch
    gs = object.__new__(rtm.GpuScene)
    gs._h, gs.device = None, 0
    good = np.zeros((4, 6), np.float32)
    for bad in (good.astype(np.float64), np.zeros((4, 5), np.float32), np.zeros(24, np.float32),
                np.zeros((4, 12), np.float32)[:, ::2], np.asfortranarray(good), [[0.0] * 6],
                torch.zeros((4, 6)), torch.zeros((4, 6), dtype=torch.float64), None):
        with pytest.raises(ValueError):
            gs.trace_rays(bad)
        with pytest.raises(ValueError):
            gs.trace_rays(bad, count=True)


# ------------------------------------------------------------------ build guards of rt_rays.hip
@needs_hipcc
def test_rays_device_ir_has_no_contraction_or_fast_math(tmp_path):
    ll = tmp_path / "rays.ll"
    subprocess.run([HIPCC] + FLAGS + ["-emit-llvm", "-S", "-o", str(ll), RAYS_SRC], check=True, capture_output=True)
    ir = ll.read_text()
    assert "k_trace_rays" in ir and "k_primary_rays" in ir
    assert "fmuladd" not in ir
    assert not re.search(r"\bllvm\.fma\.f64\b", ir)
    # no FMA of its own: the explicit ones stay in rtd::rcp_nr and box_exit_bound (test_build_guard.py counts them)
    assert not [l for l in open(RAYS_SRC).read().splitlines() if re.search(r"\bfmaf?\b|__builtin_fma", l)]
    for flag in (" contract ", " afn ", " arcp ", " nnan ", " ninf ", " nsz ", " reassoc ", " fast "):
        assert flag not in ir, flag
    assert "denormal-fp-math-f32" not in ir or '"denormal-fp-math-f32"="ieee' in ir


@needs_hipcc
def test_rays_kernels_use_no_scratch_no_lds_and_keep_8_waves(tmp_path):
    """Every k_trace_rays instantiation (the counting arm and the four fast-arm variants), k_primary_rays and
    RT_RAYS_SORT's k_ray_keys:
    scratch 0, LDS 0, and 8 waves / SIMD both by the compiler's estimate and by the hardware's admission rule
    800 // (ceil(sgpr / 16) * 16 + 16) -- the per-lane origin costs no wave."""
    table = resource_table(RAYS_SRC, ["-c", "-o", str(tmp_path / "rays.o")])
    print(table)
    rays = {n: v for n, v in table.items() if "k_trace_rays" in n}
    # kVarRays 8388608 | kVarWaveGate 2 | kVarDistSkip 8 [| kVarFastRcp 2048] [| kVarPackedRem 4096 | kVarSkipRun 4]
    for key in ("k_trace_raysILi0ELb1E", "k_trace_raysILi8394766ELb0E", "k_trace_raysILi8392718ELb0E",
                "k_trace_raysILi8390666ELb0E", "k_trace_raysILi8388618ELb0E"):
        assert [n for n in rays if key in n], (key, sorted(rays))
    assert len(rays) == 5 and len(table) == 7
    for n, (sg, vg, sc, oc, ld) in list(rays.items()) + [(n, v) for n, v in table.items() if "k_primary_rays" in n or "k_ray_keys" in n]:
        assert sc == 0 and ld == 0, (n, sc, ld)
        assert oc == 8 and 800 // (-(-sg // 16) * 16 + 16) >= 8 and vg <= 64, (n, sg, vg, oc)
