"""rt_distance_points_device without a GPU.

1. tests/distance_ref.py's reduce rule and tie rule against the reference's loop written out, on the 6,000 golden
   kat_dist cases regrouped as points x triangles.
2. tests/dist_tree_check.cpp over csrc/rt_dist_tree.h: the hierarchy's structure at every size where a level appears,
   and the cull bound lb - margin against the oracle's distances at every level, over five point families.
3. The ABI surface, and the argument checks that come before any device call.
4. The build guards of csrc/rt_distance.hip, by the method of tests/test_ao_cpu.py.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import distance_ref as D
import synth_scenes as S
from conftest import PKG_DIR, ROOT, load_kat, load_package
from hip_remarks import FLAGS, HIPCC, last_error, needs_hipcc, resource_table

rtm = load_package()
DIST_SRC = os.path.join(PKG_DIR, "csrc", "rt_distance.hip")
FAKE = ctypes.c_void_p(1)            # a scene handle the rejected calls never dereference
FLT_MAX = D.FLT_MAX


# ------------------------------------------------------------------ 1. the reduce rule and the tie rule
def loop_rule(row):
    """renderer.cpp:143-152 written out, and the lowest index whose distance equals the result."""
    dist = FLT_MAX
    for d in row:
        dist = d if d < dist else dist                  # std::min(dist, d)
    tri = D.NOTRI
    for j, d in enumerate(row):
        if d == dist:
            tri = j
            break
    return np.float32(dist), tri


def test_reduce_and_tie_rule_on_the_golden_distances(oracle):
    rin, want = load_kat("dist")
    assert rin.shape == (6000, 12)
    got = oracle.kat("dist", rin, 1)
    assert (got.view(np.uint32) == want.view(np.uint32)).all() or np.array_equal(got, want, equal_nan=True)
    d = np.ascontiguousarray(want.reshape(60, 100), np.float32)
    # every row twice over (each distance has an equal at j + 100: the lower index must win), and rows with the
    # values the loop never selects
    d = np.concatenate([d, d], axis=1)
    extra = d[:6].copy()
    extra[0, ::2] = np.nan
    extra[1, :] = np.nan
    extra[2, :] = np.inf
    extra[3, 5] = extra[3, 150] = 0.0
    extra[4, :] = FLT_MAX
    extra[5, :] = [np.nan, np.inf] * 100
    d = np.concatenate([d, extra])
    dist, tri = D.reduce_rule(d)
    assert dist.dtype == np.float32 and tri.dtype == np.uint32 and not np.isnan(dist).any()
    for i in range(d.shape[0]):
        wd, wt = loop_rule(d[i])
        assert dist[i].view(np.uint32) == wd.view(np.uint32) and tri[i] == wt, (i, dist[i], tri[i], wd, wt)
    assert (tri[:60] < 100).all()
    assert dist[61] == FLT_MAX and tri[61] == D.NOTRI and dist[62] == FLT_MAX and tri[62] == D.NOTRI
    assert dist[64] == FLT_MAX and tri[64] == 0           # d_j == FLT_MAX == dist: the rule names j
    assert dist[65] == FLT_MAX and tri[65] == D.NOTRI
    e, t = D.reduce_rule(np.zeros((3, 0), np.float32))
    assert (e == FLT_MAX).all() and (t == D.NOTRI).all()


# ------------------------------------------------------------------ 2. the hierarchy
@pytest.fixture(scope="module")
def tree_check(tmp_path_factory):
    """tests/dist_tree_check.cpp built once: with the address and undefined-behaviour sanitizers where this g++
    links them (a stand-alone program), else plain."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("dtree")
    exe = str(tmp / "dist_tree_check")
    src = os.path.join(ROOT, "tests", "dist_tree_check.cpp")
    base = [cxx, "-std=c++11", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, src]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)

    def run(tris, points, name):
        fin, fout = str(tmp / f"{name}.in"), str(tmp / f"{name}.out")
        with open(fin, "wb") as f:
            f.write(np.array([tris.shape[0], points.shape[0]], np.uint32).tobytes())
            f.write(np.ascontiguousarray(tris, np.float32).tobytes())
            f.write(np.ascontiguousarray(points, np.float32).tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout
        raw = np.fromfile(fout, np.uint32)
        nt, npts = tris.shape[0], points.shape[0]
        levels, order, pos, out = int(raw[0]), raw[1:1 + nt], 1 + nt, []
        for _ in range(levels):
            n = int(raw[pos])
            out.append(raw[pos + 1:pos + 1 + n * npts].view(np.float32).reshape(n, npts))
            pos += 1 + n * npts
        assert pos == raw.size
        return order, out
    return run


def scene8_with_degenerates():
    """Scene 8's 24,336 triangles with slivers, collinear and repeated-vertex triangles mixed in."""
    hs = rtm.HostScene.load(8)
    try:
        v, t = hs.mesh()
        tris = D.triangles_of(v, t).copy()
    finally:
        hs.close()
    assert tris.shape[0] == 24336
    for i in range(0, tris.shape[0], 97):
        tris[i, 2] = (tris[i, 0] + tris[i, 1]) * np.float32(0.5)                  # collinear
    for i in range(5, tris.shape[0], 101):
        tris[i, 1] = tris[i, 0]                                                  # a repeated vertex
    for i in range(11, tris.shape[0], 103):
        tris[i, 2] = tris[i, 1] + (tris[i, 1] - tris[i, 0]) * np.float32(1e-6)     # a sliver
    for i in range(17, tris.shape[0], 997):
        tris[i, 1] = tris[i, 2] = tris[i, 0]                                     # a point (NaN distances)
    return tris


def mesh_of_size(K):
    return S.sparse(41 + K, n=max(K, 1))[:K]


def check_bounds(oracle, tree_check, tris, n_each, name):
    pts = D.families(tris, n_each, 7)
    order, bounds = tree_check(tris, pts, name)
    d = D.all_distances(oracle, pts, tris)[:, order.astype(np.int64)]          # [np, nt] in sorted order
    nt = tris.shape[0]
    assert len(bounds) >= 1 and bounds[0].shape[0] == -(-nt // 32)
    span, worst = 32, 0
    for l, b in enumerate(bounds):
        assert b.shape[0] == -(-nt // span) and (l == len(bounds) - 1) == (b.shape[0] <= 32)
        for i in range(b.shape[0]):
            # the node's records partition [0, nt) by construction: [i span, (i + 1) span)
            lo = np.fmin.reduce(d[:, i * span:min(nt, (i + 1) * span)], axis=1, initial=FLT_MAX)
            bad = b[i] > lo
            worst += int(bad.sum())
            assert not bad.any(), (name, l, i, np.flatnonzero(bad)[:4], b[i][bad][:4], lo[bad][:4])
        span *= 32
    print(f"{name}: {nt} triangles, {[x.shape[0] for x in bounds]} nodes per level, {pts.shape[0]} points, "
          f"{worst} violations")
    return bounds


@pytest.mark.parametrize("K", [1, 31, 32, 33, 1023, 1024, 1025, 32767, 32768, 32769])
def test_tree_structure_and_bounds_at_level_edges(oracle, tree_check, K):
    tris = mesh_of_size(K)
    assert tris.shape[0] == K
    bounds = check_bounds(oracle, tree_check, tris, 24 if K <= 1025 else 4, f"k{K}")
    assert len(bounds) == (1 if K <= 1024 else 2 if K <= 32768 else 3)


def test_tree_bounds_on_the_killeroo_with_degenerates(oracle, tree_check):
    bounds = check_bounds(oracle, tree_check, scene8_with_degenerates(), 24, "scene8")
    assert [b.shape[0] for b in bounds] == [761, 24]


# ------------------------------------------------------------------ 3. the interface
def test_symbols_struct_and_constants():
    L = ctypes.CDLL(os.path.join(PKG_DIR, "librt_tracer.so"))
    assert hasattr(L, "rt_distance_points_device") and "rt_distance_points_device" in rtm.TRACER_SYMBOLS
    src = open(os.path.join(ROOT, "include", "rt_tracer.h")).read()
    assert re.search(r"typedef struct rt_point_dist \{ float dist; uint32_t tri; \} rt_point_dist;", src)
    assert re.search(r"RT_DIST_EXHAUSTIVE\s*=\s*1\b", src) and re.search(r"RT_DIST_SORT\s*=\s*2\b", src)
    assert (rtm.RT_DIST_EXHAUSTIVE, rtm.RT_DIST_SORT) == (1, 2)
    T = rtm.tracer_lib()
    assert T.rt_abi_version() == 8                         # additions bound behind hasattr: no ABI bump
    assert len(T.rt_distance_points_device.argtypes) == 7
    assert rtm.POINT_DIST_DTYPE.itemsize == 8 and rtm.POINT_DIST_DTYPE.names == ("dist", "tri")
    assert rtm.POINT_DIST_DTYPE.fields["dist"][1] == 0 and rtm.POINT_DIST_DTYPE.fields["tri"][1] == 4
    assert ctypes.sizeof(rtm.PointDistRec) == 8 and rtm.PointDistRec.dist.offset == 0 and rtm.PointDistRec.tri.offset == 4
    assert rtm.PointDist._fields == ("dist", "tri", "closest", "raw")
    assert callable(getattr(rtm.GpuScene, "distance", None))
    # the host-only header and the kernels agree on the constants they share
    kp = open(os.path.join(PKG_DIR, "csrc", "rt_kparams.h")).read()
    th = open(os.path.join(PKG_DIR, "csrc", "rt_dist_tree.h")).read()
    assert int(re.search(r"constexpr uint32_t kDistBlock = (\d+);", kp).group(1)) == \
        int(re.search(r"constexpr uint32_t kDistTreeBlock = (\d+);", th).group(1)) == 32
    assert int(re.search(r"constexpr uint32_t kDistLevels = (\d+);", kp).group(1)) == \
        int(re.search(r"constexpr uint32_t kDistMaxLevels = (\d+);", th).group(1))
    assert int(re.search(r"constexpr uint32_t kDistFan = (\d+);", th).group(1)) == 32


def test_c_abi_rejects_bad_arguments_before_the_device():
    L = rtm.tracer_lib()
    ok = ctypes.c_void_p(0x1000)

    def call(scene=FAKE, pts=ok, n=4, flags=0, out=ok, closest=None):
        return L.rt_distance_points_device(scene, pts, n, flags, out, closest, None)

    assert call(scene=None) == 1 and "scene is NULL" in last_error(L)
    assert call(pts=None) == 1 and "d_points is NULL" in last_error(L)
    assert call(out=None) == 1 and "d_out is NULL" in last_error(L)
    for bad in (0x1001, 0x1002, 0x1003):
        assert call(pts=ctypes.c_void_p(bad)) == 1 and "4-byte" in last_error(L)
        assert call(closest=ctypes.c_void_p(bad)) == 1 and "4-byte" in last_error(L)
    for bad in (0x1001, 0x1002, 0x1004):
        assert call(out=ctypes.c_void_p(bad)) == 1 and "8-byte" in last_error(L)
    for flags in (4, 8, 1 | 4, 0x80000000, 0xFFFFFFFF):
        assert call(flags=flags) == 1 and "unknown rt_dist_flags" in last_error(L)
    assert call(n=0x80000000) == 1 and "2^31" in last_error(L)
    # n == 0 is RT_OK before any pointer is looked at
    assert call(n=0, pts=None, out=None) == 0


def test_python_layer_rejects_bad_inputs_before_any_launch():
    import torch
    gs = object.__new__(rtm.GpuScene)
    gs._h, gs.device = None, 0
    good = np.zeros((5, 3), np.float32)
    for bad in (good.astype(np.float64), good.reshape(-1), good[:, :2], np.zeros((5, 4), np.float32), good[::2],
                np.asfortranarray(np.zeros((5, 3), np.float32)), good.tolist(), None, "x",
                torch.zeros((5, 3), dtype=torch.float32), torch.zeros((5, 3), dtype=torch.float64),
                torch.zeros((5, 6), dtype=torch.float32)[:, :3], torch.zeros((15,), dtype=torch.float32)):
        with pytest.raises(ValueError):
            gs.distance(bad)


# ------------------------------------------------------------------ 4. build guards of rt_distance.hip
@needs_hipcc
def test_distance_device_ir_has_no_contraction_or_fast_math(tmp_path):
    ll = tmp_path / "dist.ll"
    subprocess.run([HIPCC] + FLAGS + ["-emit-llvm", "-S", "-o", str(ll), DIST_SRC], check=True, capture_output=True)
    ir = ll.read_text()
    assert "k_distance_points" in ir and "k_point_keys" in ir
    assert "fmuladd" not in ir
    assert not re.search(r"\bllvm\.fma\.", ir)
    assert not [l for l in open(DIST_SRC).read().splitlines() if re.search(r"\bfmaf?\b|__builtin_fma", l)]
    for flag in (" contract ", " afn ", " arcp ", " nnan ", " ninf ", " nsz ", " reassoc ", " fast "):
        assert flag not in ir, flag
    assert "denormal-fp-math-f32" not in ir or '"denormal-fp-math-f32"="ieee' in ir


# (TotalSGPRs, VGPRs, waves / SIMD by the compiler's estimate); DESIGN.md §4.31 quotes them
DIST_KERNELS = {"k_distance_pointsILb0E": (85, 50, 8), "k_distance_pointsILb1E": (37, 38, 8), "k_point_keys": (18, 12, 8)}


@needs_hipcc
def test_distance_kernels_use_no_scratch_no_lds_and_keep_their_registers(tmp_path):
    table = resource_table(DIST_SRC, ["-c", "-o", str(tmp_path / "dist.o")])
    assert len(table) == 3
    print(table)
    for key, want in DIST_KERNELS.items():
        hit = [n for n in table if key in n]
        assert len(hit) == 1, (key, sorted(table))
        sg, vg, sc, oc, ld = table[hit[0]]
        assert sc == 0 and ld == 0, (key, sc, ld)
        assert (sg, vg, oc) == want, (key, (sg, vg, oc), want)
