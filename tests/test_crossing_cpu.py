"""rt_crossing_rays_device without a GPU: the contract's restatement and the build.

1. tests/crossing_ref.py's walk_count (the numpy f32 restatement of the walk in include/rt_tracer.h) is anchored before
   the GPU tests use it as their yardstick, on the 21 synthetic views' camera rays (every 7th sample) and the ray
   families of tests/golden/rays (every ray the fixture pins; every third on scene8):
     a. count <= B and front <= B_front on every ray, family H included -- B from the oracle's own IntersectRayTri
        (orc_kat_ray_tri) over every (ray, triangle) pair, B_front its hits with det > 0;
     b. count == B and front == B_front on all but at most 1 % (test_occlusion_cpu.CONVERSE_CAP) of each view's or
        family's rays with B > 0, families A-G; the observed number is printed;
     c. count >= 1 implies occlusion_ref.walk(mode="any"), over NULL, (-inf, +inf) and ray_sets.intervals;
     d. no (ray, triangle) pair counted twice, and no walk's crossing times decreased.
2. Known answers by hand, and the closed cube and 2,048-triangle sphere: parity and winding equal the analytic inside at
   every point outside a shell of 1e-3 about the cube's face planes / 0.02 about the sphere's radius.
3. The ABI surface, the argument checks of the C entry and of the Python layer.
4. Build guards of rt_crossings.hip: no contraction or fast-math in the IR; no scratch, no LDS, and the waves per SIMD
   the compiler reports for the four instantiations.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import crossing_ref as C
import occlusion_ref as R
import ray_sets as RS
import synth_scenes as S
from conftest import PKG_DIR, ROOT, load_package
from hip_remarks import FLAGS, HIPCC, last_error, needs_hipcc, resource_table
from test_occlusion_cpu import CONVERSE_CAP, FAKE, genray

rtm = load_package()
META = S.meta()
CASES = sorted(META["cases"])
RAYS_META = RS.meta()
SRC = os.path.join(PKG_DIR, "csrc", "rt_crossings.hip")
INF = np.float32(np.inf)
VIEW_STRIDE = 7                      # camera rays sampled per view: 62 x 46 x 4 / 7 = 1,630
EQUAL_FAMILIES = RS.NAMES[:-1]       # A-G are held to equality; H (origins 2^6 .. 2^20 diagonals away) to count <= B


def oracle_counts(oracle, sc, rays, tminmax=None, chunk=1 << 18):
    """B, B_front per ray from orc_kat_ray_tri's hit and t over every (ray, triangle) pair; the det whose sign
    B_front reads is crossing_ref.tri_det's (the oracle hands none out)."""
    n, nt = rays.shape[0], sc.v0.shape[0]
    tmin, tmax = C.intervals_of(n, tminmax)
    valid = np.isfinite(rays).all(1) & (tmin < tmax)
    B, Bf = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    tri = np.concatenate([sc.v0, sc.v1, sc.v2], axis=1).astype(np.float32)          # [nt, 9]
    per = max(1, chunk // nt)
    with np.errstate(all="ignore"):
        for lo in range(0, n, per):
            hi = min(n, lo + per)
            r = np.repeat(np.arange(lo, hi), nt)
            ti = np.tile(np.arange(nt), hi - lo)
            rin = np.zeros((r.size, 18), np.float32)
            rin[:, :6] = rays[r]
            rin[:, 6:15] = tri[ti]
            out = oracle.kat("ray_tri", rin, 8)
            h, t = out[:, 0].view(np.uint32) == 1, out[:, 1]
            ok = h & valid[r] & (tmin[r] < t) & (t < tmax[r])
            det = C.tri_det(rays[r[ok], 3:], sc.v0[ti[ok]], sc.v1[ti[ok]], sc.v2[ti[ok]])
            np.add.at(B, r[ok], 1)
            np.add.at(Bf, r[ok][det > np.float32(0)], 1)
    return B, Bf


@pytest.fixture(scope="module")
def anchored(oracle, tmp_path_factory):
    """Per ray set -- ("view", case) or ("rays", scene) -- computed once and never changed: the RefScene, the rays,
    the pinned mask, the family bounds, per-ray intervals, the restatement's result over (-inf, +inf) with its
    counted pairs, and the oracle's B, B_front."""
    tmp = tmp_path_factory.mktemp("crossings")
    cache = {}

    def get(kind, name):
        if (kind, name) not in cache:
            if kind == "view":
                e = META["cases"][name]
                hs = rtm.HostScene.load(S.scene_file(e, tmp))
                try:
                    sc = R.RefScene.from_host(hs)
                    rays = genray(oracle, hs.cam, hs.fov, e["W"], e["H"], e["spp"])[::VIEW_STRIDE]
                finally:
                    hs.close()
                rays = np.ascontiguousarray(rays)
                keep = np.ones(rays.shape[0], bool)
                groups = {"view": (0, rays.shape[0])}
                c = R.walk(sc, rays, mode="closest")
                rec8 = np.zeros((rays.shape[0], 8), np.uint32)
                rec8[:, 0], rec8[:, 2] = c["hit"], c["t"].view(np.uint32)
            else:
                hs = rtm.HostScene.load(RS.scene_file(name, tmp))
                try:
                    sc = R.RefScene.from_host(hs)
                finally:
                    hs.close()
                rays, rec8 = RS.load(name)
                rays = np.ascontiguousarray(rays)
                keep = RS.pinned(RAYS_META["scenes"][name])
                if name == "scene8":
                    keep &= np.arange(rays.shape[0]) % 3 == 0
                groups = RS.bounds()
            tmm = RS.intervals(rays, rec8, sc.diagonal())
            idx = np.flatnonzero(keep)
            res = C.walk_count(sc, rays[idx], pairs=True)
            B, Bf = oracle_counts(oracle, sc, rays[idx])
            cache[(kind, name)] = dict(sc=sc, rays=rays, idx=idx, groups=groups, tmm=tmm, res=res, B=B, Bf=Bf)
        return cache[(kind, name)]
    return get


SETS = [("view", n) for n in CASES] + [("rays", s) for s in RS.SCENES]


# ------------------------------------------------------------------ 1. the restatement, anchored
@pytest.mark.parametrize("kind,name", SETS)
def test_count_never_exceeds_the_brute_force_and_equals_it_off_cell_planes(anchored, kind, name):
    a = anchored(kind, name)
    cnt, fr, B, Bf, idx = a["res"]["count"], a["res"]["front"], a["B"], a["Bf"], a["idx"]
    assert (cnt <= B).all() and (fr <= Bf).all() and (fr <= cnt).all(), (kind, name)
    for g, (lo, hi) in a["groups"].items():
        m = (idx >= lo) & (idx < hi) & (B > 0)
        short = int(((cnt != B) | (fr != Bf))[m].sum())
        print(f"{kind} {name} {g}: {int(m.sum())} rays with B > 0 (most crossings {int(B[m].max()) if m.any() else 0}), "
              f"count != B or front != B_front on {short}")
        if g in EQUAL_FAMILIES or kind == "view":
            assert short <= CONVERSE_CAP * int(m.sum()), (kind, name, g, short, int(m.sum()))


@pytest.mark.parametrize("kind,name", SETS)
def test_no_pair_counts_twice_and_no_crossing_sequence_decreases(anchored, kind, name):
    a = anchored(kind, name)
    p = a["res"]["pairs"]
    assert p.shape[0] == int(a["res"]["count"].sum())
    assert np.unique(p, axis=0).shape[0] == p.shape[0], (kind, name)
    assert a["res"]["crossings"].all(), (kind, name)


@pytest.mark.parametrize("kind,name", SETS)
def test_a_counted_test_implies_the_occlusion_walk(anchored, kind, name):
    a = anchored(kind, name)
    sc, rays = a["sc"], a["rays"][a["idx"]]
    n = rays.shape[0]
    whole = C.walk_count(sc, rays, np.tile(np.array([-INF, INF], np.float32), (n, 1)))
    np.testing.assert_array_equal(whole["count"], a["res"]["count"], err_msg="explicit (-inf, +inf) vs None")
    np.testing.assert_array_equal(whole["front"], a["res"]["front"])
    tmm = np.ascontiguousarray(a["tmm"][a["idx"]])
    for label, iv, res in (("None", None, a["res"]), ("intervals", tmm, C.walk_count(sc, rays, tmm))):
        occ = R.walk(sc, rays, iv, mode="any")["occluded"]
        bad = (res["count"] >= 1) & ~occ
        assert not bad.any(), (kind, name, label, np.flatnonzero(bad)[:8])
        print(f"{kind} {name} {label}: {int((res['count'] >= 1).sum())} rays count, {int(occ.sum())} occluded, of {n}")
        if iv is not None:
            B, Bf = C.brute_count(sc, rays[::5], iv[::5])
            assert (res["count"][::5] <= B).all() and (res["front"][::5] <= Bf).all()


# ------------------------------------------------------------------ 2. known answers
def scene_of(tris, grid_res):
    v, t = S.mesh_of(np.asarray(tris, np.float32))
    hs = rtm.HostScene.from_mesh(v, t, 45.0, np.eye(4, dtype=np.float32).reshape(16), grid_res=grid_res)
    try:
        return R.RefScene.from_host(hs)
    finally:
        hs.close()


def one(sc, ray, tmin=-INF, tmax=INF):
    r = C.walk_count(sc, np.asarray(ray, np.float32).reshape(1, 6), np.array([[tmin, tmax]], np.float32))
    return int(r["count"][0]), int(r["front"][0])


SMALL = [[[-1, -1, 0], [-0.9, -1, 0], [-1, -0.9, 0]], [[1, 1, 1], [0.9, 1, 1], [1, 0.9, 1]]]     # they span the box


def test_interval_rules_by_hand():
    """One triangle in a one-cell-thick box (test_occlusion_cpu.test_restatement_interval_rules' scene): the strict
    bounds, the sign of det, the zero-without-a-walk cases."""
    sc = scene_of([[[-1, -1, 0.5], [1, -1, 0.5], [0, 1, 0.5]]] + SMALL, 8)
    ray = [0.0, -0.5, 2.0, 0.0, 0.0, -1.0]
    tr = R.walk(sc, np.array([ray], np.float32), mode="closest")["t"][0]
    assert abs(tr - 1.5) < 1e-6
    # e1 x e2 = +z and the ray runs down -z, against it: det > 0
    assert one(sc, ray) == (1, 1) and one(sc, ray, 0.0, INF) == (1, 1)
    assert one(sc, [0.0, -0.5, -1.0, 0.0, 0.0, 1.0]) == (1, 0)
    assert one(sc, ray, -INF, np.nextafter(tr, INF)) == (1, 1) and one(sc, ray, np.nextafter(tr, -INF), INF) == (1, 1)
    for tmin, tmax in ((-INF, tr), (tr, INF), (-INF, 0.5 * tr), (tr, tr), (2.0, 1.0), (np.nan, INF), (-INF, np.nan)):
        assert one(sc, ray, tmin, tmax) == (0, 0), (tmin, tmax)
    for j in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            r = list(ray)
            r[j] = bad
            assert one(sc, r) == (0, 0)
    assert one(sc, [5.0, 5.0, 2.0, 0.0, 0.0, -1.0]) == (0, 0)            # misses the grid box
    assert one(sc, [0.0, -0.5, 2.0, 0.0, 0.0, 1.0]) == (0, 0)            # t < 0 is no hit


def test_coincident_triangles_and_opposite_windings():
    a = [[-1, -1, 0.5], [1, -1, 0.5], [0, 1, 0.5]]
    flipped = [a[0], a[2], a[1]]
    ray = [0.0, -0.5, 2.0, 0.0, 0.0, -1.0]
    assert one(scene_of([a, a] + SMALL, 8), ray) == (2, 2)
    assert one(scene_of([a, flipped] + SMALL, 8), ray) == (2, 1)
    assert one(scene_of([a, flipped] + SMALL, 8), ray, 0.0, 1.5) == (0, 0)


def test_a_hit_on_a_crossing_time_counts_in_the_later_cell_only():
    """A triangle in the plane between two cells that both list it, hit at cur_t equal to the crossing: the earlier
    cell's interval excludes its end, the later cell's includes its start -- once, not twice and not never."""
    # Two cells per axis; the plane ToPos(1) between the two layers of cells (grid.h:50-51: bmin + 1 * cw, in f32) is
    # z = 0.  The triangle lies in z = y + 0.25 and spans both layers, so every cell around (x, y) = (0.125, -0.25)
    # lists it, and the ray straight down from z = 0.5 meets it at z = 0: cur_t = 0.5 = the crossing, every term exact.
    # (A triangle IN the plane z = 0 is listed by the upper layer only, and Grid::Intersect itself never accepts it.)
    corners = [[[-1, -1, -1], [-0.9, -1, -1], [-1, -0.9, -1]], [[1, 1, 1], [0.9, 1, 1], [1, 0.9, 1]]]
    sc = scene_of([[[-0.5, -0.75, -0.5], [0.5, -0.75, -0.5], [0.0, 0.25, 0.5]]] + corners, 2)
    assert tuple(sc.dims) == (2, 2, 2) and np.float32(sc.bmin[2] + np.float32(1) * sc.cw) == 0.0
    D0, D02 = 2, 4
    upper, lower = 1 + 1 * D0 + 0 * D02, 1 + 0 * D0 + 0 * D02                # GridIdx of cells (1, 0, 1) and (1, 0, 0)
    for c in (upper, lower):
        assert 0 in sc.cell_tris[sc.offs[c]:sc.offs[c + 1]], "the triangle must be listed on both sides of the plane"
    ray = np.array([[0.125, -0.25, 0.5, 0.0, 0.0, -1.0]], np.float32)
    closest = R.walk(sc, ray, mode="closest")
    assert closest["t"][0] == np.float32(0.5) and closest["steps"][0] == 2  # = the crossing time; taken in the 2nd cell
    res = C.walk_count(sc, ray, pairs=True)
    assert (int(res["count"][0]), int(res["front"][0])) == (1, 1)
    assert res["pairs"].tolist() == [[0, 0]]
    assert one(sc, ray[0], 0.0, 0.5) == (0, 0) and one(sc, ray[0], 0.0, np.nextafter(np.float32(0.5), INF)) == (1, 1)


@pytest.mark.parametrize("name", ("cube", "sphere"))
def test_parity_and_winding_on_closed_meshes(name):
    tris = C.cube_tris() if name == "cube" else C.sphere_tris()
    assert tris.shape[0] == (12 if name == "cube" else 2048)
    sc = scene_of(tris, 16)
    pts, inside = C.closed_mesh_points(name, 4000, seed=11)
    assert 400 < int(inside.sum()) < 3600
    r = np.random.Generator(np.random.PCG64(12))
    rnd = r.normal(size=(pts.shape[0], 3))
    rnd = (rnd / np.sqrt((rnd * rnd).sum(1, keepdims=True))).astype(np.float32)
    zero_inf = np.tile(np.array([0.0, np.inf], np.float32), (pts.shape[0], 1))
    for label, d in (("+x", np.tile(np.array([1, 0, 0], np.float32), (pts.shape[0], 1))), ("random", rnd)):
        res = C.walk_count(sc, np.concatenate([pts, d], axis=1), zero_inf)
        c, f = res["count"].astype(np.int64), res["front"].astype(np.int64)
        np.testing.assert_array_equal((c & 1) == 1, inside, err_msg=f"{name} {label}: parity")
        np.testing.assert_array_equal((c - f) - f, inside.astype(np.int64), err_msg=f"{name} {label}: winding")
    for rule in ("winding", "parity"):
        np.testing.assert_array_equal(C.inside_vote(sc, pts, rtm.INSIDE_DIRS, rule), inside, err_msg=f"{name} {rule}: vote")


def test_default_directions_are_unit_and_off_every_axis_and_plane():
    d = rtm.INSIDE_DIRS
    assert d.dtype == np.float32 and d.shape == (3, 3)
    assert np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(1)) - 1.0).max() < 1e-7
    assert (np.abs(d) > 0.2).all()
    doc = rtm.GpuScene.inside.__doc__
    for v in d.reshape(-1):
        assert f"{abs(float(v)):.8f}" in doc, float(v)


# ------------------------------------------------------------------ 3. the ABI surface and the argument checks
def test_symbol_signature_and_python_surface():
    L = ctypes.CDLL(os.path.join(PKG_DIR, "librt_tracer.so"))
    assert hasattr(L, "rt_crossing_rays_device")
    assert "rt_crossing_rays_device" in rtm.TRACER_SYMBOLS
    src = open(os.path.join(ROOT, "include", "rt_tracer.h")).read()
    assert re.search(r"typedef struct rt_ray_cross \{ uint32_t count; uint32_t front; \} rt_ray_cross;", src)
    assert re.search(r"int\s+rt_crossing_rays_device\(rt_scene \*scene, const rt_ray \*d_rays, const float \*d_tminmax, "
                     r"uint32_t n,\s*uint32_t flags, rt_ray_cross \*d_out, void \*hip_stream\);", src)
    assert ctypes.sizeof(rtm.RayCross) == 8 and rtm.RAY_CROSS_DTYPE.itemsize == 8
    assert [f[0] for f in rtm.RayCross._fields_] == list(rtm.RAY_CROSS_DTYPE.names) == ["count", "front"]
    for m in ("crossings", "inside", "signed_distance"):
        assert callable(getattr(rtm.GpuScene, m, None)), m
    assert rtm.Crossings._fields == ("count", "front", "raw")
    assert rtm.tracer_lib().rt_abi_version() == 8          # an addition bound behind hasattr: no ABI bump
    assert len(rtm.tracer_lib().rt_crossing_rays_device.argtypes) == 7


def test_crossings_rejects_bad_arguments_before_the_device():
    L = rtm.tracer_lib()
    ok = ctypes.c_void_p(0x1000)          # 8-byte aligned, never dereferenced by a rejected call

    def call(scene, rays, tmm, n, flags, out):
        return L.rt_crossing_rays_device(scene, rays, tmm, n, flags, out, None)

    assert call(None, ok, ok, 1, 0, ok) == 1 and "NULL" in last_error(L)
    assert call(FAKE, ok, ok, 1, rtm.RT_RAYS_COUNT, ok) == 1 and "RT_RAYS_COUNT" in last_error(L)
    assert call(FAKE, ok, ok, 1, rtm.RT_RAYS_COUNT | rtm.RT_RAYS_SORT, ok) == 1 and "RT_RAYS_COUNT" in last_error(L)
    assert call(FAKE, ok, ok, 1, 4, ok) == 1 and "unknown" in last_error(L)
    assert call(FAKE, ok, None, 1, rtm.RT_RAYS_SORT | 8, ok) == 1 and "unknown" in last_error(L)
    assert call(FAKE, ok, ok, 0x80000000, 0, ok) == 1 and "2^31" in last_error(L)
    assert call(FAKE, None, ok, 1, 0, ok) == 1 and "d_rays is NULL" in last_error(L)
    assert call(FAKE, ok, ok, 1, 0, None) == 1 and "d_out is NULL" in last_error(L)
    assert call(FAKE, ok, None, 1, 0, None) == 1 and "d_out is NULL" in last_error(L)
    for bad in (0x1004, 0x1001):
        b = ctypes.c_void_p(bad)
        assert call(FAKE, b, ok, 1, 0, ok) == 1 and "8-byte aligned" in last_error(L)
        assert call(FAKE, ok, b, 1, 0, ok) == 1 and "8-byte aligned" in last_error(L)
        assert call(FAKE, ok, ok, 1, 0, b) == 1 and "8-byte aligned" in last_error(L)
        assert call(FAKE, ok, None, 1, rtm.RT_RAYS_SORT, b) == 1 and "8-byte aligned" in last_error(L)
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
            gs.crossings(bad)
        with pytest.raises(ValueError):
            gs.crossings(bad, sort=True)
    tm = np.zeros((4, 2), np.float32)
    for bad in (tm.astype(np.float64), np.zeros((3, 2), np.float32), np.zeros((4, 3), np.float32), np.zeros(8, np.float32),
                np.zeros((4, 4), np.float32)[:, ::2], np.asfortranarray(tm), [[0.0, 1.0]] * 4, torch.zeros((4, 2))):
        with pytest.raises(ValueError):
            gs.crossings(good, bad)
    pts = np.zeros((4, 3), np.float32)
    for bad in (pts.astype(np.float64), np.zeros((4, 4), np.float32), np.zeros(12, np.float32),
                np.zeros((4, 6), np.float32)[:, ::2], [[0.0] * 3], torch.zeros((4, 3)), None):
        for fn in (gs.inside, gs.signed_distance):
            with pytest.raises(ValueError):
                fn(bad)
    for fn in (gs.inside, gs.signed_distance):
        with pytest.raises(ValueError):
            fn(pts, rule="nonzero")
        for bad in (np.zeros((2, 3), np.float32) + 1, np.ones((3, 3), np.float64), np.ones((3, 2), np.float32),
                    np.full((1, 3), np.nan, np.float32), [[1.0, 2.0, 3.0]], np.zeros((0, 3), np.float32)):
            with pytest.raises(ValueError):
                fn(pts, dirs=bad)


# ------------------------------------------------------------------ 4. build guards of rt_crossings.hip
def test_the_new_file_includes_the_hip_runtime_first():
    lines = [l for l in open(SRC).read().splitlines() if l.startswith("#include")]
    assert lines[0] == "#include <hip/hip_runtime.h>"


@needs_hipcc
def test_crossing_device_ir_has_no_contraction_or_fast_math(tmp_path):
    ll = tmp_path / "cross.ll"
    subprocess.run([HIPCC] + FLAGS + ["-emit-llvm", "-S", "-o", str(ll), SRC], check=True, capture_output=True)
    ir = ll.read_text()
    assert "k_cross_rays" in ir
    assert "fmuladd" not in ir
    assert not re.search(r"\bllvm\.fma\.f64\b", ir)
    assert not [l for l in open(SRC).read().splitlines() if re.search(r"\bfmaf?\b|__builtin_fma", l)]
    for flag in (" contract ", " afn ", " arcp ", " nnan ", " ninf ", " nsz ", " reassoc ", " fast "):
        assert flag not in ir, flag
    assert "denormal-fp-math-f32" not in ir or '"denormal-fp-math-f32"="ieee' in ir


@needs_hipcc
def test_crossing_kernels_use_no_scratch_no_lds_and_keep_8_waves(tmp_path):
    """The four k_cross_rays instantiations (k_trace_rays' fast-arm variants | kVarCross 33554432): scratch 0, LDS 0,
    8 waves / SIMD by the compiler's estimate and by the hardware's admission rule, at most 64 VGPRs -- what the
    occlusion kernels hold."""
    table = resource_table(SRC, ["-c", "-o", str(tmp_path / "cross.o")])
    print(table)
    # kVarCross 33554432 | kVarRays 8388608 | kVarWaveGate 2 | kVarDistSkip 8 [| kVarFastRcp 2048] [| 4096 | 4]
    base = 33554432 | 8388608 | 2 | 8
    for var in (base | 2048 | 4096 | 4, base | 4096 | 4, base | 2048, base):
        assert [n for n in table if f"k_cross_raysILi{var}E" in n], (var, sorted(table))
    assert len(table) == 4
    for n, (sg, vg, sc, oc, ld) in table.items():
        assert sc == 0 and ld == 0, (n, sc, ld)
        assert oc == 8 and 800 // (-(-sg // 16) * 16 + 16) >= 8 and vg <= 64, (n, sg, vg, oc)
