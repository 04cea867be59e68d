"""The cases of tests/alt_cameras.py without a GPU.

1. The live CPU restatement (oracle/liboracle_tracer.so under each case's view: the restated IntersectBruteForce and
   RayMarch loops) against every case of tests/golden/alt_cameras.json -- the reference's own records and frames.
2. tests/march_ref.py (numpy float32 over the oracle's DistancePointTri) on the camera rays of
   camera_matrices.generate_rays against every march window, bit for bit; the rays of a window are split over the
   restatement's thread pool (serially the worst case, an all-miss window of scene 8, takes about 36 s; stack1500's
   windows 1 to 4 s).
3. The frame march's receding-miss stop (march_ref.frame_stop_condition: ray_march's operations in csrc/rt_frame_isect.h):
   every ray it ends anywhere is a miss of the whole 128-step loop -- for directions of length 2^0 ... 2^20, floors
   of half-extent 1 ... 4,096 under nearly parallel rays, and the far eyes of the fixture.
"""
import time

import numpy as np
import pytest

import alt_cameras as A
import camera_matrices as C
import march_ref as M
import synth_scenes as S
from test_distance_cpu import tree_check        # noqa: F401  (the fixture: tests/dist_tree_check.cpp, built once)
from test_march_cpu import crop_rays, stop_families

rtm = A.rtm
F = np.float32
CASES, MESH_SHAS = A.fixture()
MARCH_CHUNK = 32                 # rays per march_ref.march call on the pool


@pytest.fixture(scope="module")
def live(oracle, tmp_path_factory):
    lv = A.Live(oracle, tmp_path_factory.mktemp("alt_cameras"))
    t0 = time.time()
    yield lv
    print(f"alt_cameras: live restatement of {len(lv.cache)} cases, {time.time() - t0:.0f} s in this module")
    lv.close()


def test_fixture_covers_the_case_list():
    keys = list(CASES)
    n_fac = len(C.FACTOR_NAMES)
    assert n_fac == 19
    for scene in A.A1_SCENES:
        for mode in ("brute", "march"):
            assert sum(k.startswith(f"A1|{scene}|") and k.endswith(mode) and "_spp" not in k for k in keys) == n_fac
    assert sum(k.startswith("A1|scene8|") for k in keys) == 2 * len(A.SCENE8_FACTORS)
    assert sum("_spp" in k for k in keys) == 4
    assert sum(k.startswith("A2|") for k in keys) == len(A.A2_SCENES) * len(A.A2_FACTORS) * 10
    meshes = A.meshes()
    assert {k: A.sha(v) for k, v in meshes.items()} == MESH_SHAS
    for name in meshes:
        want = len(A.FLOOR_FACTORS) if name == "floor2047" else 1
        for mode in ("brute", "march"):
            assert sum(k.startswith(f"A3|{name}|") and k.endswith(mode) for k in keys) == want, name
    for n in A.BLOCK_SIZES:
        assert meshes[f"sparse_{n}"].shape[0] == n
    assert len(keys) == 200


def test_nan_triangles_are_the_first_sorted_records(oracle, tree_check):
    """The nan_* meshes put triangles whose DistancePointTri is NaN for every point first in the order that
    dist_tree_build (csrc/rt_dist_tree.h, the function rt_scene_create runs) gives them: tests/dist_tree_check.cpp
    writes that order out.  alt_cameras.morton_order, which the generator and the GPU test use, must be that order
    on every A3 mesh."""
    meshes = A.meshes()
    pts = np.array([[0.1, 0.2, 0.3], [-3.0, 5.0, 0.0], [0.0, 0.0, 0.0]], F)
    for name, tris in meshes.items():
        order, _ = tree_check(tris, pts, "alt_" + name)
        np.testing.assert_array_equal(order, A.morton_order(tris), err_msg=name)
    for name, lead in A.NAN_FIRST.items():
        tris = meshes[name]
        order, _ = tree_check(tris, pts, "alt_" + name)
        assert sorted(order[:lead]) == list(range(lead)), name
        d = M.D.all_distances(oracle, pts, tris[:lead])
        assert np.isnan(d).all(), name
        if lead < tris.shape[0]:
            assert not np.isnan(M.D.all_distances(oracle, pts, tris[lead:])).any(), name


@pytest.mark.parametrize("key", sorted(CASES))
def test_restatement_against_the_reference(live, key):
    c = CASES[key]
    cols, img = live.expect(c)
    n = cols["hit"].size
    print(f"{key}: {int(cols['hit'].sum())} of {n} samples hit, {int(cols['steps'].astype(np.int64).sum())} steps")
    A.check_entry(cols, img, c["exp"], key)
    if c["mode"] != "march":
        return
    _, _, tris = live.scene(c["scene"])
    Wd, Ht, spp, x0, y0, w, h = c["window"]
    rays = crop_rays(c["cam"], c["fov"], Wd, Ht, rtm.sample_table(spp), x0, y0, w, h)
    rec = np.concatenate(list(live.pool.map(lambda i: M.march(live.oracle, rays[i:i + MARCH_CHUNK], tris),
                                            range(0, rays.shape[0], MARCH_CHUNK))))
    hit = rec["steps"] != 0
    np.testing.assert_array_equal(hit.astype(np.uint32), cols["hit"], err_msg=key)
    np.testing.assert_array_equal(np.where(hit, rec["steps"], A.MARCH_STEPS), cols["steps"], err_msg=key)
    np.testing.assert_array_equal(S.nan_canonical(rec["t"].view(np.uint32)), cols["t"], err_msg=key)
    y = np.repeat(np.arange(y0, y0 + h), w * spp).astype(F)
    with np.errstate(all="ignore"):
        col = np.where(hit, rec["t"] / F(3.0), y / F(Ht)).astype(F)
    np.testing.assert_array_equal(S.nan_canonical(np.repeat(col[:, None], 3, 1).view(np.uint32)), cols["rgb"], err_msg=key)


# ------------------------------------------------------------------ the frame march's stop
SCALES = (0, 2, 4, 10, 20)
FLOOR_SCALES = (0, 4, 10, 16, 20)
FLOOR_HALVES = (1.0, 64.0, 4096.0)


def floor_rays(half, n, seed):
    """n rays 0.001 ... 0.0013 x (1 + 0.01 half) below the floor of that half-extent, within a hundredth of parallel
    to it, pointing up or down."""
    r = np.random.Generator(np.random.PCG64(seed))
    o = np.zeros((n, 3))
    o[:, 0], o[:, 2] = r.uniform(-0.5 * half, 0.5 * half, n), r.uniform(-0.5 * half, 0.5 * half, n)
    o[:, 1] = -r.uniform(0.001, 0.0013, n) * (1.0 + 1e-2 * half)
    phi = r.uniform(0.0, 2.0 * np.pi, n)
    d = np.stack([np.cos(phi), r.uniform(-0.01, 0.01, n), np.sin(phi)], 1)
    d /= np.sqrt((d * d).sum(1))[:, None]
    return np.ascontiguousarray(np.concatenate([o, d], 1), F)


def scaled(rays, k):
    out = rays.copy()
    out[:, 3:] *= F(2.0 ** k)
    return out


def stop_violations(oracle, rays, tris):
    """(rays stopped, rays that hit, indices of rays the condition stops although the 128-step loop hits)."""
    vmin, vmax, scale = M.vertex_box(tris)
    trace = []
    rec = M.march(oracle, rays, tris, max_steps=A.MARCH_STEPS, min_dist=1e-3, trace=trace)
    stopped = np.zeros(rays.shape[0], bool)
    for idx, pos in trace:
        stopped[idx[M.frame_stop_condition(rays[idx, 3:], pos, vmin, vmax, scale)]] = True
    return int(stopped.sum()), int((rec["steps"] != 0).sum()), np.flatnonzero(stopped & (rec["steps"] != 0))


def test_every_ray_the_frame_stop_ends_is_a_miss(oracle, live):
    """Every ray is checked against the full 128-step loop, so no cap on unstopped rays is needed.  The condition
    must fire in every family, or the families test nothing."""
    total = viol = rays_n = 0
    sets = []
    tris = S.sparse(7, n=30)
    for name, rays in stop_families(tris, 48, 11).items():
        for k in SCALES:
            sets.append((f"{name} x 2^{k}", scaled(rays, k), tris))
    for half in FLOOR_HALVES:
        for k in FLOOR_SCALES:
            sets.append((f"floor {half:g} x 2^{k}", scaled(floor_rays(half, 400, 17 + int(half)), k), A.floor(half)))
    for key, c in sorted(CASES.items()):
        if c["group"] == "A2" and c["what"].split("@")[0] in A.FAR_EYES:
            rays = C.generate_rays(c["cam"], c["fov"], *A.MARCH_FRAME[:2], rtm.sample_table(1))
            sets.append((key, rays, live.scene(c["scene"])[2]))
    fired = {}
    for name, rays, tr in sets:
        stopped, hits, bad = stop_violations(oracle, rays, tr)
        print(f"{name}: {rays.shape[0]} rays, {hits} hit, {stopped} stopped, {bad.size} violations")
        assert bad.size == 0, (name, bad[:8], rays[bad[:8]])
        fam = name.split(" x ")[0]
        fired[fam] = fired.get(fam, 0) + stopped
        total, viol, rays_n = total + stopped, viol + bad.size, rays_n + rays.shape[0]
    print(f"frame stop: {rays_n} rays, {total} stopped, {viol} violations")
    assert all(v > 0 for v in fired.values()), fired
    assert viol == 0
