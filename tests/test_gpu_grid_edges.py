"""The device grid build (csrc/rt_grid_build.hip: k_tri_ranges, its own scan k_scan_tiles / k_scan_add,
k_candidates, its own LSD radix sort k_rs_count / k_rs_scatter, k_offsets) on the meshes of
tests/grid_meshes.py, against the reference's own Grid::Grid (tests/golden/grid.json, independent of our host
build) and, array for array, against the host build.

What the sizes are for: the scan and the sort work on 1,024-element tiles of 256 lanes x 4, so the triangle
count and the key count sit on 63 / 64 / 65 (a wave), 255 / 256 / 257 (a block's lanes), 1,023 / 1,024 / 1,025
(a tile) and 2,049 (a third tile); 1,048,577 triangles reach the scan's third level and 43-bit keys; at
resolution 1 every key of the upper passes has the same digit; the skew and all-negative cases give single
triangles a quarter of a million candidate cells.  A wrong scan or sort is a wrong CSR for every later render
of the scene, so the bar is equality of every word.

The rejected cases and the candidate limit complete their kernels and report through the error word or the
candidate count: nothing faults by design.
"""
import time

import numpy as np
import pytest

import grid_meshes as G
import synth_scenes as S
from conftest import load_package

rtm = load_package()
FIX = G.fixture()["cases"]
EYE = np.eye(4, dtype=np.float32)
SIZE_CASES = [n for n in G.ACCEPTED if G.CASES[n]["kind"] == "size"]
HOST_CASES = SIZE_CASES + ["skew", "all_negative"]
# sort passes of each size case, ceil((tb + cb) / 8): 64^3 cells are 19 bits, 8^3 are 10, one cell is 1
PASSES = {1: 3, 2: 3, 63: 4, 64: 4, 65: 4, 255: 4, 256: 4, 257: 4, 1023: 4, 1024: 4, 1025: 4, 2049: 4,
          4097: 3, 5000: 2, 100: 1}


def device_build(name):
    v, t = G.mesh(name)
    return rtm.gpu_grid_build(v, t, G.CASES[name]["res"], 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", G.ACCEPTED)
def test_device_grid_matches_reference(name):
    t0 = time.perf_counter()
    meta, offs, tris, ms = device_build(name)
    print(f"{name}: device build {ms:.2f} ms, call {time.perf_counter() - t0:.2f} s")
    G.check_against_fixture(FIX[name], meta, offs, tris, name)
    assert ms > 0.0


def test_size_cases_cover_the_sort_pass_counts():
    """One pass, an even count and an odd count: the sorted keys are read from either buffer (runs on CPU)."""
    passes = {n: G.sort_passes(FIX[n]["num_triangles"], FIX[n]["dims"]) for n in SIZE_CASES}
    assert passes["points_100_res1"] == 1 and passes["points_5000_res1"] == 2 and passes["points_4097_res7"] == 3
    assert passes["points_63_res64"] == 4 and passes["points_1_res64"] == 3
    assert G.sort_passes(FIX["big"]["num_triangles"], FIX["big"]["dims"]) == 6


@pytest.mark.gpu
@pytest.mark.parametrize("name", HOST_CASES)
def test_device_grid_matches_host_build(name):
    c = G.CASES[name]
    v, t = G.mesh(name)
    hs = rtm.HostScene.from_mesh(v, t, 45.0, EYE, grid_res=c["res"])
    try:
        hm, ho, ht = hs.grid()
    finally:
        hs.close()
    meta, offs, tris, _ = rtm.gpu_grid_build(v, t, c["res"], 0)
    nt = t.shape[0]
    if c["kind"] == "size":                                    # the preconditions the case is for
        assert int(ho[-1]) == nt == c["args"][0]
        tb, cb = max(1, int(nt - 1).bit_length()), int(np.prod(hm["dims"])).bit_length()    # as build() does
        assert -(-(tb + cb) // 8) == PASSES[nt]
    assert meta["dims"] == hm["dims"]
    assert G.meta_bits(meta) == G.meta_bits(hm)
    np.testing.assert_array_equal(offs, ho, err_msg=name)
    np.testing.assert_array_equal(tris, ht, err_msg=name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", G.REJECTED)
def test_device_rejects_what_the_reference_aborts_on(name):
    """grid.cpp:121 (a cell index outside the grid) or grid.cpp:125 (a triangle touches no cell)."""
    assert not FIX[name]["accepted"]
    with pytest.raises(rtm.RtError, match=r"overlaps a cell outside the grid|touches no cell \(grid\.cpp:121-125\)"):
        device_build(name)


@pytest.mark.gpu
def test_candidate_limit_is_reported():
    """8,300 triangles in the minimum-corner cell of an all-negative mesh: 8,300 x 64^3 >= 2^31 candidate cells.
    Only k_tri_ranges and the scan run; the build must raise and return no CSR.  The reference accepts such a
    mesh (a limit of the device build); no host build here, it would take minutes."""
    v, t = S.mesh_of(G.candidate_limit_mesh())
    assert t.shape[0] * 64 ** 3 >= 2 ** 31 and (v[:, :3] < 0).all()
    with pytest.raises(rtm.RtError, match="too many candidate cells"):
        rtm.gpu_grid_build(v, t, 64, 0)


RENDER_VIEWS = {"planes_res7": ((0.3, 0.2, 3.0), (0.0, 0.0, 0.0), 45.0),
                "all_negative": ((-1.1, -0.8, 1.6), (-1.4, -1.4, -1.4), 45.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RENDER_VIEWS))
def test_scene_from_mesh_at_any_resolution_renders_identically(name):
    """rt_scene_create_from_mesh at the case's resolution against rt_scene_create on the host's CSR: the same
    62x46x4 frame and the same rt_trace_samples records, from a camera that sees hits and misses."""
    eye, at, fov = RENDER_VIEWS[name]
    res = G.CASES[name]["res"]
    v, t = G.mesh(name)
    hs = rtm.HostScene.from_mesh(v, t, fov, S.look(eye, at), grid_res=res)
    a = rtm.GpuScene(hs, 0)
    b = rtm.GpuScene(hs, 0, gpu_grid=True, grid_res=res)
    try:
        assert hs.grid()[0]["dims"] == FIX[name]["dims"]
        fa, fb = a.frame(S.W, S.H, S.SPP), b.frame(S.W, S.H, S.SPP)
        ra, rb = a.trace_samples(fa, 0, 0, S.W, S.H), b.trace_samples(fb, 0, 0, S.W, S.H)
        hits = int((ra["hit"] == 1).sum())
        assert hits >= 100 and ra.shape[0] - hits >= 100, (hits, ra.shape[0])
        np.testing.assert_array_equal(ra.view(np.uint32), rb.view(np.uint32))
        np.testing.assert_array_equal(a.render_frame(fa), b.render_frame(fb))
        assert a.device_bytes() == b.device_bytes()
    finally:
        a.close()
        b.close()
        hs.close()
