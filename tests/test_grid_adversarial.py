"""The host grid build (host/rt_host.cpp build_grid) and the oracle's restatement (oracle/cpu_tracer.cpp
BuildGrid) against the reference's own Grid::Grid on the meshes of tests/grid_meshes.py: vertices on cell
planes, triangles lying in cell planes, degenerate triangles, offsets on either side of where the 0.0001 pad
rounds away, all-negative meshes, single triangles, needles, tiny extents, resolutions 1, 7, 128 and 200, one
triangle that spans the grid among tiny ones, 1,048,577 triangles.  tests/golden/grid.json holds what the
reference made of each (oracle/gen_golden_grid.py); a case the reference aborts on must raise here.
Needs no GPU and no reference tree.
"""
import numpy as np
import pytest

import grid_meshes as G
import synth_scenes as S
from conftest import OrcInfo, load_package

rtm = load_package()
FIX = G.fixture()["cases"]
EYE = np.eye(4, dtype=np.float32)


def host_build(name, nthreads=0):
    v, t = G.mesh(name)
    hs = rtm.HostScene.from_mesh(v, t, 45.0, EYE, grid_res=G.CASES[name]["res"], nthreads=nthreads)
    try:
        return hs.grid()
    finally:
        hs.close()


def test_fixture_covers_the_catalogue():
    """Every catalogue case has a fixture entry made from the mesh the generator builds today, the reference
    accepted exactly the cases the catalogue lists as accepted, and none was dropped."""
    assert set(FIX) == set(G.CASES)
    assert sorted(n for n, e in FIX.items() if not e["accepted"]) == sorted(G.REJECTED)
    assert len(G.REJECTED) == sum(not e["accepted"] for e in FIX.values()) == 5
    for name, c in G.CASES.items():
        e = FIX[name]
        assert e["res"] == c["res"] and e["accepted"] == c["accept"], name
        if not e["accepted"]:
            assert set(e) == {"mesh_sha256", "res", "accepted", "exit_status"} and e["exit_status"] == 134, name
        elif c["kind"] == "size":
            assert e["num_refs"] == e["num_triangles"] == c["args"][0], name     # one key per point triangle
    # what the cases are for
    assert FIX["planes_res7"]["dims"] == [8, 8, 8]                   # ceil yields more cells than asked
    assert FIX["single_flat_z"]["dims"] == [64, 64, 1] and FIX["single_needle"]["dims"] == [64, 1, 1]
    assert FIX["single_point"]["num_refs"] == 1 and FIX["single_point"]["dims"] == [64, 64, 64]
    assert FIX["shift_-65536"]["max_refs_per_cell"] == 202           # the grid reaches to 0: all in one cell
    assert FIX["big"]["num_triangles"] == 1048577 and FIX["big"]["dims"] == [128, 128, 128]
    assert FIX["all_negative"]["meta_bits"][3:6] == G.bits([np.float32(1.17549435e-38) + np.float32(0.0001)] * 3)


@pytest.mark.parametrize("name", list(G.CASES))
def test_mesh_bytes_are_pinned(name):
    """The generator reproduces the mesh the fixture was made from, byte for byte."""
    assert G.mesh_sha(*G.mesh(name)) == FIX[name]["mesh_sha256"]


@pytest.mark.parametrize("name", G.ACCEPTED)
def test_host_grid_matches_reference(name):
    meta, offs, tris = host_build(name)
    G.check_against_fixture(FIX[name], meta, offs, tris, name)


@pytest.mark.parametrize("nthreads", [1, 3, 8])
@pytest.mark.parametrize("name", G.THREADED)
def test_host_grid_thread_count_invariant(name, nthreads):
    """The stable merge of the threads' triangle ranges keeps every cell's list ascending (grid.cpp:122)."""
    meta, offs, tris = host_build(name, nthreads)
    G.check_against_fixture(FIX[name], meta, offs, tris, f"{name} nthreads {nthreads}")


@pytest.mark.parametrize("name", G.REJECTED)
def test_host_rejects_what_the_reference_aborts_on(name):
    with pytest.raises(rtm.RtError, match=r"grid\.cpp:121-125"):
        host_build(name)


@pytest.mark.parametrize("name", [n for n in G.ACCEPTED if G.CASES[n]["res"] == 64])
def test_oracle_grid_matches_reference(oracle, tmp_path, name):
    """The oracle's BuildGrid on the same scene file.  orc_scene_load builds at 64 cells only (scene.cpp:7), so
    the cases at other resolutions do not go through it."""
    v, t = G.mesh(name)
    path = str(tmp_path / (name + ".rtscene"))
    G.write_rtscene(path, v, t)
    sc = S.OracleScene(oracle, path)
    try:
        i = OrcInfo()
        assert sc.L.orc_scene_info(sc.h, i) == 0
        offs, refs = np.zeros(i.num_cells + 1, np.uint32), np.zeros(max(1, i.num_refs), np.uint32)
        assert sc.L.orc_scene_csr(sc.h, offs.ctypes.data, refs.ctypes.data) == 0
        meta = {"dims": list(i.dims), "aabb_min": np.array(i.aabb_min, np.float32),
                "aabb_max": np.array(i.aabb_max, np.float32), "cell_wdh": i.cell_wdh, "inv_cell_wdh": i.inv_cell_wdh}
        G.check_against_fixture(FIX[name], meta, offs, refs[:i.num_refs], "oracle " + name)
    finally:
        sc.close()
