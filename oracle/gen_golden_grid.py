#!/usr/bin/env python3
"""oracle/gen_golden_grid.py -- TEST INFRASTRUCTURE ONLY; runs in the build container only.

Pins the meshes of tests/grid_meshes.py to the reference's OWN Grid::Grid (oracle/_ref/refdriver grid, see
oracle/Makefile): each case is written as a .rtscene to a temporary directory, the reference builds its grid
at the case's resolution, and tests/golden/grid.json records what it made -- hashes and settings only, no mesh:

  accepted case   mesh SHA-256, resolution, dims, the eight metadata words as bits (aabb_min, aabb_max,
                  cell_wdh, inv_cell_wdh), num_refs, the most references in a cell, and the CSR SHA-256 in the
                  form of tests/test_host_grid.py (offsets || refs)
  rejected case   mesh SHA-256, resolution and the reference's exit status (134: an assert of grid.cpp:121-125)

Nothing is written when a case the catalogue lists as accepted is rejected or the other way round, or when a
point-triangle case has num_refs != nt: fix the seed, do not relax the case.

    make -C oracle ref && python oracle/gen_golden_grid.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grid_meshes as G   # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "refdriver")
REF_TIMEOUT_S = 300


def reference_grid(tmp, name, v, t, res):
    """The reference's grid of one mesh: (exit status, None) when it rejects it, else (0, entry fields)."""
    path, out = os.path.join(tmp, name + ".rtscene"), os.path.join(tmp, name + ".grid")
    G.write_rtscene(path, v, t)
    p = subprocess.run([REF, "grid", path, out, str(res)], capture_output=True, text=True, timeout=REF_TIMEOUT_S)
    os.remove(path)
    if p.returncode != 0:
        return (128 - p.returncode if p.returncode < 0 else p.returncode), None
    with open(out, "rb") as f:
        raw = f.read()
    os.remove(out)
    dims = np.frombuffer(raw, "<u4", 3, 0)
    meta = np.frombuffer(raw, "<u4", 8, 12)
    nc, nr = (int(x) for x in np.frombuffer(raw, "<u4", 2, 44))
    assert nc == int(dims[0]) * int(dims[1]) * int(dims[2])
    offs = np.frombuffer(raw, "<u4", nc + 1, 52)
    refs = np.frombuffer(raw, "<u4", nr, 52 + 4 * (nc + 1))
    assert len(raw) == 52 + 4 * (nc + 1 + nr) and int(offs[-1]) == nr
    return 0, {"dims": [int(d) for d in dims], "meta_bits": [f"{w:08x}" for w in meta], "num_refs": nr,
               "max_refs_per_cell": int(np.diff(offs).max()), "csr_sha256": G.csr_sha(offs, refs)}


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference driver first: make -C oracle ref")
    tmp = tempfile.mkdtemp()
    cases, wrong = {}, []
    for name, c in G.CASES.items():
        v, t = G.mesh(name)
        status, e = reference_grid(tmp, name, v, t, c["res"])
        entry = {"mesh_sha256": G.mesh_sha(v, t), "res": c["res"], "accepted": e is not None}
        if e is None:
            entry["exit_status"] = status
        else:
            entry.update(e)
            entry["num_triangles"] = int(t.shape[0])
        if entry["accepted"] != c["accept"]:
            wrong.append(f"{name}: the catalogue says accept={c['accept']}, the reference exit status is {status}")
        elif e is not None and c["kind"] == "size" and e["num_refs"] != t.shape[0]:
            wrong.append(f"{name}: {t.shape[0]} point triangles but {e['num_refs']} references")
        cases[name] = entry
        print(name, "rejected, exit status %d" % status if e is None else
              f"dims {e['dims']} refs {e['num_refs']} max/cell {e['max_refs_per_cell']}", flush=True)
    if wrong:
        sys.exit("nothing written:\n  " + "\n  ".join(wrong))
    meta = {"generator": "oracle/gen_golden_grid.py via oracle/_ref/refdriver grid", "cases": cases}
    with open(G.FIXTURE, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {G.FIXTURE}: {len(cases)} cases, {sum(not c['accepted'] for c in cases.values())} rejected, "
          f"{os.path.getsize(G.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
