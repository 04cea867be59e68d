#!/usr/bin/env python3
"""oracle/gen_golden_alt_cameras.py -- TEST INFRASTRUCTURE ONLY; runs in the build container only.

Pins Renderer::IntersectBruteForce and Renderer::RayMarch under cameras whose 3x3 is not orthonormal, from eyes in
odd places and on degenerate meshes (tests/alt_cameras.py has the case list) to the reference's OWN code, as
gen_golden_alt.py pins them on the shipped scenes at their own cameras and gen_golden_cameras.py pins the grid walk:

  * records of a window through `refdriver alt-samples ... brute|march <out> --view <file>`;
  * frames through `refdriver render ... --isect brute|march --view <file>`.

Writes tests/golden/alt_cameras.json: per case the camera's bits, the SHA-256 of every record column and of the frame,
the hit count and the sum of the march steps -- hashes and counts only.

Checked on the CPU before anything is written: the reference and the live CPU restatement (liboracle_tracer.so under
the case's view) agree on every column of every case and on every frame; every march window named in
alt_cameras.WINDOW holds hits and misses under the scene's own camera; the NaN-distance triangles of the nan_* meshes
are the first records of the Morton order.  RayMarch and IntersectBruteForce convert no float to an integer, so no
sample's reference result rests on undefined behaviour and none is left out.

    make -C oracle ref && make -C oracle && python oracle/gen_golden_alt_cameras.py
"""
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import alt_cameras as A            # noqa: E402
from conftest import ALT_REC_DTYPE, Oracle        # noqa: E402
import gen_golden_synth as G       # noqa: E402  (REF)

REF_TIMEOUT_S = 600
GENERATOR = "oracle/gen_golden_alt_cameras.py via oracle/_ref/refdriver (alt-samples --view; render --isect --view)"


def ref(args):
    subprocess.run([G.REF] + args, check=True, capture_output=True, timeout=REF_TIMEOUT_S)


def reference(tmp, i, path, c):
    """(columns of the reference's records of the case's window, its frame or None)."""
    vp = os.path.join(tmp, f"{i}.view")
    with open(vp, "wb") as f:
        f.write(np.asarray(c["cam"], "<f4").tobytes() + np.asarray([c["fov"]], "<f4").tobytes())
    rp, bp = os.path.join(tmp, f"{i}.rec"), os.path.join(tmp, f"{i}.bgra")
    ref(["alt-samples", path] + [str(x) for x in c["window"]] + [c["mode"], rp, "--view", vp])
    rec = np.fromfile(rp, ALT_REC_DTYPE)
    Wd, Ht, spp, _, _, w, h = c["window"]
    assert rec.size == w * h * spp, c["key"]
    img = None
    if c["frame"]:
        ref(["render", path] + [str(x) for x in c["frame"]] + ["--isect", c["mode"], "--threads", "2", "--out", bp, "--view", vp])
        img = np.fromfile(bp, "<u4").reshape(c["frame"][1], c["frame"][0])
    for p in (vp, rp, bp):
        if os.path.exists(p):
            os.remove(p)
    return A.columns(rec, c["mode"]), img


def main():
    if not os.path.exists(G.REF):
        sys.exit("build the reference drivers first: make -C oracle ref")
    tmp = tempfile.mkdtemp()
    t0 = time.time()
    specs = A.specs(tmp)
    meshes = A.meshes()
    for name, lead in A.NAN_FIRST.items():
        assert sorted(A.morton_order(meshes[name])[:lead]) == list(range(lead)), name
    paths = {c["scene"]: A.scene_file(c["scene"], tmp) for c in specs}
    with ThreadPoolExecutor(max_workers=max(1, (os.cpu_count() or 2) // 2)) as ex:
        refs = list(ex.map(lambda ic: reference(tmp, ic[0], paths[ic[1]["scene"]], ic[1]), enumerate(specs)))
    print(f"reference: {len(specs)} cases in {time.time() - t0:.0f} s", flush=True)
    t0 = time.time()
    live = A.Live(Oracle(), tmp)
    cases = {}
    for c, (cols, img) in zip(specs, refs):
        lcols, limg = live.expect(c)
        A.check_columns(lcols, cols, c["key"] + " (restatement vs reference)")
        if img is not None:
            np.testing.assert_array_equal(limg, img, err_msg=c["key"] + " frame (restatement vs reference)")
        e = A.entry(cols, img)
        n = cols["hit"].size
        if c["what"] == "identity" and c["mode"] == "march" and c["scene"] in A.WINDOW and c["scene"] != "nan_only":
            assert 0 < e["hits"] < n, (c["key"], "the march window needs hits and misses", e["hits"], n)
        if c["scene"] == "nan_only":
            assert e["hits"] == 0, c["key"]
        cases[c["key"]] = A.to_json(c, e)
        print(f"{c['key']}: {e['hits']} of {n} samples hit, {e['steps']} steps", flush=True)
    live.close()
    print(f"restatement: {time.time() - t0:.0f} s", flush=True)
    text = A.fixture_text(GENERATOR, {k: A.sha(v) for k, v in meshes.items()}, cases)
    with open(A.FIXTURE, "w") as f:
        f.write(text)
    print(f"wrote {len(cases)} cases, {os.path.getsize(A.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
