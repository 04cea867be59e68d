#!/usr/bin/env python3
"""oracle/gen_golden_cameras.py -- TEST INFRASTRUCTURE ONLY; runs in the build container only.

Pins cameras whose 3x3 is NOT orthonormal (tests/camera_matrices.py: a rotation times a scale, a shear, a
mirror, a rank-2 matrix ...) to the reference's OWN code, as gen_golden_synth.cameras() pins the orthonormal ones:

  * the 64-cell scenes (scene 1, scene 8, stack1500, inside) through `refdriver render --view` at 96x54x4: the
    frame's and the per-sample hit IDs' SHA-256 per (scene, factor);
  * the single-cell scenes (grid_res = 1: the frozen sliver scene in its nine list shapes, facing9, edge_on17)
    through `refdriver rays <file> 1` -- the reference's Grid::Intersect on a one-cell grid, which `render` cannot
    build -- on the frame's camera rays at 64x64x4 with the suite's sample offsets: the hit IDs' SHA-256.  The rays
    are GenerateRay restated in numpy float32 (camera_matrices.generate_rays), checked here bit for bit against
    orc_kat_genray, which tests/test_oracle_golden.py pins to the reference's recorded rays.

Writes tests/golden/cameras.json: hashes and bit patterns only, in camera_matrices.compact()'s form (the base cameras;
every other matrix and the pad triangles are recomputed on loading).  The sliver scene is frozen there as float32
bits: its camera, the sliver triangle, and what tests/record_gate_check.cpp counts on it (checked before writing:
wholly_gated_ok1 >= 1 at S = 1024 and at 2^20, 0 at S = 1).

Checked on the CPU before anything is written: the reference and the live CPU restatement (liboracle_tracer.so;
tests/occlusion_ref.py for the one-cell grids) agree on every case, and no sample's reference result rests on
undefined behaviour (the float the reference converts to int at grid.h:46 is finite and below 2^30 for every ray
its box test accepts).  A (scene, factor) with such a sample is left out and listed under "dropped"; none may be
dropped for the uniform scales and the mirror.

    make -C oracle ref && python oracle/gen_golden_cameras.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import camera_matrices as C        # noqa: E402
import occlusion_ref as R          # noqa: E402
import synth_scenes as S           # noqa: E402
from conftest import Oracle        # noqa: E402
import gen_golden_synth as G       # noqa: E402  (run, render, view_file)

SLIVER_SEED, SLIVER_WIDTH = 3, 1e-3       # chosen on the CPU with tests/record_gate_check.cpp (scene mode)
REF_TIMEOUT_S = 120


def sha(b):
    return hashlib.sha256(b).hexdigest()


def ref_rays(tmp, path, rays, grid_res):
    rp, op = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.rec")
    np.ascontiguousarray(rays, "<f4").tofile(rp)
    subprocess.run([G.REF, "rays", path, rp, op, str(grid_res)], check=True, capture_output=True, timeout=REF_TIMEOUT_S)
    rec = np.fromfile(op, "<u4").reshape(-1, 8)
    assert rec.shape[0] == rays.shape[0]
    return rec


def undefined(sc, rays):
    """Rays the reference's box test accepts whose grid.h:46 operand is not finite or not below 2^30 (as
    gen_golden_rays.undefined_rays)."""
    inside, ok, enter, g = R.box_entry(sc, rays[:, :3].copy(), rays[:, 3:].copy())
    with np.errstate(all="ignore"):
        x = ((g - sc.bmin) * sc.icw).astype(np.float32).astype(np.float64)
    bad = ~(np.isfinite(x) & (np.abs(x) < 2.0 ** 30)).all(1)
    return np.flatnonzero((inside | ok) & bad)


def kat_rays(oracle, cam, fov, Wd, Ht, smp):
    """orc_kat_genray for every (y, x, sample): the pinned restatement of the reference's GenerateRay."""
    smp = np.asarray(smp, np.float32).reshape(-1, 2)
    y, x, s = [a.reshape(-1) for a in np.meshgrid(np.arange(Ht), np.arange(Wd), np.arange(smp.shape[0]), indexing="ij")]
    rin = np.zeros((x.size, 23), np.float32)
    rin[:, :16] = np.asarray(cam, np.float32)
    b = rin.view(np.uint32)
    b[:, 16], b[:, 17], b[:, 18], b[:, 19] = x, y, Wd, Ht
    rin[:, 20], rin[:, 21], rin[:, 22] = smp[s, 0], smp[s, 1], np.float32(fov)
    return np.ascontiguousarray(oracle.kat("genray", rin, 6), np.float32)


def checker(tmp):
    exe = os.path.join(tmp, "record_gate_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "record_gate_check.cpp"), "-o", exe], check=True)
    return exe


def gate_counts(exe, path, cam):
    a = [exe, "scene", path, str(C.W), str(C.H), str(C.SPP), "1", "8", "--cam"] + C.hexf(cam) + \
        ["--grid-res", "1", "--offsets"] + C.hexf(C.OFFSETS)
    r = json.loads(subprocess.run(a, check=True, capture_output=True, text=True, timeout=REF_TIMEOUT_S).stdout)
    return {k: r[k] for k in ("wholly_gated_ok1", "violations", "ok1_true", "long_records", "gate_ok")}


def main():
    if not os.path.exists(G.REF):
        sys.exit("build the reference drivers first: make -C oracle ref")
    oracle = Oracle()
    tmp = tempfile.mkdtemp()
    fac = C.factors()
    out = {"generator": "oracle/gen_golden_cameras.py via oracle/_ref/refdriver (render --view; rays <file> 1)",
           "factors": [n for n, _ in fac], "bases": {}, "cams": {}, "cases": {}, "dropped": {}}

    # ---- the sliver scene, frozen
    scam = C.sliver_camera(SLIVER_SEED)
    out["sliver"] = {"seed": SLIVER_SEED, "width": SLIVER_WIDTH, "cam_bits": C.bits(scam), "scenes": {}, "gate_check": {}}
    for nt, pos in C.SLIVER_LISTS:
        out["sliver"]["scenes"][f"{nt}_{pos}"] = C.bits(C.sliver_scene(scam, SLIVER_WIDTH, nt, pos))
    exe = checker(tmp)

    def one_case(key, scene, fname, cam, fov, e):
        e.update({"scene": scene, "factor": fname})
        out["cases"][key] = e

    # ---- single-cell scenes: refdriver rays <file> 1
    cells = C.cell_scenes(out)
    smp = C.OFFSETS.reshape(-1, 2)
    for scene, (tris, cam0) in cells.items():
        hs = C.host_scene(tris, cam0)
        path = os.path.join(tmp, scene + ".rtscene")
        try:
            assert hs.grid()[0]["dims"] == [1, 1, 1], scene
            hs.save(path)
            sc = R.RefScene.from_host(hs)
        finally:
            hs.close()
        base = C.base_of(scene)
        out["bases"][base] = {"cam_bits": C.bits(cam0)}
        for fname, f in fac:
            cam = C.apply_factor(cam0, f)
            out["cams"].setdefault(base, {})[fname] = C.bits(cam)
            rays = C.generate_rays(cam, 45.0, C.W, C.H, smp)
            assert np.array_equal(rays.view(np.uint32), kat_rays(oracle, cam, 45.0, C.W, C.H, smp).view(np.uint32)), \
                (scene, fname, "numpy GenerateRay differs from orc_kat_genray")
            key = f"{scene}|{fname}"
            bad = undefined(sc, rays)
            if bad.size:
                assert fname not in C.NO_SKIP, (key, bad.size)
                out["dropped"][key] = f"{bad.size} samples whose reference result is undefined (grid.h:46)"
                continue
            rec = ref_rays(tmp, path, rays, 1)
            hid = np.where(rec[:, 0] == 1, rec[:, 1], np.uint32(C.NOTRI)).astype("<u4")
            live = R.walk(sc, rays)
            lid = np.where(live["hit"], live["tri"], np.uint32(C.NOTRI)).astype("<u4")
            assert np.array_equal(hid, lid), (key, "reference vs occlusion_ref", int((hid != lid).sum()))
            one_case(key, scene, fname, cam, 45.0,
                     {"W": C.W, "H": C.H, "spp": C.SPP, "grid_res": 1, "cam": base, "hits_sha256": sha(hid.tobytes()),
                      "hit_samples": int((hid != C.NOTRI).sum())})
            if scene == "sliver9_4" and fname in ("identity", C.S1024, "scale_2^20"):
                out["sliver"]["gate_check"][fname] = gate_counts(exe, path, cam)
        print("cell scene", scene, flush=True)
    g = out["sliver"]["gate_check"]
    assert g["identity"]["wholly_gated_ok1"] == 0 and g["identity"]["violations"] == 0 and g["identity"]["gate_ok"], g
    assert g[C.S1024]["wholly_gated_ok1"] >= 1 and g["scale_2^20"]["wholly_gated_ok1"] >= 1, g
    # the sliver must be SEEN where the gate wrongly skips it: the reference hits it in the factor's frame
    assert out["cases"][f"sliver9_4|{C.S1024}"]["hit_samples"] > 0

    # ---- 64-cell scenes: refdriver render --view
    Wd, Ht, spp = C.CAM_FRAME
    for scene in C.GRID_SCENES:
        path = S.scene_file({"scene": scene}, tmp)
        hs = S.rtm.HostScene.load(path)
        try:
            cam0, fov = hs.cam.copy(), hs.fov
            sc = R.RefScene.from_host(hs)
        finally:
            hs.close()
        osc = S.OracleScene(oracle, path)
        smp = S.rtm.sample_table(spp)
        out["bases"][scene] = {"cam_bits": C.bits(cam0), "fov_bits": C.bits([fov])[0]}
        for fname, f in fac:
            cam = C.apply_factor(cam0, f)
            out["cams"].setdefault(scene, {})[fname] = C.bits(cam)
            out["cams"][scene]["fov_bits"] = C.bits([fov])[0]
            key = f"{scene}|{fname}"
            rays = C.generate_rays(cam, fov, Wd, Ht, smp)
            assert np.array_equal(rays.view(np.uint32), kat_rays(oracle, cam, fov, Wd, Ht, smp).view(np.uint32)), key
            bad = undefined(sc, rays)
            if bad.size:
                assert fname not in C.NO_SKIP, (key, bad.size)
                out["dropped"][key] = f"{bad.size} samples whose reference result is undefined (grid.h:46)"
                continue
            bgra, hits = G.render(tmp, path, Wd, Ht, spp, view=G.view_file(tmp, cam, fov))
            img, hid = osc.render(Wd, Ht, spp, cam=cam, fov=fov)
            assert img.astype("<u4").tobytes() == bgra and hid.astype("<u4").tobytes() == hits, (key, "reference vs restatement")
            one_case(key, scene, fname, cam, fov,
                     {"W": Wd, "H": Ht, "spp": spp, "grid_res": 64, "cam": scene, "bgra_sha256": sha(bgra),
                      "hits_sha256": sha(hits), "hit_samples": int((np.frombuffer(hits, "<u4") != C.NOTRI).sum())})
        osc.close()
        print("grid scene", scene, flush=True)
    for n in C.FACTOR_NAMES:
        kept = [k for k in out["cases"] if k.endswith("|" + n)]
        assert kept, ("every case of a factor was dropped: replace it", n)
    text = C.fixture_text(out)
    assert C.expand(json.loads(text)) == json.loads(json.dumps(out)), "the committed form does not expand to what was checked"
    with open(C.FIXTURE, "w") as f:
        f.write(text)
    print(f"wrote {len(out['cases'])} cases ({len(out['dropped'])} dropped), {os.path.getsize(C.FIXTURE)} bytes")
    for k, v in out["dropped"].items():
        print("  dropped", k, v)


if __name__ == "__main__":
    main()
