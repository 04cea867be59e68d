#!/usr/bin/env python3
"""oracle/gen_golden_synth.py -- TEST INFRASTRUCTURE ONLY; runs in the build container only.

Pins the synthetic scenes of tests/synth_scenes.py to the reference's OWN code (oracle/_ref/refdriver,
refdriver_instr, refdriver_bary: see oracle/Makefile).  The meshes are built with our host library
(HostScene.from_mesh ... save), one .rtscene per view since the camera is part of the file:

  tests/golden/synth/<name>.rtscene.gz          the scene file the tests load
  tests/golden/synth/<name>.bgra.gz             the reference's 62x46x4 frame
  tests/golden/synth/<name>.rec.gz              its per-sample records, all 11 columns (refdriver_instr,
                                                columns 0-7 checked equal to the plain refdriver's); kept only
                                                where the compressed file stays under REC_MAX_BYTES -- the
                                                column SHA-256s in synth.json pin the others
  tests/golden/synth/<name>.bary.rec.gz, alt_*  A2: IntersectRayTriBarycentric, brute force, ray march
  tests/golden/synth.json                       everything else: SHAs, grid properties, seeded cameras

A case that is not all-miss by design must have at least MIN_EACH hit and MIN_EACH miss samples in the
reference's records, or nothing is written for it: a view that sees nothing cannot be committed.

    make -C oracle ref && python oracle/gen_golden_synth.py
"""
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth_scenes as S   # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "refdriver")
REF_INSTR = os.path.join(ROOT, "oracle", "_ref", "refdriver_instr")
REF_BARY = os.path.join(ROOT, "oracle", "_ref", "refdriver_bary")
OUT = S.SYNTH
REC_MAX_BYTES = 96 << 10
MIN_EACH = 100
REF_TIMEOUT_S = 60


def run(args, exe=REF):
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True, timeout=REF_TIMEOUT_S).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def gz_bytes(data):
    import io
    b = io.BytesIO()
    with gzip.GzipFile(fileobj=b, mode="wb", mtime=0) as f:
        f.write(data)
    return b.getvalue()


def put(name, data):
    with open(os.path.join(OUT, name), "wb") as f:
        f.write(gz_bytes(data))


def view_file(tmp, cam, fov):
    vp = os.path.join(tmp, "v.view")
    with open(vp, "wb") as f:
        f.write(np.asarray(cam, "<f4").tobytes() + np.asarray([fov], "<f4").tobytes())
    return vp


def samples(tmp, path, Wd, Ht, spp, exe, rect=None, view=None):
    x0, y0, w, h = rect or (0, 0, Wd, Ht)
    rp = os.path.join(tmp, "s.rec")
    run(["samples", path, str(Wd), str(Ht), str(spp), str(x0), str(y0), str(w), str(h), rp] +
        (["--view", view] if view else []), exe=exe)
    words = 8 if exe == REF else 11
    a = np.fromfile(rp, "<u4").reshape(-1, words)
    os.remove(rp)
    return a


def render(tmp, path, Wd, Ht, spp, exe=REF, view=None):
    bp, hp = os.path.join(tmp, "f.bgra"), os.path.join(tmp, "f.hits")
    run(["render", path, str(Wd), str(Ht), str(spp), "--out", bp, "--hits", hp] + (["--view", view] if view else []),
        exe=exe)
    with open(bp, "rb") as f:
        b = f.read()
    with open(hp, "rb") as f:
        h = f.read()
    return b, h


def rec_entry(name, fname, rec, cols=("hit_tri", "tuv", "voxel", "rgb", "steps", "tests")):
    e = {"name": name}
    e.update(S.rec_shas(rec, cols))
    canon = rec.copy()
    canon[:, 2:8] = S.nan_canonical(canon[:, 2:8])
    e["nan_canonical_shas"] = S.rec_shas(canon, cols)
    data = gz_bytes(rec.tobytes())
    e["rec"] = fname if len(data) <= REC_MAX_BYTES else None
    if e["rec"]:
        with open(os.path.join(OUT, fname), "wb") as f:
            f.write(data)
    return e


def one_case(tmp, name, case):
    Wd, Ht, spp = S.W, S.H, S.SPP
    hs = S.build_host(case)
    path = os.path.join(tmp, name + ".rtscene")
    try:
        g, offs, _ = hs.grid()
        if case["dims"] is not None:
            assert g["dims"] == case["dims"], (name, g["dims"])
        hs.save(path)
        stats = dict(hs.stats)
    finally:
        hs.close()
    with open(path, "rb") as f:
        raw = f.read()
    e = ref_frame(tmp, name, name, path, (Wd, Ht, spp), case["all_miss"])
    put(name + ".rtscene.gz", raw)
    e.update({"rtscene_sha256": hashlib.sha256(raw).hexdigest(), "dims": g["dims"], "num_refs": stats["num_refs"],
              "max_refs_per_cell": stats["max_refs_per_cell"], "num_triangles": stats["num_triangles"],
              "aabb_min_bits": [f"{x:08x}" for x in g["aabb_min"].view(np.uint32)],
              "aabb_max_bits": [f"{x:08x}" for x in g["aabb_max"].view(np.uint32)]})
    if name in S.AXIS_CASES:
        e["axis_frame"] = ref_frame(tmp, name, f"{name}_{S.AXIS_FRAME[0]}x{S.AXIS_FRAME[1]}", path, S.AXIS_FRAME, False)
    print(f"{name}: dims {g['dims']} refs {stats['num_refs']} max/cell {stats['max_refs_per_cell']}", flush=True)
    return e, path


def ref_frame(tmp, scene, name, path, frame, all_miss):
    """One frame of one scene file through the reference: frame, hit IDs, records; the hit / miss condition."""
    Wd, Ht, spp = frame
    t0 = time.time()
    inst = samples(tmp, path, Wd, Ht, spp, REF_INSTR)
    plain = samples(tmp, path, Wd, Ht, spp, REF)
    assert np.array_equal(plain, inst[:, :8]), name
    bgra, hits = render(tmp, path, Wd, Ht, spp)
    nhit = int((inst[:, 0] == 1).sum())
    nmiss = inst.shape[0] - nhit
    if all_miss:
        assert nhit == 0, (name, nhit)
    else:
        assert nhit >= MIN_EACH and nmiss >= MIN_EACH, (name, nhit, nmiss)
    hid = np.where(inst[:, 0] == 1, inst[:, 1], np.uint32(0xFFFFFFFF)).astype("<u4")
    assert hid.tobytes() == hits, name
    put(name + ".bgra.gz", bgra)
    e = rec_entry(name, name + ".rec.gz", inst)
    e.update({"scene": scene, "W": Wd, "H": Ht, "spp": spp, "all_miss": all_miss, "hit_samples": nhit,
              "miss_samples": nmiss, "bgra": name + ".bgra.gz", "bgra_sha256": hashlib.sha256(bgra).hexdigest(),
              "hits_sha256": hashlib.sha256(hits).hexdigest(),
              "nan_samples": int(np.isnan(inst[:, 5:8].view(np.float32)).any(1).sum())})
    if frame == S.AXIS_FRAME:
        c = inst[(S.AXIS_PIXEL[1] * Wd + S.AXIS_PIXEL[0]) * spp]
        e["axis_sample"] = [f"{x:08x}" for x in c]
    print(f"  {name}: hit {nhit} miss {nmiss} records {'stored' if e['rec'] else 'as SHAs'} "
          f"reference {time.time() - t0:.1f} s", flush=True)
    return e


def bary_alt(tmp, name, path):
    """A2: the same view through IntersectRayTriBarycentric (whole frame) and, on windows around the frame
    centre, brute force and the ray march (records in the layout of tests/golden/alt)."""
    Wd, Ht, spp = S.W, S.H, S.SPP
    out = {}
    rec = samples(tmp, path, Wd, Ht, spp, REF_BARY)
    bgra, hits = render(tmp, path, Wd, Ht, spp, exe=REF_BARY)
    e = rec_entry(name, name + ".bary.rec.gz", rec)
    e.update({"bgra_sha256": hashlib.sha256(bgra).hexdigest(), "hits_sha256": hashlib.sha256(hits).hexdigest()})
    out["bary"] = e
    for mode, (x0, y0, w, h) in S.ALT_CROPS.items():
        rp = os.path.join(tmp, "alt.rec")
        run(["alt-samples", path, str(Wd), str(Ht), str(spp), str(x0), str(y0), str(w), str(h), mode, rp])
        with open(rp, "rb") as f:
            data = f.read()
        fname = f"alt_{mode}_{name}.rec.gz"
        put(fname, data)
        out[mode] = {"rec": fname, "x0": x0, "y0": y0, "w": w, "h": h}
    print("bary/alt", name, flush=True)
    return out


def big_frame(tmp, name, path):
    Wd, Ht, spp = S.BIG_FRAME
    bgra, hits = render(tmp, path, Wd, Ht, spp)
    print("big", name, flush=True)
    return {"W": Wd, "H": Ht, "spp": spp, "bgra_sha256": hashlib.sha256(bgra).hexdigest(),
            "hits_sha256": hashlib.sha256(hits).hexdigest(),
            "hit_samples": int((np.frombuffer(hits, "<u4") != 0xFFFFFFFF).sum())}


def cameras(tmp, paths):
    """A3: sixteen seeded cameras per scene (scene 1, scene 8, `inside`) at 96x54x4: the view's bits, the
    reference's frame and per-sample hit-ID SHA-256 (refdriver render --view)."""
    out = {}
    Wd, Ht, spp = S.CAM_FRAME
    with open(os.path.join(S.GOLD, "golden.json")) as f:
        gold = json.load(f)["scenes"]
    for sc in S.CAM_SCENES:
        if sc.startswith("scene"):
            path = os.path.join(ROOT, "data", "scenes", sc + ".rtscene")
            g = gold[sc[5:]]
            lo, hi = S.bits_f32(g["aabb_min_bits"]), S.bits_f32(g["aabb_max_bits"])
        else:
            path, lo, hi = paths[sc][0], S.bits_f32(paths[sc][1]["aabb_min_bits"]), S.bits_f32(paths[sc][1]["aabb_max_bits"])
        with open(path, "rb") as f:
            fov = float(np.frombuffer(f.read(80)[12:16], "<f4")[0])
        for vname, cam, vfov in S.seeded_cameras(lo, hi, fov):
            bgra, hits = render(tmp, path, Wd, Ht, spp, view=view_file(tmp, cam, vfov))
            out[f"{sc}_{vname}"] = {
                "scene": sc, "view": vname, "W": Wd, "H": Ht, "spp": spp,
                "cam_bits": [f"{x:08x}" for x in np.asarray(cam, "<f4").view("<u4")],
                "fov_bits": f"{int(np.asarray([vfov], '<f4').view('<u4')[0]):08x}",
                "bgra_sha256": hashlib.sha256(bgra).hexdigest(), "hits_sha256": hashlib.sha256(hits).hexdigest(),
                "hit_samples": int((np.frombuffer(hits, "<u4") != 0xFFFFFFFF).sum())}
        print("cameras", sc, flush=True)
    return out


def main():
    for exe in (REF, REF_INSTR, REF_BARY):
        if not os.path.exists(exe):
            sys.exit("build the reference drivers first: make -C oracle ref")
    # the axis ray of S.AXIS_FRAME needs the first Hammersley sample at (-0.5, -0.5)
    assert (S.rtm.sample_table(S.SPP)[0] == -0.5).all()
    os.makedirs(OUT, exist_ok=True)
    for f in os.listdir(OUT):
        os.remove(os.path.join(OUT, f))
    tmp = tempfile.mkdtemp()
    meta = {"generator": "oracle/gen_golden_synth.py via oracle/_ref/refdriver, refdriver_instr, refdriver_bary",
            "cases": {}, "dropped": {}, "bary_alt": {}, "big": {}}
    paths = {}
    for name, case in S.cases().items():
        try:
            e, path = one_case(tmp, name, case)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired, S.rtm.RtError) as x:
            meta["dropped"][name] = f"{type(x).__name__}: {x}"[:300]
            print("DROPPED", name, meta["dropped"][name], flush=True)
            continue
        meta["cases"][name] = e
        paths[name] = (path, e)
    for name in S.BARY_ALT:
        meta["bary_alt"][name] = bary_alt(tmp, name, paths[name][0])
    for name in S.BIG:
        meta["big"][name] = big_frame(tmp, name, paths[name][0])
    # the wide section's frame (tests/test_gpu_synth.py): enough work items per rank for both of its tiers
    meta["wide"] = ref_frame(tmp, "stack1500", "stack1500_%dx%d" % S.WIDE_FRAME[:2], paths["stack1500"][0],
                             S.WIDE_FRAME, False)
    meta["cameras"] = cameras(tmp, paths)
    with open(os.path.join(S.GOLD, "synth.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"wrote {len(os.listdir(OUT))} files, {total / 1e6:.2f} MB, and synth.json")


if __name__ == "__main__":
    main()
