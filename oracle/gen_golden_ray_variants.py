#!/usr/bin/env python3
"""oracle/gen_golden_ray_variants.py -- TEST INFRASTRUCTURE ONLY; runs in the build container only.

The eight ray families of tests/ray_sets.py on the seven scenes of tests/ray_variant_scenes.py, which reach the ray,
occlusion and AO kernels' other instantiations, and the expected records for them:

  tests/golden/ray_variants/<scene>.rays.gz    the rays, n x 6 f32 (origin, direction as passed)
  tests/golden/ray_variants/<scene>.rec.gz     n x 8 words: hit, tri, t, u, v, voxel, steps, tests
  tests/golden/ray_variants/huge_tri.out.gz    the huge scenes: `refdriver tri` on every (ray, appended triangle) pair,
                                               n x 4 words hit, t, u, v per scene, in HUGE_SCENES' order
  tests/golden/ray_variants/ray_variants.json  families, SHA-256s, counts, excluded rays, grid meta, mesh SHA-256s

The ribbons and sheets16: the records are the reference's OWN Grid::Intersect at the scene's grid resolution
(`refdriver_instr rays <scene> <in> <out> <grid_res>`), cross-checked against the plain refdriver on hit, tri, t, u, v;
before that the host builder's grid at that resolution is compared with `refdriver grid <scene> <out> <grid_res>`, the
whole export (meta and CSR): 513, 512 and 16 are not among the resolutions of tests/golden/grid.json.

The two huge scenes: the reference cannot build their grids (the appended triangle is listed by hand), so the records
are tests/occlusion_ref.py's walk over CallerBuilt's arrays, committed so that the CPU tests notice a drift; its
ray/triangle half is anchored to the reference's IntersectRayTri through `refdriver tri`.

Asserted before anything is written (on the reference's records, the restatement's for the huge scenes): per scene hits
and misses are each >= 20 % of the pinned rays; families A, B, E, G have >= 32 hits and >= 32 misses, D >= 16
(sheets16's B is waived by name: every interior ray hits a sheet); <= 0.5 % of a scene's rays are excluded (grid.h:46's
operand not finite or >= 2^30, as gen_golden_rays.py lists them); each huge scene has >= 100 closest hits on the
appended triangle; on huge_axis_z IntersectRayTri accepts >= 32 (ray, appended triangle) pairs with a non-finite u or v
(huge_stack2100's figure is recorded, and for both how many of them are a ray's closest-hit record: at least 1); over ray_sets.intervals the occluded count among the hits lies strictly between 0 and the hit count.

    make -C oracle ref && python oracle/gen_golden_ray_variants.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden_rays as G        # noqa: E402
import occlusion_ref as R          # noqa: E402
import ray_sets as RS              # noqa: E402
import ray_variant_scenes as V     # noqa: E402
import synth_scenes as S           # noqa: E402
from conftest import Oracle        # noqa: E402

REF_TIMEOUT_S = 300


def ref_rays(tmp, exe, path, rays, res):
    """`refdriver rays ... <res>` on rays f32 [n, 6] -> records u32 [n, 8]."""
    rp, op = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.rec")
    np.ascontiguousarray(rays, "<f4").tofile(rp)
    subprocess.run([exe, "rays", path, rp, op, str(res)], check=True, capture_output=True, timeout=REF_TIMEOUT_S)
    rec = np.fromfile(op, "<u4").reshape(-1, 8)
    assert rec.shape[0] == rays.shape[0]
    return rec


def ref_tri(tmp, pairs):
    """`refdriver tri` on pairs f32 [n, 15] -> u32 [n, 4]: hit, t, u, v of the reference's IntersectRayTri."""
    rp, op = os.path.join(tmp, "pairs.f32"), os.path.join(tmp, "pairs.out")
    np.ascontiguousarray(pairs, "<f4").tofile(rp)
    subprocess.run([G.REF, "tri", rp, op], check=True, capture_output=True, timeout=REF_TIMEOUT_S)
    out = np.fromfile(op, "<u4").reshape(-1, 4)
    assert out.shape[0] == pairs.shape[0]
    return out


def grid_export(sc):
    """The host builder's grid in `refdriver grid`'s layout: dims, aabb_min, aabb_max, cell_wdh, inv_cell_wdh, ncells,
    nrefs, offsets, refs."""
    gm = sc.gm
    return np.concatenate([np.array(gm["dims"], "<u4"), gm["aabb_min"].view("<u4"), gm["aabb_max"].view("<u4"),
                           np.array([gm["cell_wdh"], gm["inv_cell_wdh"]], "<f4").view("<u4"),
                           np.array([sc.ref.offs.size - 1, sc.num_refs], "<u4"),
                           sc.ref.offs.astype("<u4"), sc.ref.cell_tris.astype("<u4")])


def canon(words, cols):
    out = np.array(words, np.uint32)
    out[:, cols] = S.nan_canonical(out[:, cols])
    return out


def one_scene(tmp, oracle, name):
    sc = V.Scene(name, tmp)
    try:
        sc.check_static()
        cam = G.camera_rays(oracle, sc.host)
        res = V.GRID_RES.get(name)
        if res:
            path = os.path.join(tmp, name + ".rtscene")
            sc.save(path)
            gp = os.path.join(tmp, "grid.bin")
            subprocess.run([G.REF, "grid", path, gp, str(res)], check=True, capture_output=True, timeout=REF_TIMEOUT_S)
            assert np.array_equal(np.fromfile(gp, "<u4"), grid_export(sc)), (name, "host grid differs from the reference's")
            crec = ref_rays(tmp, G.REF_INSTR, path, cam, res)
        else:
            crec = V.rec8(R.walk(sc.ref, cam, mode="closest"))
        rays, lat = RS.build(name, sc.gm, sc.ray_mesh[0], sc.ray_mesh[1], cam, crec[:, 0] == 1, crec[:, 2].view(np.float32))

        box = RS.Box(sc.gm)
        assert np.isfinite(rays).all()
        assert np.abs(rays[:, :3]).max() <= 2.0 ** 21 * float(box.diag)
        dm = np.abs(rays[:, 3:]).max(1).astype(np.float64)
        scale = max(1.0, float(box.diag))
        # (gen_golden_rays.py's bounds; an aimed direction is a difference of two points of the box, so on a ribbon,
        # 0.01 across, the lower one scales with the box's smallest extent)
        small = min(1.0, float(box.ext.min()))
        assert dm.min() >= 2.0 ** -20 / 64 * small and dm.max() <= 2.0 ** 20 * 4 * scale, (name, dm.min(), dm.max())

        if res:
            rec = ref_rays(tmp, G.REF_INSTR, path, rays, res)
            plain = ref_rays(tmp, G.REF, path, rays, res)
            assert np.array_equal(plain[:, :5], rec[:, :5]) and (plain[:, 5:] == 0).all(), name
            source = "Grid::Intersect (refdriver_instr rays, grid_res %d)" % res
        else:
            rec = V.rec8(R.walk(sc.ref, rays, mode="closest"))
            source = "tests/occlusion_ref.py walk over CallerBuilt's arrays"
        miss = rec[:, 0] == 0
        assert (rec[miss, 1] == RS.NOTRI).all() and (rec[miss, 2:5] == 0).all()

        excluded = [{"index": int(i), "family": next(n for n, (a, b) in RS.bounds().items() if a <= i < b),
                     "reference": "grid.h:46",
                     "reason": "int() of a float that is NaN, infinite or >= 2^30 in ToVoxel: the entry point is "
                               "o + d * enter_t with a NaN enter_t (0 * inf in the x slab of IntersectRayAABB, aabb.h)"}
                    for i in G.undefined_rays(sc.ref, rays)]
        assert len(excluded) <= RS.MAX_EXCLUDED_SHARE * RS.TOTAL, (name, len(excluded))
        keep = np.ones(RS.TOTAL, bool)
        keep[[x["index"] for x in excluded]] = False

        counts = RS.counts(rec, keep)
        bad = V.check_non_vacuity(name, counts)
        assert not bad, bad
        hit = keep & (rec[:, 0] == 1)
        tmm = RS.intervals(rays, rec, sc.ref.diagonal())
        occ = R.walk(sc.ref, rays, tmm, mode="any")["occluded"]
        assert 0 < int(occ[hit].sum()) < int(hit.sum()), (name, int(occ[hit].sum()), int(hit.sum()))
        extra = {"occluded": int(occ[keep].sum()), "occluded_hits": int(occ[hit].sum()), "longest_walk": int(rec[keep, 6].max())}
        tri_out = None
        if sc.big is not None:
            tri_out = ref_tri(tmp, sc.big_pairs(rays))
            k = np.full(RS.TOTAL, sc.big)
            h, t, u, v = R.ray_tri(rays[:, :3], rays[:, 3:], sc.ref.v0[k], sc.ref.v1[k], sc.ref.v2[k])
            assert np.array_equal(tri_out[:, 0], h.astype(np.uint32)), (name, "ray_tri's hit vs IntersectRayTri")
            mine = np.stack([t, u, v], axis=1).astype(np.float32).view(np.uint32)
            on = tri_out[:, 0] == 1
            assert np.array_equal(canon(tri_out[on, 1:], [0, 1, 2]), canon(mine[on], [0, 1, 2])), (name, "ray_tri's t, u, v")
            uv = rec[:, 3:5].view(np.float32)
            big_hits = hit & (rec[:, 1] == sc.big)
            extra["big_tri_hits"] = int(big_hits.sum())
            extra["big_tri_pair_hits"] = int(on.sum())
            # hits IntersectRayTri accepts with a non-finite u or v (u < 0 || u > 1 is false for a NaN), among the
            # (ray, appended triangle) pairs; and how many of them end up as a ray's closest-hit record
            extra["nonfinite_uv_pair_hits"] = int((on & ~np.isfinite(tri_out[:, 2:].view(np.float32)).all(1)).sum())
            extra["nonfinite_uv_records"] = int((hit & ~np.isfinite(uv).all(1)).sum())
            assert extra["big_tri_hits"] >= V.MIN_BIG_TRI_HITS, (name, extra)
            assert extra["nonfinite_uv_pair_hits"] >= V.MIN_NONFINITE_UV.get(name, 0), (name, extra)
            assert extra["nonfinite_uv_records"] >= 1, (name, extra)

        rdata, cdata = G.gz_bytes(rays.astype("<f4").tobytes()), G.gz_bytes(rec.astype("<u4").tobytes())
        assert len(rdata) < V.MAX_FILE and len(cdata) < V.MAX_FILE, (name, len(rdata), len(cdata))
        gm = sc.gm
        entry = {"rays": name + ".rays.gz", "rec": name + ".rec.gz", "n": RS.TOTAL, "records_from": source,
                 "rays_sha256": RS.sha256(rdata), "rec_sha256": RS.sha256(cdata),
                 "families": {n: list(ab) for n, ab in RS.bounds().items()},
                 "counts": counts, "excluded": excluded, "waived": [f for s, f in V.WAIVED if s == name],
                 "mesh": sc.mesh_shas(), "num_refs": sc.num_refs, "grid_res": res if res else 64, "info": V.INFO[name],
                 "grid": {"dims": [int(x) for x in gm["dims"]],
                          "aabb_min_bits": [f"{x:08x}" for x in gm["aabb_min"].view(np.uint32)],
                          "aabb_max_bits": [f"{x:08x}" for x in gm["aabb_max"].view(np.uint32)],
                          "cell_wdh_bits": f"{int(np.float32(gm['cell_wdh']).view(np.uint32)):08x}"}}
        entry.update(extra)
        print(f"{name}: hits/misses " + " ".join(f"{n} {counts[n][0]}/{counts[n][1]}" for n in RS.NAMES) +
              f"; total {int(hit.sum())}/{int((keep & miss).sum())}; excluded {len(excluded)}; {extra}; "
              f"{len(rdata)} + {len(cdata)} bytes", flush=True)
        return entry, rdata, cdata, tri_out
    finally:
        sc.close()


def main():
    for exe in (G.REF, G.REF_INSTR):
        if not os.path.exists(exe):
            sys.exit("build the reference drivers first: make -C oracle ref")
    oracle = Oracle()
    tmp = tempfile.mkdtemp()
    out = {"generator": "oracle/gen_golden_ray_variants.py via oracle/_ref/refdriver_instr and refdriver, commands "
                        "`rays <grid_res>`, `grid <grid_res>` and `tri`",
           "record": list(RS.REC_COLS), "huge_tri": "huge_tri.out.gz", "scenes": {}}
    files, tri = {}, []
    for name in V.SCENES:
        entry, rdata, cdata, tri_out = one_scene(tmp, oracle, name)
        out["scenes"][name] = entry
        files[entry["rays"]], files[entry["rec"]] = rdata, cdata
        if tri_out is not None:
            tri.append(tri_out)
    assert len(tri) == len(V.HUGE_SCENES)
    tdata = G.gz_bytes(np.concatenate(tri).astype("<u4").tobytes())
    assert len(tdata) < V.MAX_FILE, len(tdata)
    files[out["huge_tri"]] = tdata
    out["huge_tri_sha256"] = RS.sha256(tdata)
    os.makedirs(V.DIR, exist_ok=True)
    for f in os.listdir(V.DIR):
        os.remove(os.path.join(V.DIR, f))
    for name, data in files.items():
        with open(os.path.join(V.DIR, name), "wb") as f:
            f.write(data)
    with open(os.path.join(V.DIR, "ray_variants.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(files)} files, {sum(len(d) for d in files.values()) / 1e6:.2f} MB, and ray_variants.json")


if __name__ == "__main__":
    main()
