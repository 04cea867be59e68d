#!/usr/bin/env python3
"""Measures rt_trace_rays_device (GpuScene.trace_rays) on scenes 8 and 1 at 1920x1080x4 and writes
profiles/rays_bench.json (with the loaded library's rt_build_hash).

Legs, each in rays/s between HIP events on the launch stream -- 0.2 s of the leg's own launches to bring the
clocks up (as bench.py does), `--warmup` launches, then the median of 5 samples of `--steps` launches and the
spread (max - min) / median of the five:
  (a) camera order: the frame's rays from primary_rays, next to render_frame_device's samples/s for the same
      frame from the PARENT build (--parent-lib, a librt_tracer.so of the parent commit in the package
      directory) and from this build, same session, and the ratio -- the price of per-lane origins and 48-byte
      records against the per-camera-origin records;
  (b) the same rays shuffled with PCG64(41);
  (c) one ambient-occlusion bounce: 4 seeded hemisphere rays per primary hit, from the hit point pushed off
      the surface;
  (d) (b) and (c) with RT_RAYS_SORT, the sort's own kernels inside the timed span (arm `this_sorted` of those
      legs; `d_sort` holds the comparison, and the sorted call on camera-order rays, where it can only cost).
--ab-lib NAME=LIB adds the same legs from another build of the library in the package directory (how the
lock-step walk was measured, profiles/rays_walk_ab.json), samples interleaved with this build's, and checks
that its results are the same bits.

--occlusion measures rt_occluded_rays_device (GpuScene.occluded) instead, against trace_rays on the same rays in the
same session, into profiles/occlusion_bench.json (occlusion_legs).

--ao measures rt_render_ao_device (GpuScene.render_ao), the AO frame in one launch, against the composition it fuses
on the same frame, in the same session, into profiles/ao_bench.json (ao_legs).

--distance measures rt_distance_points_device (GpuScene.distance) on jittered hit points and uniform points: the
default arm against RT_DIST_EXHAUSTIVE and a chunked torch brute force, into profiles/distance_bench.json
(distance_legs).

--march measures rt_march_rays_device (GpuScene.march) on the 1920x1080x1 camera rays: the fused call against the
loop of GpuScene.distance calls it replaces, RT_MARCH_EXHAUSTIVE, the other seed and the arm without the early stop
(--ab-lib builds of tools/build_variant.sh) and the RT_ISECT_RAY_MARCH frame, into profiles/march_bench.json
(march_legs).

    python3 tools/bench_rays.py --parent-lib librt_tracer_parent.so [--ab-lib other=librt_tracer_other.so]
    python3 tools/bench_rays.py --occlusion
    python3 tools/bench_rays.py --ao
    python3 tools/bench_rays.py --distance
    python3 tools/bench_rays.py --crossings
    tools/build_variant.sh seedmorton -DRT_MARCH_SEED=0 && tools/build_variant.sh nostop -DRT_MARCH_STOP=0 &&
        python3 tools/bench_rays.py --march --ab-lib seed_morton=librt_tracer_seedmorton.so --ab-lib no_stop=librt_tracer_nostop.so
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch  # first: share torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INIT = os.path.join(ROOT, "cpp-11-ray-trace-march-framework_amd", "__init__.py")
W, H, SPP = 1920, 1080, 4
AO_PER_HIT = 4
AO_OFFSET = 1e-4            # of the grid's largest extent: the bounce origin's push along the facing normal


def load(name, lib):
    if lib:
        os.environ["RT_TRACER_LIB"] = lib
    spec = importlib.util.spec_from_file_location(name, INIT)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    m.tracer_lib()
    m.host_lib()
    os.environ.pop("RT_TRACER_LIB", None)
    return m


def sample(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps            # ms per launch


def warm(fn, warmup, clock_warmup=0.2):
    t_end = time.perf_counter() + clock_warmup
    while time.perf_counter() < t_end:
        fn()
        torch.cuda.synchronize()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()


def measure(fns, n_items, steps, warmup, per_arm=None):
    """fns: {arm: callable}; samples interleaved over the arms.  Per arm: median ms, items/s, spread.
    per_arm: {arm: (steps, warmup, n_items)} for arms that are timed over fewer launches or items."""
    per_arm = per_arm or {}
    for k, fn in fns.items():
        w = per_arm.get(k, (steps, warmup, n_items))[1]
        warm(fn, w, clock_warmup=0.2 if w == warmup else 0.0)
    ms = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            ms[k].append(sample(fn, per_arm.get(k, (steps, warmup, n_items))[0]))
    out = {}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = {"ms": round(med, 4), "per_s": round(per_arm.get(k, (steps, warmup, n_items))[2] / (med * 1e-3), 1),
                  "spread": round((max(v) - min(v)) / med, 4), "samples_ms": [round(x, 4) for x in v]}
    return out


def ao_rays(rays, hits, tri_n, ext, seed=43):
    """4 seeded directions in the hemisphere of the hit triangle's face normal turned against the incoming
    ray, from the hit point pushed AO_OFFSET * ext along that normal (torch, on the device)."""
    g = torch.Generator(device=rays.device)
    g.manual_seed(seed)
    tri = hits[:, 0]
    hit = tri != -1
    t = hits[hit, 1].view(torch.float32)
    o, d = rays[hit, :3], rays[hit, 3:]
    n = tri_n[tri[hit].long()]
    n = torch.where((n * d).sum(1, keepdim=True) > 0, -n, n)
    p = o + d * t[:, None] + n * (AO_OFFSET * ext)
    p, n = p.repeat_interleave(AO_PER_HIT, 0), n.repeat_interleave(AO_PER_HIT, 0)
    v = torch.randn(p.shape, generator=g, device=rays.device, dtype=torch.float32)
    v = v / v.norm(dim=1, keepdim=True)
    v = torch.where((v * n).sum(1, keepdim=True) < 0, -v, v)
    return torch.cat([p, v], 1).contiguous()


def occlusion_legs(args):
    """--occlusion: rt_occluded_rays_device (GpuScene.occluded) against rt_trace_rays_device ON THE SAME RAYS, the two
    arms' samples interleaved (measure), into profiles/occlusion_bench.json:
      camera order and shuffled (PCG64(41)) over the infinite interval;
      the ambient-occlusion bounce of leg (c) with tmin = 1e-4 x the box diagonal and tmax = +inf / 0.1 x the diagonal;
      the bounce with RT_RAYS_SORT in both arms.
    Per leg: both arms' ms, rays/s and spread, speedup = trace ms / occluded ms, and `slower`: the occlusion arm is
    slower by more than the larger spread.  `consistent`: over the infinite interval the bytes equal the closest
    call's hit; with an interval they imply it (include/rt_tracer.h)."""
    rtm = load("rtm_this", None)
    res = {"tool": "tools/bench_rays.py --occlusion", "frame": [W, H, SPP], "steps": args.steps, "warmup": args.warmup,
           "samples": 5, "build_hash": rtm.library_build_hash(), "device": torch.cuda.get_device_name(0), "scenes": {}}
    st = torch.cuda.current_stream().cuda_stream
    n = W * H * SPP
    for sid in args.scenes:
        hs = rtm.HostScene.load(sid)
        gs = rtm.GpuScene(hs, 0)
        rays = gs.primary_rays(gs.frame(W, H, SPP))
        torch.cuda.synchronize()
        meta = hs.grid()[0]
        e = (meta["aabb_max"] - meta["aabb_min"]).astype(np.float64)
        diag = float(np.sqrt((e * e).sum()))
        entry = {"box_diagonal": diag}

        def leg(r, tmin=None, tmax=None, sort=False):
            tmm = None
            if tmin is not None:
                tmm = torch.empty((r.shape[0], 2), dtype=torch.float32, device=r.device)
                tmm[:, 0], tmm[:, 1] = tmin, tmax
            hit = gs.trace_rays(r).hits[:, 0] != -1
            occ = gs.occluded(r, tmm) != 0
            same_sorted = bool(torch.equal(gs.occluded(r, tmm, sort=True) != 0, occ))
            consistent = bool(torch.equal(occ, hit)) if tmm is None else bool((hit | ~occ).all())
            out = measure({"trace_rays": lambda: gs.trace_rays(r, sort=sort, stream=st),
                           "occluded": lambda: gs.occluded(r, tmm, sort=sort, stream=st)}, r.shape[0], args.steps, args.warmup)
            for k in out:
                out[k]["unit"] = "rays/s"
            a, b = out["trace_rays"], out["occluded"]
            spread = max(a["spread"], b["spread"])
            return {"rays": int(r.shape[0]), "closest_hits": int(hit.sum()), "occluded": int(occ.sum()),
                    "tmin": tmin, "tmax": None if tmax is None else (tmax if np.isfinite(tmax) else "inf"), "sort": sort,
                    "consistent": consistent, "sorted_same_bytes": same_sorted, **out,
                    "speedup": round(a["ms"] / b["ms"], 3), "larger_spread": spread,
                    "slower": bool(b["ms"] > a["ms"] * (1.0 + spread))}

        entry["camera_order"] = leg(rays)
        perm = torch.from_numpy(np.random.Generator(np.random.PCG64(41)).permutation(n)).cuda()
        entry["shuffled"] = leg(rays[perm].contiguous())
        v, t = hs.mesh()
        tri_n = torch.from_numpy(np.ascontiguousarray(t[:, 3:6]).view(np.float32).copy()).cuda()
        ao = ao_rays(rays, gs.trace_rays(rays).hits, tri_n, float((meta["aabb_max"] - meta["aabb_min"]).max()))
        tmin, short = 1e-4 * diag, 0.1 * diag
        entry["ao_tmax_inf"] = leg(ao, tmin, float("inf"))
        entry["ao_tmax_short"] = leg(ao, tmin, short)
        entry["ao_tmax_inf_sorted"] = leg(ao, tmin, float("inf"), sort=True)
        entry["ao_tmax_short_sorted"] = leg(ao, tmin, short, sort=True)
        res["scenes"][str(sid)] = entry
        print(json.dumps({str(sid): entry}), flush=True)
        gs.close()
        hs.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


def ao_compose(rtm, gs, f, dirs, rot, tmin, tmax, e1, e2, st, parts=None):
    """The composition rt_render_ao_device fuses, on the device: primary_rays -> trace_rays -> the contract's steps 4-5
    in torch (tests/ao_ref.py's operations, one torch operation each) -> occluded -> counts and the resolve in torch.
    -> (pixels int32 [H, W], counts uint8 [H, W, spp]).  parts: a dict that receives the AO rays and intervals (for the
    legs that time the library calls alone)."""
    Wf, Hf, spp = f.width, f.height, max(1, f.spp)
    K = dirs.shape[0]
    rays = gs.primary_rays(f, stream=st)
    hits = gs.trace_rays(rays, stream=st).hits
    tri = hits[:, 0]
    idx = (tri != -1).nonzero().squeeze(1)
    t = hits[idx, 1].view(torch.float32)
    o, d = rays[idx, :3], rays[idx, 3:]
    a, b = e1[tri[idx].long()], e2[tri[idx].long()]
    g = torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    n = g / torch.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])[:, None]
    flip = ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]) > 0
    n = torch.where(flip[:, None], -n, n)
    p = o + t[:, None] * d
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    sg = torch.copysign(torch.ones_like(nz), nz)
    fa = -1.0 / (sg + nz)
    fb = (nx * ny) * fa
    t1 = torch.stack([1.0 + (sg * (nx * nx)) * fa, sg * fb, -(sg * nx)], 1)
    t2 = torch.stack([fb, sg + (ny * ny) * fa, -ny], 1)
    lx, ly, lz = dirs[None, :, 0], dirs[None, :, 1], dirs[None, :, 2]
    if rot is not None:
        s_ = idx % spp
        x_ = (idx // spp) % Wf
        y_ = idx // (spp * Wf)
        j = ((x_ & 3) | ((y_ & 3) << 2)) ^ (s_ & 15)
        c, sn = rot[j, 0][:, None], rot[j, 1][:, None]
        lx, ly = c * lx - sn * ly, sn * lx + c * ly
    w = (lx[:, :, None] * t1[:, None, :] + ly[:, :, None] * t2[:, None, :]) + lz[:, :, None] * n[:, None, :]
    ao = torch.cat([p[:, None, :].expand(-1, K, -1), w], 2).reshape(-1, 6).contiguous()
    tmm = torch.empty((ao.shape[0], 2), dtype=torch.float32, device=ao.device)
    tmm[:, 0], tmm[:, 1] = tmin, tmax
    if parts is not None:
        parts["rays"], parts["ao"], parts["tmm"] = rays, ao, tmm
    occ = gs.occluded(ao, tmm, stream=st)
    cnt = torch.full((Wf * Hf * spp,), 255, dtype=torch.uint8, device=ao.device)
    cnt[idx] = occ.view(-1, K).sum(1, dtype=torch.int32).to(torch.uint8)
    cnt = cnt.view(Hf, Wf, spp)
    y = torch.arange(Hf, device=ao.device, dtype=torch.float32)[:, None, None]
    col = torch.where(cnt == 255, (y / float(Hf)).expand(-1, Wf, spp), (float(K) - cnt.to(torch.float32)) / float(K))
    total = col[:, :, 0]
    for k in range(1, spp):
        total = total + col[:, :, k]
    gch = torch.sqrt(total * (1.0 / spp))
    ch = torch.where(gch > 1.0, torch.full_like(gch, 255.0), torch.trunc(gch * 255.0)).to(torch.int32) & 255
    return (ch << 16) | (ch << 8) | ch, cnt


def ao_legs(args):
    """--ao: per scene, K in {4, 16}, tmin = 1e-4 x the box diagonal, tmax = +inf and 0.1 x the diagonal, rotated, the
    built-in table, into profiles/ao_bench.json.  Arms, samples interleaved (measure), ms per frame:
      fused            rt_render_ao_device, with d_counts;
      composition      ao_compose: the three library calls and the torch kernels between them;
      primary_rays, trace_rays, occluded   each library call of the composition alone, on the composition's own rays.
    three_call_sum = the last three; fused_over_three_calls and fused_over_composition are ms ratios (below 1: the
    fused call is faster); `slower_than_three_calls`: by more than the larger spread of
    fused, trace_rays and occluded.  same_counts / same_pixels: the
    share of the fused call's bytes / words the composition reproduces (torch's kernels are not held to the
    contract's roundings; the tests compare against numpy)."""
    rtm = load("rtm_this", None)
    res = {"tool": "tools/bench_rays.py --ao", "frame": [W, H, SPP], "steps": args.steps, "warmup": args.warmup,
           "samples": 5, "build_hash": rtm.library_build_hash(), "device": torch.cuda.get_device_name(0),
           "arm_b": "removed: the packing arm lost every leg to arm A (DESIGN.md 4.30); the committed "
                    "profiles/ao_bench.json was written while it existed and holds its figures (fused_pack)", "scenes": {}}
    st = torch.cuda.current_stream().cuda_stream
    n = W * H * SPP
    rot = torch.from_numpy(rtm.ao_rotations()).cuda()
    for sid in args.scenes:
        hs = rtm.HostScene.load(sid)
        gs = rtm.GpuScene(hs, 0)
        f = gs.frame(W, H, SPP)
        meta = hs.grid()[0]
        e = (meta["aabb_max"] - meta["aabb_min"]).astype(np.float64)
        diag = float(np.sqrt((e * e).sum()))
        v, t = hs.mesh()
        pos = np.ascontiguousarray(v[:, :3], np.float32)
        ti = t[:, :3].astype(np.int64)
        e1 = torch.from_numpy(pos[ti[:, 1]] - pos[ti[:, 0]]).cuda()
        e2 = torch.from_numpy(pos[ti[:, 2]] - pos[ti[:, 0]]).cuda()
        entry = {"box_diagonal": diag}
        out = torch.empty((H, W), dtype=torch.int32, device="cuda")
        for K in (4, 16):
            dirs = torch.from_numpy(rtm.ao_table(K)).cuda()
            for label, tmax in (("inf", float("inf")), ("short", 0.1 * diag)):
                tmin = 1e-4 * diag
                parts = {}
                pix, cnt = ao_compose(rtm, gs, f, dirs, rot, tmin, tmax, e1, e2, st, parts)
                fpix, fcnt = gs.render_ao(f, K, tmin, tmax, counts=True)
                torch.cuda.synchronize()
                same_c = float((fcnt == cnt).float().mean())
                same_p = float((fpix.view(torch.int32) == pix).float().mean())
                rays, ao, tmm = parts["rays"], parts["ao"], parts["tmm"]
                hit = fcnt != 255
                m = measure({"fused": lambda: gs.render_ao(f, K, tmin, tmax, out=out, counts=True, stream=st),
                             "composition": lambda: ao_compose(rtm, gs, f, dirs, rot, tmin, tmax, e1, e2, st),
                             "primary_rays": lambda: gs.primary_rays(f, stream=st),
                             "trace_rays": lambda: gs.trace_rays(rays, stream=st),
                             "occluded": lambda: gs.occluded(ao, tmm, stream=st)}, n, args.steps, args.warmup)
                for k in m:
                    m[k]["unit"] = "samples/s"
                three = m["primary_rays"]["ms"] + m["trace_rays"]["ms"] + m["occluded"]["ms"]
                # (primary_rays is 0.04 ms of the sum and its spread is launch jitter: it does not enter the comparison)
                spread = max(m[k]["spread"] for k in ("fused", "trace_rays", "occluded"))
                entry[f"K{K}_tmax_{label}"] = {
                    "K": K, "tmin": tmin, "tmax": "inf" if label == "inf" else tmax, "hit_samples": int(hit.sum()),
                    "ao_rays": int(ao.shape[0]), "occluded_share": round(float(fcnt[hit].float().sum()) / max(1, ao.shape[0]), 4),
                    "same_counts": round(same_c, 6), "same_pixels": round(same_p, 6), **m,
                    "three_call_sum_ms": round(three, 4), "fused_over_three_calls": round(m["fused"]["ms"] / three, 3),
                    "fused_over_composition": round(m["fused"]["ms"] / m["composition"]["ms"], 3), "larger_spread": spread,
                    "slower_than_three_calls": bool(m["fused"]["ms"] > three * (1.0 + spread)),
                    "composition_bytes": int(n * 40 + ao.shape[0] * 33), "fused_bytes": int(W * H * 4 + n)}
                del parts, rays, ao, tmm, pix, cnt
                torch.cuda.empty_cache()
        res["scenes"][str(sid)] = entry
        print(json.dumps({str(sid): entry}), flush=True)
        gs.close()
        hs.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


def torch_brute_distance(points, v0, v1, v2, chunk=1024):
    """What a caller has without GpuScene.distance: DistancePointTri's formulas (inside branch or the nearest of the
    three edges) over points x triangles in float32 torch, `chunk` points at a time, reduced with min.  torch fuses
    and orders the sums as it likes, so the result is NOT the reference's bits."""
    e0, e1, e12 = v2 - v0, v1 - v0, v2 - v1
    d00, d01, d11, d1212 = (e0 * e0).sum(1), (e0 * e1).sum(1), (e1 * e1).sum(1), (e12 * e12).sum(1)
    inv = 1.0 / (d00 * d11 - d01 * d01)
    out = torch.empty(points.shape[0], dtype=torch.float32, device=points.device)

    def seg(p, a, ab, ll):
        t = (((p[:, None, :] - a[None]) * ab[None]).sum(2) / ll[None]).clamp(0.0, 1.0)
        q = a[None] + t[:, :, None] * ab[None]
        return ((p[:, None, :] - q) ** 2).sum(2)

    for i in range(0, points.shape[0], chunk):
        p = points[i:i + chunk]
        w = p[:, None, :] - v0[None]
        d02, d12 = (w * e0[None]).sum(2), (w * e1[None]).sum(2)
        u = (d00[None] * d12 - d01[None] * d02) * inv[None]
        v = (d11[None] * d02 - d01[None] * d12) * inv[None]
        q = v1[None] * u[:, :, None] + v2[None] * v[:, :, None] + v0[None] * (1.0 - u - v)[:, :, None]
        inside = ((p[:, None, :] - q) ** 2).sum(2)
        edges = torch.minimum(seg(p, v0, e1, d11), torch.minimum(seg(p, v0, e0, d00), seg(p, v1, e12, d1212)))
        d2 = torch.where((u >= 0) & (v >= 0) & (u + v < 1), inside, edges)
        out[i:i + chunk] = torch.nan_to_num(d2, nan=float("inf")).min(1).values.sqrt()
    return out


def distance_legs(args):
    """--distance: rt_distance_points_device (GpuScene.distance) into profiles/distance_bench.json.  Points: the hit
    points of the 1920x1080x1 primary rays jittered by a normal of 1 % of the box diagonal (seed 47) -- in camera
    order, shuffled (PCG64(41)), shuffled with RT_DIST_SORT -- and as many uniform points in 1.5 x the box.  Arms,
    samples interleaved (measure): the default (the box hierarchy), RT_DIST_EXHAUSTIVE, and a chunked float32 torch
    brute force (torch_brute_distance: what a caller has today; not bit-exact; timed over the leg's first
    TORCH_POINTS points).  `beats_exhaustive`: the default arm is faster by more than the larger spread."""
    TORCH_POINTS = 1 << 15
    rtm = load("rtm_this", None)
    res = {"tool": "tools/bench_rays.py --distance", "frame": [W, H, 1], "steps": args.steps, "warmup": args.warmup,
           "samples": 5, "build_hash": rtm.library_build_hash(), "device": torch.cuda.get_device_name(0),
           "torch_arm": f"chunked float32 brute force over the first {TORCH_POINTS} points of a leg; not bit-exact",
           "flat_sweep": "the flat sweep of all block boxes (compile-time RT_DIST_FLAT) lost to the hierarchy and was "
                         "removed; profiles/distance_bench.json was written while it existed and holds its figures "
                         "(flat_sweep_ab), and the culled kernel's on scene 1 (small_mesh_culled)",
           "scenes": {}}
    st = torch.cuda.current_stream().cuda_stream
    for sid in args.scenes:
        hs = rtm.HostScene.load(sid)
        gs = rtm.GpuScene(hs, 0)
        rays = gs.primary_rays(gs.frame(W, H, 1))
        hits = gs.trace_rays(rays)
        hit = hits.hits[:, 0] != -1
        v, t = hs.mesh()
        pos = torch.from_numpy(np.ascontiguousarray(v[:, :3])).cuda()
        idx = torch.from_numpy(np.ascontiguousarray(t[:, :3]).astype(np.int64)).cuda()
        v0, v1, v2 = pos[idx[:, 0]].contiguous(), pos[idx[:, 1]].contiguous(), pos[idx[:, 2]].contiguous()
        lo, hi = pos.min(0).values, pos.max(0).values
        diag = float((hi - lo).norm())
        g = torch.Generator(device="cuda")
        g.manual_seed(47)
        p = rays[hit, :3] + rays[hit, 3:] * hits.t[hit][:, None]
        p = (p + torch.randn(p.shape, generator=g, device="cuda") * (0.01 * diag)).contiguous()
        n = p.shape[0]
        perm = torch.from_numpy(np.random.Generator(np.random.PCG64(41)).permutation(n)).cuda()
        mid = 0.5 * (lo + hi)
        uni = (mid + (torch.rand((n, 3), generator=g, device="cuda") - 0.5) * 1.5 * (hi - lo)).contiguous()
        torch.cuda.synchronize()
        entry = {"triangles": int(t.shape[0]), "points": int(n), "box_diagonal": diag}

        def leg(q, sort=False):
            a = gs.distance(q, closest=True, sort=sort)
            b = gs.distance(q, closest=True, sort=sort, exhaustive=True)
            same = bool(torch.equal(a.raw, b.raw) and torch.equal(a.closest.view(torch.int32), b.closest.view(torch.int32)))
            sub = q[:TORCH_POINTS].contiguous()
            tb = torch_brute_distance(sub, v0, v1, v2)
            err = float((tb - a.dist[:sub.shape[0]]).abs().max())
            out = measure({"default": lambda: gs.distance(q, sort=sort, stream=st),
                           "exhaustive": lambda: gs.distance(q, sort=sort, exhaustive=True, stream=st),
                           "torch_brute_force": lambda: torch_brute_distance(sub, v0, v1, v2)}, n, args.steps, args.warmup,
                          per_arm={"exhaustive": (2, 1, n), "torch_brute_force": (1, 1, sub.shape[0])})
            for k in out:
                out[k]["unit"] = "points/s"
            d, e = out["default"], out["exhaustive"]
            spread = max(d["spread"], e["spread"])
            return {"points": int(n), "sort": sort, "exhaustive_same_bytes": same, "torch_max_abs_diff": err, **out,
                    "speedup_over_exhaustive": round(e["ms"] / d["ms"], 3),
                    "speedup_over_torch": round(d["per_s"] / out["torch_brute_force"]["per_s"], 3),
                    "larger_spread": spread, "beats_exhaustive": bool(d["ms"] < e["ms"] * (1.0 - spread))}

        entry["camera_order"] = leg(p)
        shuffled = p[perm].contiguous()
        entry["shuffled"] = leg(shuffled)
        entry["shuffled_sorted"] = leg(shuffled, sort=True)
        entry["uniform"] = leg(uni)
        res["scenes"][str(sid)] = entry
        print(json.dumps({str(sid): entry}), flush=True)
        gs.close()
        hs.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


def torch_brute_crossings(rays, tmin, tmax, v0, v1, v2, chunk=512):
    """What a caller has without GpuScene.crossings: IntersectRayTri's formulas over rays x triangles in float32 torch,
    `chunk` rays at a time, the hits inside (tmin, tmax) summed -> (count, front) int64.  torch fuses and orders the
    sums as it likes, so the counts are NOT the walk's on rays that graze an edge."""
    e1, e2 = v1 - v0, v2 - v0
    cnt = torch.empty(rays.shape[0], dtype=torch.int64, device=rays.device)
    fr = torch.empty_like(cnt)
    for i in range(0, rays.shape[0], chunk):
        o, d = rays[i:i + chunk, None, :3], rays[i:i + chunk, None, 3:]
        p = torch.cross(d.expand(-1, e2.shape[0], -1), e2[None].expand(o.shape[0], -1, -1), dim=2)
        det = (e1[None] * p).sum(2)
        inv = 1.0 / det
        tv = o - v0[None]
        u = (tv * p).sum(2) * inv
        q = torch.cross(tv, e1[None].expand(o.shape[0], -1, -1), dim=2)
        v = (d * q).sum(2) * inv
        t = (e2[None] * q).sum(2) * inv
        hit = (det.abs() >= 1e-8) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t > tmin) & (t < tmax)
        cnt[i:i + chunk] = hit.sum(1)
        fr[i:i + chunk] = (hit & (det > 0)).sum(1)
    return cnt, fr


def crossing_legs(args):
    """--crossings: rt_crossing_rays_device (GpuScene.crossings) into profiles/crossings_bench.json.
      Rays: the 1920x1080x4 camera rays shuffled (PCG64(41)) over the infinite interval, and the ambient-occlusion
      bounce of the ray legs over (1e-4 box diagonals, +inf).  Arms, samples interleaved (measure): crossings, and
      occluded on the same rays and interval -- the floor: that walk stops at its first counted test and this one
      cannot (`ratio` = crossings ms / occluded ms; not a pass condition) -- and a chunked float32 torch brute force
      over all triangles (torch_brute_crossings: what a caller has today; timed over the leg's first TORCH_RAYS rays).
      `implies`: count >= 1 implies occluded on every ray (include/rt_tracer.h).
      Points: the hit points of the 1920x1080x1 primary rays jittered by a normal of 1 % of the box diagonal (seed 47;
      distance_legs' points): inside (three directions per point, one crossings call, the vote in torch) and
      signed_distance beside distance() alone."""
    TORCH_RAYS = 1 << 15
    rtm = load("rtm_this", None)
    res = {"tool": "tools/bench_rays.py --crossings", "frame": [W, H, SPP], "steps": args.steps, "warmup": args.warmup,
           "samples": 5, "build_hash": rtm.library_build_hash(), "device": torch.cuda.get_device_name(0),
           "torch_arm": f"chunked float32 brute force over the first {TORCH_RAYS} rays of a leg; not bit-exact", "scenes": {}}
    st = torch.cuda.current_stream().cuda_stream
    n = W * H * SPP
    for sid in args.scenes:
        hs = rtm.HostScene.load(sid)
        gs = rtm.GpuScene(hs, 0)
        rays = gs.primary_rays(gs.frame(W, H, SPP))
        v, t = hs.mesh()
        pos = torch.from_numpy(np.ascontiguousarray(v[:, :3])).cuda()
        idx = torch.from_numpy(np.ascontiguousarray(t[:, :3]).astype(np.int64)).cuda()
        v0, v1, v2 = pos[idx[:, 0]].contiguous(), pos[idx[:, 1]].contiguous(), pos[idx[:, 2]].contiguous()
        meta = hs.grid()[0]
        e = (meta["aabb_max"] - meta["aabb_min"]).astype(np.float64)
        diag = float(np.sqrt((e * e).sum()))
        torch.cuda.synchronize()
        entry = {"triangles": int(t.shape[0]), "box_diagonal": diag}

        def leg(r, tmin=None, tmax=None):
            tmm = None
            if tmin is not None:
                tmm = torch.empty((r.shape[0], 2), dtype=torch.float32, device=r.device)
                tmm[:, 0], tmm[:, 1] = tmin, tmax
            c = gs.crossings(r, tmm)
            occ = gs.occluded(r, tmm) != 0
            same_sorted = bool(torch.equal(gs.crossings(r, tmm, sort=True).raw, c.raw))
            sub = r[:TORCH_RAYS].contiguous()
            lo, hi = (float("-inf"), float("inf")) if tmin is None else (tmin, tmax)
            bc, bf = torch_brute_crossings(sub, lo, hi, v0, v1, v2)
            m = sub.shape[0]
            out = measure({"crossings": lambda: gs.crossings(r, tmm, stream=st),
                           "occluded": lambda: gs.occluded(r, tmm, stream=st),
                           "torch_brute_force": lambda: torch_brute_crossings(sub, lo, hi, v0, v1, v2)}, r.shape[0],
                          args.steps, args.warmup, per_arm={"torch_brute_force": (1, 1, m)})
            for k in out:
                out[k]["unit"] = "rays/s"
            a, b = out["crossings"], out["occluded"]
            return {"rays": int(r.shape[0]), "counted_rays": int((c.raw[:, 0] > 0).sum()), "occluded": int(occ.sum()),
                    "crossings_total": int(c.raw[:, 0].sum(dtype=torch.int64)), "front_total": int(c.raw[:, 1].sum(dtype=torch.int64)),
                    "max_count": int(c.raw[:, 0].max()), "tmin": tmin,
                    "tmax": None if tmax is None else (tmax if np.isfinite(tmax) else "inf"),
                    "implies": bool((occ | (c.raw[:, 0] == 0)).all()), "sorted_same_bytes": same_sorted,
                    "torch_rays_with_another_count": int((bc != c.raw[:m, 0]).sum()),
                    "torch_rays_with_another_front": int((bf != c.raw[:m, 1]).sum()), **out,
                    "ratio_over_occluded": round(a["ms"] / b["ms"], 3), "larger_spread": max(a["spread"], b["spread"]),
                    "speedup_over_torch": round(a["per_s"] / out["torch_brute_force"]["per_s"], 3)}

        perm = torch.from_numpy(np.random.Generator(np.random.PCG64(41)).permutation(n)).cuda()
        entry["shuffled"] = leg(rays[perm].contiguous())
        tri_n = torch.from_numpy(np.ascontiguousarray(t[:, 3:6]).view(np.float32).copy()).cuda()
        ao = ao_rays(rays, gs.trace_rays(rays).hits, tri_n, float((meta["aabb_max"] - meta["aabb_min"]).max()))
        entry["ao_bounce"] = leg(ao, 1e-4 * diag, float("inf"))
        del ao, rays
        # inside / signed distance: distance_legs' jittered hit points
        r1 = gs.primary_rays(gs.frame(W, H, 1))
        h1 = gs.trace_rays(r1)
        hit = h1.hits[:, 0] != -1
        g = torch.Generator(device="cuda")
        g.manual_seed(47)
        p = r1[hit, :3] + r1[hit, 3:] * h1.t[hit][:, None]
        p = (p + torch.randn(p.shape, generator=g, device="cuda") * (0.01 * float((pos.max(0).values - pos.min(0).values).norm()))).contiguous()
        ins = gs.inside(p)
        sd, pd = gs.signed_distance(p), gs.distance(p)
        out = measure({"distance": lambda: gs.distance(p, stream=st), "inside": lambda: gs.inside(p, stream=st),
                       "signed_distance": lambda: gs.signed_distance(p, stream=st)}, p.shape[0], args.steps, args.warmup)
        for k in out:
            out[k]["unit"] = "points/s"
        entry["points"] = {"points": int(p.shape[0]), "inside_points": int(ins.sum()),
                           "inside_parity_differs": int((gs.inside(p, rule="parity") != ins).sum()),
                           "abs_signed_same_bits": bool(torch.equal(sd.dist.abs().view(torch.int32), pd.dist.view(torch.int32))),
                           **out, "signed_over_distance": round(out["signed_distance"]["ms"] / out["distance"]["ms"], 3)}
        res["scenes"][str(sid)] = entry
        print(json.dumps({str(sid): entry}), flush=True)
        gs.close()
        hs.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


def march_loop(gs, rays, max_steps, min_dist, st, sort=False):
    """What a caller had before rt_march_rays_device: the contract's loop as GpuScene.distance calls with torch float32
    arithmetic between them (one torch operation per rounding: the same bytes), on the rays still marching, until
    every ray is done -> the [n, 4] rt_march_hit words."""
    n = rays.shape[0]
    o, d = rays[:, :3].contiguous(), rays[:, 3:].contiguous()
    t = torch.zeros(n, dtype=torch.float32, device=rays.device)
    out = torch.zeros((n, 4), dtype=torch.int32, device=rays.device)
    out[:, 2] = -1
    idx = torch.arange(n, device=rays.device)
    for s in range(max_steps):
        if idx.numel() == 0:            # (a host read per step: the caller has to know when to stop)
            break
        prod = t[idx, None] * d[idx]
        res = gs.distance((o[idx] + prod).contiguous(), sort=sort, stream=st)
        tn = t[idx] + res.dist
        t[idx] = tn
        h = res.dist < min_dist
        done = idx[h]
        out[done, 0] = tn[h].view(torch.int32)
        out[done, 1] = res.dist[h].view(torch.int32)
        out[done, 2] = res.raw[h, 1]
        out[done, 3] = s + 1
        idx = idx[~h]
    return out


def idle_share(steps, max_steps, count_miss):
    """Share of lane-steps idle in waves of 64 consecutive rays: 1 - sum(lane steps) / (64 x sum(the wave's longest
    lane)), a hit marching its steps and a miss count_miss steps (max_steps: the arm without the early stop, exact;
    1: a lower bound of what a stopped miss marches -- where a miss stopped cannot be read from the output)."""
    s = np.where(steps == 0, count_miss, steps).astype(np.int64)
    lanes = np.concatenate([s, np.zeros((-s.size) % 64, np.int64)]).reshape(-1, 64)
    return round(1.0 - float(s.sum()) / float(lanes.max(1).sum() * 64), 4)


def march_legs(args):
    """--march: rt_march_rays_device (GpuScene.march), max_steps 128, min_dist 1e-3, into profiles/march_bench.json.
    Rays: the 1920x1080x1 camera rays in camera order, shuffled (PCG64(41)), and shuffled with RT_MARCH_SORT.  Arms,
    samples interleaved (measure), one launch per sample:
      fused          the call as it ships;
      distance_loop  march_loop: what a caller had before, the same bytes;
      exhaustive     RT_MARCH_EXHAUSTIVE over the leg's first EXH_RAYS rays (compared per ray);
      <--ab-lib>     the same call from variant builds: the other seed, no early stop.
    Per scene also the RT_ISECT_RAY_MARCH frame of the same camera at spp 1 (render_frame_device between events: the
    flat sweep of all block boxes per step against the hierarchy), and the idle share of lane-steps from `steps`."""
    EXH_RAYS = 1 << 15
    MAX_STEPS, MIN_DIST = 128, 1e-3
    mods = {"this": load("rtm_this", None)}
    for spec in args.ab_lib:
        name, lib = spec.split("=", 1)
        mods[name] = load("rtm_" + name, lib)
    rtm = mods["this"]
    res = {"tool": "tools/bench_rays.py --march", "frame": [W, H, 1], "max_steps": MAX_STEPS, "min_dist": MIN_DIST,
           "launches_per_sample": args.steps, "warmup": args.warmup, "samples": 5, "build_hash": rtm.library_build_hash(),
           "device": torch.cuda.get_device_name(0), "arms": {k: m.library_build_hash() for k, m in mods.items()},
           "exhaustive_arm": f"RT_MARCH_EXHAUSTIVE over the first {EXH_RAYS} rays of a leg; rays/s compared",
           "scenes": {}}
    st = torch.cuda.current_stream().cuda_stream
    for sid in args.scenes:
        hs = {k: m.HostScene.load(sid) for k, m in mods.items()}
        gs = {k: m.GpuScene(hs[k], 0) for k, m in mods.items()}
        g0 = gs["this"]
        rays = g0.primary_rays(g0.frame(W, H, 1))
        torch.cuda.synchronize()
        n = rays.shape[0]
        entry = {"triangles": int(hs["this"].mesh()[1].shape[0]), "rays": int(n)}

        def leg(r, sort=False):
            ref = g0.march(r, MAX_STEPS, MIN_DIST, sort=sort).raw
            sub = r[:EXH_RAYS].contiguous()
            same = {"distance_loop": bool(torch.equal(march_loop(g0, r, MAX_STEPS, MIN_DIST, st, sort), ref)),
                    "exhaustive": bool(torch.equal(g0.march(sub, MAX_STEPS, MIN_DIST, exhaustive=True, sort=sort).raw, ref[:EXH_RAYS]))}
            fns = {"fused": lambda: g0.march(r, MAX_STEPS, MIN_DIST, sort=sort, stream=st),
                   "distance_loop": lambda: march_loop(g0, r, MAX_STEPS, MIN_DIST, st, sort),
                   "exhaustive": lambda: g0.march(sub, MAX_STEPS, MIN_DIST, exhaustive=True, sort=sort, stream=st)}
            for k, g in gs.items():
                if k != "this":
                    fns[k] = lambda g=g: g.march(r, MAX_STEPS, MIN_DIST, sort=sort, stream=st)
                    same[k] = bool(torch.equal(g.march(r, MAX_STEPS, MIN_DIST, sort=sort).raw, ref))
            out = measure(fns, n, args.steps, args.warmup, per_arm={"distance_loop": (1, 1, n), "exhaustive": (1, 1, sub.shape[0])})
            for k in out:
                out[k]["unit"] = "rays/s"
                if k in same:
                    out[k]["same_bytes_as_fused"] = same[k]
            steps = ref[:, 3].cpu().numpy()
            f, lp, ex = out["fused"], out["distance_loop"], out["exhaustive"]
            o = {"rays": int(n), "sort": sort, "hits": int((steps != 0).sum()), "max_hit_steps": int(steps.max()), **out,
                 "speedup_over_distance_loop": round(lp["ms"] / f["ms"], 3),
                 "speedup_over_exhaustive_per_ray": round(f["per_s"] / ex["per_s"], 1),
                 "beats_distance_loop": bool(f["ms"] < lp["ms"] * (1.0 - max(f["spread"], lp["spread"]))),
                 "beats_exhaustive": bool(f["per_s"] * (1.0 - max(f["spread"], ex["spread"])) > ex["per_s"])}
            for k in out:
                if k not in ("fused", "distance_loop", "exhaustive"):
                    o[f"fused_beats_{k}"] = bool(f["ms"] < out[k]["ms"] * (1.0 - max(f["spread"], out[k]["spread"])))
                    o[f"{k}_over_fused"] = round(out[k]["ms"] / f["ms"], 3)
            if not sort:
                o["idle_lane_steps"] = {"misses_at_max_steps": idle_share(steps, MAX_STEPS, MAX_STEPS),
                                        "misses_at_one_step": idle_share(steps, MAX_STEPS, 1)}
            return o

        entry["camera_order"] = leg(rays)
        perm = torch.from_numpy(np.random.Generator(np.random.PCG64(41)).permutation(n)).cuda()
        shuffled = rays[perm].contiguous()
        entry["shuffled"] = leg(shuffled)
        entry["shuffled_sorted"] = leg(shuffled, sort=True)
        fm = g0.frame(W, H, 1, intersector=rtm.RT_ISECT_RAY_MARCH)
        out = torch.empty(W * H, dtype=torch.int32, device="cuda")
        fr = measure({"march_frame": lambda: g0.render_frame_device(fm, out.data_ptr(), st)}, n, args.steps, args.warmup)
        fr["march_frame"]["unit"] = "samples/s"
        entry["frame_ray_march_spp1"] = fr["march_frame"]
        entry["frame_over_fused_camera_order"] = round(fr["march_frame"]["ms"] / entry["camera_order"]["fused"]["ms"], 3)
        res["scenes"][str(sid)] = entry
        print(json.dumps({str(sid): entry}), flush=True)
        for g in gs.values():
            g.close()
        for h in hs.values():
            h.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


def march_frame_legs(args):
    """--march-frame: march_legs' frame leg alone -- the RT_ISECT_RAY_MARCH frame of the scene's camera at 1920x1080x1,
    render_frame_device between events -- from this build and from --parent-lib, samples interleaved (measure)."""
    mods = {"this": load("rtm_this", None)}
    if args.parent_lib:
        mods["parent"] = load("rtm_parent", args.parent_lib)
    res = {"tool": "tools/bench_rays.py --march-frame", "frame": [W, H, 1], "launches_per_sample": args.steps,
           "warmup": args.warmup, "samples": 5, "device": torch.cuda.get_device_name(0),
           "arms": {k: m.library_build_hash() for k, m in mods.items()}, "scenes": {}}
    st = torch.cuda.current_stream().cuda_stream
    for sid in args.scenes:
        hs = {k: m.HostScene.load(sid) for k, m in mods.items()}
        gs = {k: m.GpuScene(hs[k], 0) for k, m in mods.items()}
        outs = {k: torch.empty(W * H, dtype=torch.int32, device="cuda") for k in mods}
        fms = {k: gs[k].frame(W, H, 1, intersector=m.RT_ISECT_RAY_MARCH) for k, m in mods.items()}
        fr = measure({k: (lambda k=k: gs[k].render_frame_device(fms[k], outs[k].data_ptr(), st)) for k in mods},
                     W * H, args.steps, args.warmup)
        torch.cuda.synchronize()
        entry = {"triangles": int(hs["this"].mesh()[1].shape[0]), **fr}
        for k in fr:
            fr[k]["unit"] = "samples/s"
        if "parent" in fr:
            entry["same_frame_as_parent"] = bool(torch.equal(outs["this"], outs["parent"]))
            entry["this_over_parent_ms"] = round(fr["this"]["ms"] / fr["parent"]["ms"], 4)
            entry["tie_within_spread"] = bool(abs(fr["this"]["ms"] - fr["parent"]["ms"]) <=
                                              max(fr["this"]["spread"], fr["parent"]["spread"]) * fr["parent"]["ms"])
        res["scenes"][str(sid)] = entry
        print(json.dumps({str(sid): entry}), flush=True)
        for g in gs.values():
            g.close()
        for h in hs.values():
            h.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's librt_tracer.so (file in the package directory)")
    ap.add_argument("--ab-lib", action="append", default=[], help="NAME=LIB: the ray legs from another build too")
    ap.add_argument("--occlusion", action="store_true", help="the occlusion legs (occlusion_legs) instead of the ray legs")
    ap.add_argument("--ao", action="store_true", help="the AO-frame legs (ao_legs) instead of the ray legs")
    ap.add_argument("--distance", action="store_true", help="the distance-query legs (distance_legs) instead of the ray legs")
    ap.add_argument("--crossings", action="store_true", help="the crossing-query legs (crossing_legs) instead of the ray legs")
    ap.add_argument("--march", action="store_true", help="the march-query legs (march_legs) instead of the ray legs; "
                                                        "--steps / --warmup default to 1 there: a launch is long")
    ap.add_argument("--march-frame", action="store_true", help="the RT_ISECT_RAY_MARCH frame leg alone, this build beside "
                                                              "--parent-lib (march_frame_legs); --out is required")
    ap.add_argument("--out", default=None, help="default: profiles/rays_bench.json (--occlusion: profiles/occlusion_bench.json; "
                                                "--ao: profiles/ao_bench.json; --distance: profiles/distance_bench.json; --march: profiles/march_bench.json; "
                                                "--crossings: profiles/crossings_bench.json)")
    args = ap.parse_args()
    if args.march_frame and args.out is None:
        raise SystemExit("--march-frame needs --out")
    if args.march or args.march_frame:
        args.steps = 1 if args.steps == ap.get_default("steps") else args.steps
        args.warmup = 1 if args.warmup == ap.get_default("warmup") else args.warmup
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "crossings_bench.json" if args.crossings else "march_bench.json" if args.march else "ao_bench.json" if args.ao else "distance_bench.json" if args.distance else
                                "occlusion_bench.json" if args.occlusion else "rays_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_rays.py measures on the GPU; none is visible")
    if args.march_frame:
        return march_frame_legs(args)
    if args.march:
        return march_legs(args)
    if args.crossings:
        return crossing_legs(args)
    if args.distance:
        return distance_legs(args)
    if args.ao:
        return ao_legs(args)
    if args.occlusion:
        return occlusion_legs(args)
    mods = {"this": load("rtm_this", None)}
    for spec in args.ab_lib:
        name, lib = spec.split("=", 1)
        mods[name] = load("rtm_" + name, lib)
    parent = load("rtm_parent", args.parent_lib) if args.parent_lib else None
    rtm = mods["this"]
    res = {"tool": "tools/bench_rays.py", "frame": [W, H, SPP], "steps": args.steps, "warmup": args.warmup,
           "samples": 5, "build_hash": rtm.library_build_hash(), "device": torch.cuda.get_device_name(0),
           "arms": {k: m.library_build_hash() for k, m in mods.items()},
           "parent_build_hash": parent.library_build_hash() if parent else None, "scenes": {}}
    st = torch.cuda.current_stream().cuda_stream
    n = W * H * SPP
    for sid in args.scenes:
        hs = {k: m.HostScene.load(sid) for k, m in mods.items()}
        gs = {k: m.GpuScene(hs[k], 0) for k, m in mods.items()}
        g0 = gs["this"]
        f = g0.frame(W, H, SPP)
        rays = g0.primary_rays(f)
        torch.cuda.synchronize()
        entry = {}

        def ray_leg(r, sort=False):
            fns = {k: (lambda g=g: g.trace_rays(r, stream=st)) for k, g in gs.items()}
            ref = g0.trace_rays(r).hits
            same = {k: bool(torch.equal(g.trace_rays(r).hits, ref)) for k, g in gs.items()}
            if sort:            # (d): this build with RT_RAYS_SORT, the sort's own kernels inside the timed span
                fns["this_sorted"] = lambda: g0.trace_rays(r, sort=True, stream=st)
                same["this_sorted"] = bool(torch.equal(g0.trace_rays(r, sort=True).hits, ref))
            out = measure(fns, r.shape[0], args.steps, args.warmup)
            for k in out:
                out[k]["unit"] = "rays/s"
                out[k]["same_bits_as_this"] = same[k]
            return {"rays": int(r.shape[0]), "hits": int((ref[:, 0] != -1).sum()), **out}

        # (a) camera order, beside the frame
        entry["a_camera_order"] = ray_leg(rays)
        frames = {}
        out = torch.empty(W * H, dtype=torch.int32, device="cuda")
        fr = {"this": (rtm, g0, f)}
        if parent:
            ph = parent.HostScene.load(sid)
            pg = parent.GpuScene(ph, 0)
            fr["parent"] = (parent, pg, pg.frame(W, H, SPP))
        fm = measure({k: (lambda g=g, ff=ff: g.render_frame_device(ff, out.data_ptr(), st)) for k, (_, g, ff) in fr.items()},
                     n, args.steps, max(args.warmup, 40))
        for k in fm:
            fm[k]["unit"] = "samples/s"
        entry["a_render_frame_device"] = fm
        base = fm.get("parent", fm["this"])
        entry["a_ratio_rays_over_frame"] = {"frame_from": "parent" if parent else "this",
                                            "ratio": round(entry["a_camera_order"]["this"]["per_s"] / base["per_s"], 4)}
        # (b) shuffled
        perm = torch.from_numpy(np.random.Generator(np.random.PCG64(41)).permutation(n)).cuda()
        shuffled = rays[perm].contiguous()
        entry["b_shuffled"] = ray_leg(shuffled, sort=True)
        # (c) one ambient-occlusion bounce
        v, t = hs["this"].mesh()
        tri_n = torch.from_numpy(np.ascontiguousarray(t[:, 3:6]).view(np.float32).copy()).cuda()
        meta = hs["this"].grid()[0]
        ext = float((meta["aabb_max"] - meta["aabb_min"]).max())
        ao = ao_rays(rays, g0.trace_rays(rays).hits, tri_n, ext)
        entry["c_ao_bounce"] = ray_leg(ao, sort=True)
        # (d) the ordering pass against the unsorted call: it is kept only if it wins both legs by more than
        # the larger of the two arms' spreads
        d = {}
        for leg in ("b_shuffled", "c_ao_bounce"):
            u, so = entry[leg]["this"], entry[leg]["this_sorted"]
            d[leg] = {"unsorted_ms": u["ms"], "sorted_ms": so["ms"], "speedup": round(u["ms"] / so["ms"], 3),
                      "wins": bool(so["ms"] < u["ms"] * (1.0 - max(u["spread"], so["spread"])))}
        d["also_camera_order"] = ray_leg(rays, sort=True)
        entry["d_sort"] = d
        res["scenes"][str(sid)] = entry
        print(json.dumps({str(sid): entry}), flush=True)
        for g in list(gs.values()) + ([pg] if parent else []):
            g.close()
        for h in list(hs.values()) + ([ph] if parent else []):
            h.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
