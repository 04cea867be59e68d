"""The common harness of the miss skip's device tests (csrc/rt_miss_mask.h, k_miss_mask, process_item; DESIGN.md
§4.32), shared by tests/test_gpu_miss_skip.py, tests/test_gpu_miss_reach.py, tests/test_gpu_miss_sequences.py and
tests/test_miss_reach_cpu.py (the checker's arguments, the oracle's additions, the expected counts).  A plain
module, not a conftest.

A key gets its mask only at its second request, so a frame that is rendered once never runs k_miss_mask or the
flagged branch of process_item.  masked_vs_reference renders a case until its mask is in use for a second frame
and holds the settled frame to a reference that is never the library under test: a golden frame of the
reference's own, or the CPU restatement (conftest.Oracle / synth_scenes.OracleScene, which the CPU suite pins to
those goldens; oracle_frame below takes a caller's sample table through orc_render_smp).  The unskipped arms -- a
scene created with RT_MISS_SKIP=0, and RT_KERNEL_LANES -- are secondary checks, and the device's flagged count
must equal what the CPU checker (tests/miss_mask_check.cpp, which compiles csrc/rt_miss_mask.h itself) flags for the
same scene file, shape, region, camera, field of view, sample table and shard: a mask that silently stayed null
would pass every comparison of pixels.
"""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np

from conftest import ROOT, load_package

rtm = load_package()
SETTLE = 14          # requests until a mask may take a buffer in use (kMissKeep) and more
CHECKER_SRC = os.path.join(ROOT, "tests", "miss_mask_check.cpp")
GATE_DMAX, RCP_MAX_DIR = 1.0001, 8.0          # csrc/rt_record_gate.h kGateDmax, csrc/rt_cam_bound.h kCamRcpMaxDir


def gpu_scene(hs, skip):
    old = os.environ.get("RT_MISS_SKIP")
    os.environ["RT_MISS_SKIP"] = "1" if skip else "0"
    try:
        return rtm.GpuScene(hs, 0)
    finally:
        if old is None:
            del os.environ["RT_MISS_SKIP"]
        else:
            os.environ["RT_MISS_SKIP"] = old


def build_checker(directory, sanitize=False):
    """tests/miss_mask_check.cpp as a stand-alone program under `directory`; sanitize: with the address and
    undefined-behaviour sanitizers where g++ links them (as tests/test_distance_cpu.py builds its checker)."""
    exe = os.path.join(str(directory), "miss_mask_check")
    base = ["g++", "-std=c++17", "-ffp-contract=off", CHECKER_SRC, "-o", exe]
    if sanitize:
        san = base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        if subprocess.run(san, capture_output=True).returncode == 0:
            return exe
    subprocess.run(base + ["-O2"], check=True)
    return exe


def samples_file(directory, name, table):
    """A sample table [spp, 2] as the checker's samples=FILE reads it (raw float32); its path."""
    path = os.path.join(str(directory), name + ".smp")
    np.ascontiguousarray(table, "<f4").tofile(path)
    return path


def case_args(W, H, spp, rect=None, cam=None, fov=None, samples=None, rank=None, nranks=None):
    """The checker's arguments for one case (after the scene file)."""
    args = [W, H, spp]
    if rect is not None or cam is not None:
        x0, y0, x1, y1 = rect or (0, 0, W, H)
        args += [x0, y0, x1 - x0, y1 - y0]
    if cam is not None:
        args += [float(x).hex() for x in np.asarray(cam, np.float32)]
    if fov is not None:
        args.append("fov=" + float(np.float32(fov)).hex())
    if samples is not None:
        args.append("samples=" + samples)
    if nranks is not None:
        args += [f"rank={rank}", f"nranks={nranks}"]
    return [str(a) for a in args]


def cpu_mask(checker, path, W, H, spp, rect=None, cam=None, fov=None, samples=None, rank=None, nranks=None):
    """The CPU checker's counts for a scene file: {"items", "all_miss", "flagged", "flagged_with_hit"}."""
    args = [checker, "scene", path] + case_args(W, H, spp, rect, cam, fov, samples, rank, nranks)
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = json.loads(r.stdout)["mask"]
    assert m["flagged_with_hit"] == 0
    return m


def cpu_masks(checker, path, cases, directory, name="cases"):
    """cpu_mask for a list of case_args(...) of ONE scene file, the file read once (the checker's batch mode)."""
    listing = os.path.join(str(directory), name + ".txt")
    with open(listing, "w") as f:
        f.write("".join(" ".join(c) + "\n" for c in cases))
    r = subprocess.run([checker, "batch", path, listing], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    masks = json.loads(r.stdout)["masks"]
    assert len(masks) == len(cases)
    for m in masks:
        assert m["flagged_with_hit"] == 0, m
    return masks


def cam16(cam):
    return rtm.look_at(*cam) if cam is not None and len(cam) == 2 else cam


def frame(gs, W, H, spp, cam=None, kernel=rtm.RT_KERNEL_AUTO, fov=None, offsets=None, tri_test=rtm.RT_TRI_MOLLER_TRUMBORE):
    f = gs.frame(W, H, spp, kernel=kernel, sample_offsets=offsets, tri_test=tri_test)
    c = cam16(cam)
    if c is not None:
        for k in range(16):
            f.cam[k] = float(c[k])
    if fov is not None:
        f.fov = float(fov)
    return f


def settle(render, gs, reps=SETTLE):
    """render() repeated until the frame's mask is in use for a second frame (or `reps` frames): every repeat gives
    the same result; returns (result, flagged items of the last frame, frames that ran with a mask in use)."""
    first, flagged, used = None, 0, 0
    for _ in range(reps):
        got = render()
        if first is None:
            first = got
        for a, b in zip(first, got):
            assert np.array_equal(a, b)
        flagged = gs.miss_mask()[0]
        used += flagged > 0
        if used >= 2:
            break
    return first, flagged, used


def settled(render, gs):
    """settle() as tests/test_gpu_miss_skip.py takes it: (result, flagged items of the last frame)."""
    first, flagged, _ = settle(render, gs)
    return first, flagged


def cam_dir_bound(cam):
    """csrc/rt_cam_bound.h cam_dir_bound44: the largest column norm of the 3x3 times (1 + 2^-20).  Above GATE_DMAX
    a frame runs without gate records, above RCP_MAX_DIR without kVarFastRcp."""
    m = np.asarray(cam, np.float32).reshape(4, 4)[:3, :3].astype(np.float64)
    return float(np.sqrt((m * m).sum(0)).max() * (1.0 + 1.0 / 1048576.0))


def oracle_scene(oracle, path, grid_res=64):
    """synth_scenes.OracleScene on a scene file, its grid built at grid_res (orc_scene_load_res; 64: orc_scene_load's)."""
    import synth_scenes as ss
    if grid_res == 64:
        return ss.OracleScene(oracle, path)
    osc = ss.OracleScene.__new__(ss.OracleScene)
    osc.L = oracle.L
    osc.L.orc_scene_load_res.restype = ctypes.c_void_p
    osc.L.orc_scene_load_res.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    osc.h = ctypes.c_void_p(osc.L.orc_scene_load_res(path.encode(), grid_res))
    assert osc.h, f"oracle failed to load {path}"
    return osc


_SMP_BOUND = set()


def oracle_frame(oracle, handle, W, H, spp, cam, fov, offsets=None):
    """The CPU restatement's frame [H, W] u32 and hit IDs [W H spp] of scene `handle` (OracleScene.h or
    Oracle.scene(sid)) under a camera, a field of view and -- offsets [spp, 2] -- the caller's sample table
    (orc_render_smp; None: the Hammersley table, where it is orc_render_cam)."""
    L = oracle.L
    if id(L) not in _SMP_BOUND:
        vp = ctypes.c_void_p
        L.orc_render_smp.argtypes = [vp] + [ctypes.c_uint32] * 3 + [vp, ctypes.c_float, vp, vp, vp]
        _SMP_BOUND.add(id(L))
    out, hid = np.zeros(W * H, np.uint32), np.zeros(W * H * spp, np.uint32)
    c = np.ascontiguousarray(cam16(cam), np.float32)
    smp = None if offsets is None else np.ascontiguousarray(offsets, np.float32).reshape(-1)
    assert smp is None or smp.size == 2 * spp
    rc = L.orc_render_smp(handle, W, H, spp, ctypes.c_void_p(c.ctypes.data), float(fov),
                          None if smp is None else ctypes.c_void_p(smp.ctypes.data), ctypes.c_void_p(out.ctypes.data),
                          ctypes.c_void_p(hid.ctypes.data))
    assert rc == 0
    return out.reshape(H, W), hid


def synth_meshes():
    """{name: (tris, grid_res)} of tests/test_gpu_miss_skip.py: a one-cell grid and a 64-cell grid over [-1, 1]^3
    whose box outline crosses work items, tiles and the frame's edge."""
    import camera_matrices as cm
    import synth_scenes as ss
    return {"cell1": (np.concatenate([cm.facing_stack([0.1 * i for i in range(5)]), ss.anchors()]), 1),
            "grid64": (ss.sparse(20261020, n=40), 64)}


def masked_vs_reference(skip, plain, W, H, spp, expected, cpu, cam=None, fov=None, offsets=None, what="", sha256=None):
    """One case on `skip` (a scene created with the skip) and `plain` (created with RT_MISS_SKIP=0):

      * the frame is rendered on `skip` until its mask is in use for a second frame, every repetition byte-equal
        (where the checker flags nothing a mask is computed once, found empty and dropped: three frames -- the key's
        first request, the one that computes the mask, and the one that finds its count zero);
      * the settled frame equals `expected`, the reference's frame [H, W] u32 (None: its SHA-256 is `sha256`, where
        the golden fixtures hold the reference's 1920x1080 frames as hashes);
      * ... and, secondarily, the frame of `plain` and the RT_KERNEL_LANES frame of `skip`, neither with a mask;
      * the flagged count of the last frame equals `cpu`["flagged"], the CPU checker's for the same case (cpu_mask /
        cpu_masks assert flagged_with_hit == 0).  Where the checker flags items, a mask that was never in use for two
        frames fails here: the frame does not count before.

    Returns (frame, flagged)."""
    def fr(gs, kernel=rtm.RT_KERNEL_AUTO):
        return frame(gs, W, H, spp, cam, kernel, fov=fov, offsets=offsets)
    want = int(cpu["flagged"])
    (a,), flagged, used = settle(lambda: [skip.render_frame(fr(skip))], skip, SETTLE if want else 3)
    print(what, (W, H, spp), "flagged", flagged, "frames with a mask", used, "cpu", cpu)
    assert flagged == want, f"{what}: the device flags {flagged} items, the CPU checker {want}"
    assert used >= 2 or want == 0, f"{what}: no mask in use after {SETTLE} frames"
    if expected is not None:
        assert np.array_equal(a, expected), f"{what}: the masked frame differs from the reference"
    else:
        assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == sha256, \
            f"{what}: the masked frame differs from the reference's SHA-256"
    b = plain.render_frame(fr(plain))
    assert plain.miss_mask() == (0, 0)
    c = skip.render_frame(fr(skip, rtm.RT_KERNEL_LANES))
    assert skip.miss_mask()[0] == 0          # the LANES arm takes no mask
    assert np.array_equal(a, b), f"{what}: RT_MISS_SKIP=0"
    assert np.array_equal(a, c), f"{what}: RT_KERNEL_LANES"
    return a, flagged
