"""The gated wave-uniform record loop (test_cell in rt_walk.h, csrc/rt_record_gate.h) on
single-cell scenes that sit on its edges.

A list of kGateMinList (8) records or more is walked over the records' 32-byte gate records, a pair per
trip and one wave vote per pair; only a record some lane's gate does not reject is loaded and tested.  The
loop must test the same (ray, record) pairs that can change a lane, in the same order: every frame is
byte-equal to RT_KERNEL_LANES' and to the frame of a scene created with RT_REC_GATE=0 (no gate pointer,
every list takes the ungated loop), and every product record is bit-equal to the plain walk's
(check_against_plain_walk of test_gpu_uniform_lists.py).

List lengths: 7 (below the threshold), 8, 9, 10, 15, 16, 17, 33 -- every tail of the four-record trip (0 to 3
records: a lone record, a pair, a pair and a lone record), one trip and several.  64x64x4 frames of a few
triangles: every case takes well under a second.
"""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from test_gpu_uniform_lists import (AT, EYE, H, SPP, W, OFFSETS, Scene, centre_record, check_against_plain_walk,
                                    facing_stack, rtm)

LENGTHS = [7, 8, 9, 10, 15, 16, 17, 33]


@contextmanager
def gate_env(value):
    """RT_REC_GATE as rt_scene_create reads it (once, at creation)."""
    old = os.environ.get("RT_REC_GATE")
    if value is None:
        os.environ.pop("RT_REC_GATE", None)
    else:
        os.environ["RT_REC_GATE"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("RT_REC_GATE", None)
        else:
            os.environ["RT_REC_GATE"] = old


def side_triangle(i, z):
    """A triangle off to one side of everything the 64x64 frame sees (|x| < 1.7 on z >= 0 from z = 4), with
    e1 along x: u = (x - v0.x) / |e1| lies outside [0, 1] for every ray (left ones above 1, right ones below
    0), so every lane's first half -- and the gate -- rejects it."""
    x0 = 5.0 + 0.25 * (i % 4) if i % 2 else -7.0 - 0.25 * (i % 3)
    return [[x0, -1.0, z], [x0 + 1.0, -1.0 + 0.01 * (i % 5), z], [x0 + 0.1, 1.0, z]]


def check_both_arms(tris, eyes=(EYE,), at=AT):
    """Every view: AUTO against the plain walk (gated scene), and the gated scene's frame against the frame
    of a scene created with RT_REC_GATE=0.  Returns the gated scene's records of the last view."""
    with gate_env(None):
        on = Scene(tris, eyes[0], at, grid_res=1)
    with gate_env("0"):
        off = Scene(tris, eyes[0], at, grid_res=1)
    try:
        assert on.hs.grid()[0]["dims"] == [1, 1, 1]
        rec = None
        for eye in eyes:
            on.look(eye, at)
            off.look(eye, at)
            rec = check_against_plain_walk(on)
            f_on = on.gs.render_frame(on.gs.frame(W, H, SPP, sample_offsets=OFFSETS))
            f_off = off.gs.render_frame(off.gs.frame(W, H, SPP, sample_offsets=OFFSETS))
            assert f_on.tobytes() == f_off.tobytes(), f"{(f_on != f_off).sum()} pixels differ from RT_REC_GATE=0"
        return rec
    finally:
        on.close()
        off.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nt", LENGTHS)
@pytest.mark.parametrize("nearest", ["last", "first"])
def test_every_record_passes(nt, nearest):
    """Every triangle faces the camera and covers the frame's middle: every gate passes, every record is
    loaded on demand and tested; the nearest is the last or the first of the list."""
    zs = [0.05 * i for i in range(nt)]
    if nearest == "first":
        zs = zs[::-1]
    rec = check_both_arms(facing_stack(zs))
    c = centre_record(rec)
    assert c[0] == 1 and c[1] == (nt - 1 if nearest == "last" else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("nt", LENGTHS)
@pytest.mark.parametrize("where", ["first", "second", "middle", "middle+1", "last"])
def test_one_hit_among_rejected_records(nt, where):
    """All but one triangle lie off to the side (the gate rejects them for every lane); the one that is hit
    sits at the first, the second (the second record of the first pair), a middle (both parities: first and
    second record of a pair) or the last list position (the lone record of an odd tail, or a pair's second)."""
    pos = {"first": 0, "second": 1, "middle": nt // 2, "middle+1": nt // 2 + 1, "last": nt - 1}[where]
    tris = [side_triangle(i, 0.03 * i) for i in range(nt)]
    tris[pos] = facing_stack([0.5])[0]
    rec = check_both_arms(tris)
    hits = rec[rec[:, 0] == 1]
    assert len(hits) and (hits[:, 1] == pos).all()
    c = centre_record(rec)
    assert c[0] == 1 and c[1] == pos


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [8, 10, 17])
def test_two_hits_in_one_pair_keep_list_order(nt):
    """Both records of a pair pass and both are hit at the same t (the same triangle twice): record a is
    handled completely before record b, so the strict '<' keeps the first."""
    for first in (2, 3):            # a pair's (a, b), and b of one pair with a of the next
        tris = [side_triangle(i, 0.03 * i) for i in range(nt)]
        tris[first] = facing_stack([0.5])[0]
        tris[first + 1] = [list(p) for p in tris[first]]
        rec = check_both_arms(tris)
        hits = rec[rec[:, 0] == 1]
        assert len(hits) and (hits[:, 1] == first).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [8, 17])
def test_triangles_nearly_edge_on_to_the_camera_axis(nt):
    """Triangles whose plane holds the camera axis to within 1e-7 (tilted either way, and exactly edge-on):
    det is at the 1e-8 threshold for the rays around the axis, where the gate must not reject a lane the
    first half passes.  A facing triangle behind them takes the hits that get through."""
    tris = []
    for i in range(nt - 1):
        tilt = (i - (nt - 1) // 2) * 2.5e-8           # within +-1e-7, 0 included
        x = 0.01 * (i % 3 - 1)
        tris.append([[x, -1.0, 0.5], [x + tilt, 1.0, 0.6], [x - tilt, 0.1 * (i % 4), 2.5]])
    tris.insert(nt // 2, facing_stack([0.0])[0])
    rec = check_both_arms(tris)
    assert (rec[:, 0] == 1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [9, 16])
def test_camera_moved_twice_recomputes_both_gate_buffers(nt):
    """Origins A, B, C, A: k_origin_pre fills both gate arrays again (the scene's records only: the pad stays
    zero), off-axis origins change which side triangles the gate can reject."""
    tris = [side_triangle(i, 0.03 * i) for i in range(nt)]
    tris[nt // 2] = facing_stack([0.5])[0]
    tris[1] = facing_stack([0.2])[0]
    check_both_arms(tris, eyes=(EYE, (0.7, -0.4, 3.5), (-1.1, 0.6, 5.0), EYE))


@pytest.mark.gpu
def test_device_bytes_counts_the_gate_arrays():
    sc = Scene(facing_stack([0.0, 0.1, 0.2]), EYE, AT, grid_res=1)
    try:
        nrefs = sc.hs.stats["num_refs"]
        pad = 2 * (256 // 64)
        assert sc.gs.device_bytes() >= 48 * nrefs + 2 * rtm.fref_buffer_bytes(nrefs) + 2 * 32 * (nrefs + pad)
    finally:
        sc.close()
