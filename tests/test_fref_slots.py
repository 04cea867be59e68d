"""The per-origin record buffer policy (csrc/rt_fref_slots.h) on the CPU: which of a
scene's two buffers a frame reads, when one is recomputed and when a launch may overlap the one before it.
tests/fref_slot_check.cpp compiles the header librt_tracer.so runs and enumerates EVERY sequence of 4
launches on one scene over 4 camera origins -- single frames, batches of 2 frames at 1 or 2 origins,
batches of 3 with a repeat, each ordered or asking to overlap (112 launch kinds, 112^4 sequences: the state
is two buffers and a 2-bit mask, so depth 4 takes every transition out of every reachable state).  Against
its own bookkeeping of what each buffer holds and which launches may still run:

  * an ordered launch of at most 2 distinct origins always gets a buffer for every frame;
  * no recompute targets a buffer that the possibly-running previous launch reads, nor one that an
    earlier frame of the same launch reads;
  * the buffer handed to a frame holds the frame's origin when the launch is issued and still does after
    the launch's remaining frames are placed;
  * a granted overlap needs no wait that order_overlap does not give.

With the rule before this header (an ordered launch kept the last launch's buffers busy) the same walk
ends 9,501,696 sequences in "no free per-origin record buffer", the shortest "ordered[A] ordered[B,C]"."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

DEPTH, ORIGINS = 4, 4
KINDS = 2 * (ORIGINS + ORIGINS * ORIGINS + 3 * ORIGINS * (ORIGINS - 1))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frefslots") / "fref_slot_check")
    subprocess.run(["g++", "-O2", "-std=c++11", "-pthread", os.path.join(ROOT, "tests", "fref_slot_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe, str(DEPTH), str(ORIGINS)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_every_sequence_was_walked(report):
    """No sequence ends early (a launch without a buffer would end it), so the walk is the full tree."""
    assert (report["depth"], report["origins"], report["launch_kinds"]) == (DEPTH, ORIGINS, KINDS), report
    assert KINDS == 112
    assert report["sequences"] == KINDS ** DEPTH, report
    assert report["launches"] == sum(KINDS ** d for d in range(1, DEPTH + 1)), report
    # the walk does reach the cases the invariants are about
    assert report["overlaps_granted"] > 0 and report["recomputes"] > report["launches"] // 2, report


def test_no_violation(report):
    assert report["violations"] == 0 and not any(report["by_kind"].values()), report
    assert report["shortest_violating_sequence"] == ""
    assert set(report["by_kind"]) == {
        "ordered_launch_without_slot", "overlapped_launch_without_slot", "recompute_of_running_launchs_buffer",
        "recompute_of_same_launchs_buffer", "wrong_origin_at_issue", "wrong_origin_at_end",
        "overlap_needs_missing_wait"}
