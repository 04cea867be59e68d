"""The lean add chains of AUTO's per-lane box runs (csrc/rt_lane_run.h) on the CPU: the header's
own functions, compiled with g++ over 64-lane value types, against the three guarded `while` loops lane by lane --
every lane's (c0, c1, c2) and the bits of its three crossing times.  tests/lane_chain_check.cpp is the checker.

* every run of every 16th tile of scenes 1, 4, 5, 8 at 1920x1080x4, the 64 slots of a work item walked in lock-step
  through the approach phase as the wave walks them: zero mismatches, and no wave fails the vote (scene 5's camera
  stands in a non-empty cell, so its waves go straight to lock-step and take no per-lane run: its count is 0);
* seeded families of 10^6 waves each: zero mismatches; the families built to fail the vote fail it in every wave,
  the one-lane family by a single lane.
"""
import json
import os
import subprocess

import pytest

from conftest import ROOT

_EXE = {}
FAMILIES = ("plain", "still", "tiny", "dt0", "stuck", "naninf", "fields", "scales", "onefail")
MUST_FAIL_THE_VOTE = ("naninf", "onefail")


def _checker(tmp_path_factory):
    if "exe" not in _EXE:
        exe = str(tmp_path_factory.mktemp("lanechain") / "lane_chain_check")
        subprocess.run(["g++", "-O2", "-std=c++11", "-pthread", "-ffp-contract=off", "-I", os.path.join(ROOT, "oracle"),
                        os.path.join(ROOT, "tests", "lane_chain_check.cpp"), "-o", exe], check=True)
        _EXE["exe"] = exe
    return _EXE["exe"]


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    print(out)
    assert out["mismatches"] == 0 and out["waves"] > 0, out
    return out


@pytest.mark.parametrize("sid", [1, 4, 5, 8])
def test_lean_chains_on_bench_frames(tmp_path_factory, sid):
    out = _run(_checker(tmp_path_factory), "scene", os.path.join(ROOT, "data", "scenes", f"scene{sid}.rtscene"),
               1920, 1080, 4, 16)
    assert out["vote_failed"] == 0, out
    assert out["waves"] == 120 * 68 // 16 * 16, out      # every 16th of 120 x 68 tiles, 16 work items each
    if sid != 5:
        assert out["runs"] > 1000 and out["lanes"] > 64 * 1000, out
        # whole blocks: the lean loop never runs fewer trips than the guarded loop's longest lane
        assert out["guarded_trips_per_wave"] <= out["lean_trips_per_wave"], out


@pytest.mark.parametrize("family", FAMILIES)
def test_lean_chains_on_seeded_families(tmp_path_factory, family):
    out = _run(_checker(tmp_path_factory), "family", family, 1000000, 12)
    assert out["waves"] == out["runs"] == 1000000, out
    if family in MUST_FAIL_THE_VOTE:
        assert out["vote_failed"] == out["waves"] and out["lean_trips_per_wave"] == 0, out
        # lanes whose bounds hold a NaN: exactly the one built to in `onefail`, at least one a wave in `naninf`
        assert out["unproven_lanes"] == out["waves"] if family == "onefail" else out["unproven_lanes"] >= out["waves"], out
    else:
        # every value of these families keeps the bounds' arithmetic finite (the largest, `tiny`'s steps of ~1.6e28
        # times a field of 1,023, stays below 2e31), so no wave may fail the vote: all of them take the lean chains
        assert out["vote_failed"] == 0 and out["unproven_lanes"] == 0, out
        assert out["lean_trips_per_wave"] >= out["guarded_trips_per_wave"] > 0, out
    if family == "fields":
        assert out["max_trips_in_a_run"] >= 1023, out     # a chain that runs a whole field


def test_subnormal_components_fail_the_vote():
    """The caller rays of tests/test_gpu_lane_chains.py that are meant to reach the guarded fall-back on the device: a
    direction component of 1e-40 or 1e-44 makes the step cw / d exceed 1e38 (or infinite), so any field of 2 or more
    takes f dt + x out of f32 and box_exit_bound (restated here in f32) is a NaN; a component of 1e-30 does not."""
    import numpy as np
    cw = np.float32(2.0 / 64.0)

    def bound(x, dt, f):
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.float32(np.float64(f) * np.float64(dt) + np.float64(x))        # one rounding, as the fused form
            k = np.float32(f + 2) * np.float32(2.0 ** -23)
            return e - np.float32(np.float64(abs(x)) * np.float64(k) + np.float64(np.abs(e) * k))

    with np.errstate(over="ignore", divide="ignore"):
        for d in np.float32([1e-40, 1e-44]):
            for f in (2, 8, 1023):
                assert np.isnan(bound(np.float32(1.0), cw / d, f)), (d, f)
        for f in (0, 8, 1023):
            assert np.isfinite(bound(np.float32(1.0), cw / np.float32(1e-30), f)), f
