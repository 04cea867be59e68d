"""Build-level guard of the lean add chains of the per-lane box runs (csrc/rt_lane_run.h; CPU-only,
needs hipcc).

* The kernels tests/test_build_guard.py, tests/test_fixed_cost_guard.py and tests/test_prologue_guard.py name keep
  0 scratch and their waves per SIMD with both chain forms in them (the lean loops and the guarded fall-back): the
  compiler's 8 and at most 64 VGPRs for the 8-wave group, 8 by the hardware's admission rule
  (floor(800 / (ceil(sgpr / 16) * 16 + 16))) for the bench's own kernels, and the 256-lane fused batch kernels
  their 7 waves at 72 VGPRs or fewer.
* No fused multiply-add is added: rt_lane_run.h holds none (code or comment), and the device IR of rt_kernels.hip
  holds exactly as many llvm.fma calls per grid_intersect walk as box_exit_bound and rcp_nr put there -- the count
  with the lean chains equals the count with the guarded loops alone (-DRT_LANE_CHAIN_UNROLL=0).
* The bench kernel's lean loop is what DESIGN.md §4.39 counts: per block of four trips 16 VALU instructions, one
  s_bcnt1_i32_b64 vote and one s_cbranch_scc1 among at most six scalar-side instructions (s_nop aside), and no
  lane-mask bookkeeping on exec between them.
"""
import os
import re
import subprocess

import pytest

from conftest import PKG_DIR
from hip_remarks import FLAGS, HIPCC, resource_table

SRC = os.path.join(PKG_DIR, "csrc", "rt_kernels.hip")
HEADER = os.path.join(PKG_DIR, "csrc", "rt_lane_run.h")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

EIGHT_WAVES = ("k_render_lanesILi0ELi80398E", "k_render_lanesILi0ELi78350E", "k_render_lanesILi0ELi76298E",
               "k_render_lanesILi0ELi74250E", "k_render_lanesILi0ELi604686E", "k_render_lanesILi0ELi0E",
               "k_render_compact", "k_render_lanes_w64ILi0ELi80398E", "k_render_batch_w64ILi0ELi80398E",
               "k_render_batch_w64ILi0ELi1653262E", "k_render_batch_w64ILi0ELi3750414E",
               "k_render_batchILi0ELi80398E", "k_render_whILj16E", "k_render_whILj4E")
HARDWARE_RULE = ("k_render_lanes_w64ILi0ELi80398E", "k_render_lanesILi0ELi80398E", "k_render_batch_w64ILi0ELi80398E",
                 "k_render_batch_w64_o8ILi0ELi1653262E", "k_render_batch_w64_o8ILi0ELi3750414E")
SEVEN_WAVES = ("k_render_batchILi0ELi1653262E", "k_render_batchILi0ELi3750414E")
BENCH_KERNEL = "k_render_lanes_w64ILi0ELi80398E"
UNROLL = int(re.search(r"^#define RT_LANE_CHAIN_UNROLL (\d+)$", open(HEADER).read(), re.M).group(1))


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    asm = tmp_path_factory.mktemp("lanechain") / "rt_kernels.s"
    table = resource_table(SRC, ["-S", "-o", str(asm)])
    return asm.read_text().splitlines(), table


def test_guarded_kernels_keep_waves_and_scratch(build):
    table = build[1]
    for key in EIGHT_WAVES:
        arm = {n: v for n, v in table.items() if key in n}
        assert arm, key
        for n, (sg, vg, sc, oc, ld) in arm.items():
            assert sc == 0 and oc == 8 and vg <= 64, (n, sg, vg, sc, oc)
    for key in HARDWARE_RULE:
        arm = {n: v for n, v in table.items() if key in n}
        assert arm, key
        for n, (sg, vg, sc, oc, ld) in arm.items():
            assert sc == 0 and min(oc, 800 // (-(-sg // 16) * 16 + 16)) == 8, (n, sg, vg, sc, oc)
    for key in SEVEN_WAVES:
        arm = {n: v for n, v in table.items() if key in n}
        assert arm, key
        for n, (sg, vg, sc, oc, ld) in arm.items():
            assert sc == 0 and oc >= 7 and vg <= 72, (n, sg, vg, sc, oc)
    assert all(sc == 0 for n, (sg, vg, sc, oc, ld) in table.items() if "k_render_" in n)


def test_no_fused_operation_is_added(tmp_path):
    text = open(HEADER).read()
    assert not re.search(r"\bfmaf?\b|__builtin_fma", text)

    def fma_calls(extra, name):
        ll = tmp_path / name
        subprocess.run([HIPCC] + FLAGS + extra + ["-emit-llvm", "-S", "-o", str(ll), SRC], check=True, capture_output=True)
        ir = ll.read_text()
        assert "fmuladd" not in ir
        return len(re.findall(r"call [^\n]*@llvm\.fma\.f32", ir))

    lean, guarded = fma_calls([], "lean.ll"), fma_calls(["-DRT_LANE_CHAIN_UNROLL=0"], "guarded.ll")
    print("llvm.fma.f32 calls:", lean, "with the lean chains,", guarded, "with the guarded loops alone")
    assert lean == guarded and lean > 0


def test_the_bench_kernel_runs_the_lean_loop(build):
    lines = build[0]
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + BENCH_KERNEL + r"\w*:", l)]
    assert len(starts) == 1, starts
    end = next(i for i in range(starts[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = [l.split(";")[0].strip() for l in lines[starts[0] + 1:end]]
    votes = [i for i, l in enumerate(body) if l.startswith("s_bcnt1_i32_b64")]
    # three axes per grid_intersect instance in the kernel, each loop one vote
    assert votes and len(votes) % 3 == 0, len(votes)
    for i in votes:
        lo = max(j for j in range(i) if body[j].endswith(":"))                   # the loop's label
        hi = next(j for j in range(i, len(body)) if body[j].startswith("s_cbranch"))
        loop = [l for l in body[lo + 1:hi + 1] if l]
        valu = [l for l in loop if l.startswith("v_")]
        salu = [l for l in loop if l.startswith("s_")]
        print(len(valu), "VALU", len(salu), "scalar-side:", loop)
        assert body[hi].startswith("s_cbranch_scc1") and body[hi].split()[-1] == body[lo][:-1], loop
        assert not any("exec" in l for l in loop), loop
        assert sum(l.startswith("v_add_f32") for l in loop) == UNROLL, loop        # a block of UNROLL trips
        assert len(valu) <= 4 * UNROLL and len([l for l in salu if not l.startswith("s_nop")]) <= 6, loop
