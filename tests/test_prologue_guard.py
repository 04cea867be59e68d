"""Build-level guard of the lane kernels' prologue (CPU-only, needs hipcc).

The block map of the lane kernels (xcd_band_block) took two runtime u32 divisions per wave, each compiled to a
float-reciprocal sequence (v_cvt_f32_u32, v_rcp_iflag_f32, ..., v_readfirstlane and ~14 dependent scalar
instructions) -- four copies in k_render_lanes_w64<0, 80398>, with and without a heavy-first front.  Both quotients
now come from the host (KParams::xcd_chunk_m, xcd_full), so the ISA of the bench's lane kernels holds no
v_rcp_iflag_f32 at all; and the three kernels keep 8 waves per SIMD by the hardware's admission rule,
floor(800 / (ceil(sgpr / 16) * 16 + 16)), as tests/test_build_guard.py checks it.
"""
import os
import re

import pytest

from conftest import PKG_DIR
from hip_remarks import HIPCC, resource_table

SRC = os.path.join(PKG_DIR, "csrc", "rt_kernels.hip")
KERNELS = ("k_render_lanes_w64ILi0ELi80398E", "k_render_lanesILi0ELi80398E", "k_render_batch_w64ILi0ELi80398E")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    """One compile for both tests: the assembly, and the resource remarks of the same code."""
    asm = tmp_path_factory.mktemp("prologue") / "rt_kernels.s"
    table = resource_table(SRC, ["-S", "-o", str(asm)])
    return asm.read_text().splitlines(), table


def kernel_body(lines, key):
    """The lines between the label of the one kernel whose mangled name holds `key` and its end."""
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + key + r"\w*:", l)]
    assert len(starts) == 1, (key, starts)
    end = next(i for i in range(starts[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[starts[0] + 1:end]
    assert any("s_endpgm" in l for l in body), key
    return body


@pytest.mark.parametrize("key", KERNELS)
def test_no_runtime_division_in_the_lane_kernels(build, key):
    body = kernel_body(build[0], key)
    hits = [l.strip() for l in body if "v_rcp_iflag_f32" in l]
    print(key, len(body), "lines,", len(hits), "v_rcp_iflag_f32")
    assert not hits, (key, hits)


def test_the_three_keep_eight_waves_by_the_hardware_rule(build):
    for key in KERNELS:
        arm = [(n, sg, sc, oc) for n, (sg, vg, sc, oc, ld) in build[1].items() if key in n]
        assert len(arm) == 1, (key, arm)
        n, sg, sc, oc = arm[0]
        print(n, "sgpr", sg, "scratch", sc, "waves", oc)
        assert sc == 0 and min(oc, 800 // (-(-sg // 16) * 16 + 16)) == 8, arm
