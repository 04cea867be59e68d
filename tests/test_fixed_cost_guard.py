"""Build-level guards of the per-wave fixed-cost changes (CPU-only, needs hipcc and g++).

* csrc/rt_setup_div.h: explicit FMAs appear only inside the division helper setup_div (four of them), and the
  header is hashed into the library's build hash at the same position in csrc/Makefile and in the package's
  kernel_source_hash().
* The render kernels tests/test_build_guard.py names keep 0 scratch, the compiler's 8 waves per SIMD and at
  most 64 VGPRs with the tile origin carried across the walk in a VGPR (process_item); the bench's own kernels keep 8
  waves per SIMD by the hardware's admission rule (floor(800 / (ceil(sgpr / 16) * 16 + 16))).
* process_item's division-free tile coordinates (udiv_by_magic, shard_tile_xy_m in csrc/rt_kparams.h) equal
  the divisions they replace: tests/shard_magic_check.cpp, every divisor up to 4096 tiles across and four
  million random pairs over the whole 32-bit range, and the shard deal of ranks 1 to 9.
"""
import json
import os
import re
import subprocess

import pytest

from conftest import PKG_DIR, ROOT, load_package
from hip_remarks import HIPCC, makefile_words, needs_hipcc, resource_table

HEADER = os.path.join(PKG_DIR, "csrc", "rt_setup_div.h")
SRC = os.path.join(PKG_DIR, "csrc", "rt_kernels.hip")
ROCM_INC = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "include")

# tests/test_build_guard.py's kernels: its 8-wave group, and the group it holds to the hardware rule
EIGHT_WAVES = ("k_render_lanesILi0ELi80398E", "k_render_lanesILi0ELi78350E", "k_render_lanesILi0ELi76298E",
               "k_render_lanesILi0ELi74250E", "k_render_lanesILi0ELi604686E", "k_render_lanesILi0ELi0E",
               "k_render_compact", "k_render_lanes_w64ILi0ELi80398E", "k_render_batch_w64ILi0ELi80398E",
               "k_render_batch_w64ILi0ELi1653262E", "k_render_batch_w64ILi0ELi3750414E",
               "k_render_batchILi0ELi80398E", "k_render_whILj16E", "k_render_whILj4E")
HARDWARE_RULE = ("k_render_lanes_w64ILi0ELi80398E", "k_render_batch_w64ILi0ELi80398E",
                 "k_render_batch_w64_o8ILi0ELi1653262E", "k_render_batch_w64_o8ILi0ELi3750414E")


def test_explicit_fmas_only_inside_the_division_helper():
    text = open(HEADER).read().splitlines()
    code = [(i, l.split("//")[0]) for i, l in enumerate(text)]
    fma = [i for i, l in code if re.search(r"\bfmaf?\b|__builtin_fma", l)]
    assert len(fma) == 4 and all("__builtin_fmaf(" in code[i][1] for i in fma), [text[i] for i in fma]
    start = next(i for i, l in code if re.search(r"\bfloat setup_div\(float n, float d, float r\)", l))
    end = next(i for i, l in code if i > start and l.startswith("}"))
    assert all(start < i < end for i in fma), [text[i] for i in fma]
    # no lower-case word for it in the comments either (tests/test_build_guard.py counts such lines in the
    # files it guards; the same habit here keeps a moved line from tripping it)
    assert not [l for i, l in enumerate(text) if i not in fma and re.search(r"\bfmaf?\b|__builtin_fma", l)]


def test_header_is_hashed_at_the_same_position():
    # (both sides apply one rule to the directory, byte-sorted names: the header's neighbour is the name that sorts
    # before it)
    hashed = makefile_words("print-hashed")
    names = [os.path.basename(n) for n in load_package().kernel_sources()]
    mk_names = [os.path.basename(n) for n in hashed]
    assert "rt_setup_div.h" in mk_names and "rt_setup_div.h" in names
    assert mk_names == names
    assert mk_names.index("rt_setup_div.h") == names.index("rt_setup_div.h")
    assert mk_names[mk_names.index("rt_setup_div.h") - 1] == names[names.index("rt_setup_div.h") - 1] == "rt_scene.h"


@needs_hipcc
def test_guarded_kernels_keep_their_registers(tmp_path):
    table = {n: (sg, sc, vg, oc) for n, (sg, vg, sc, oc, ld) in resource_table(SRC, ["-c", "-o", str(tmp_path / "rt.o")]).items()}
    for key in EIGHT_WAVES:
        arm = {n: v for n, v in table.items() if key in n}
        assert arm, key
        for n, (sg, sc, vg, oc) in arm.items():
            print(n, "sgpr", sg, "vgpr", vg, "scratch", sc, "waves", oc)
            assert sc == 0 and oc == 8 and vg <= 64, (n, sg, sc, vg, oc)
    for key in HARDWARE_RULE:
        arm = {n: v for n, v in table.items() if key in n}
        assert arm, key
        for n, (sg, sc, vg, oc) in arm.items():
            assert sc == 0 and min(oc, 800 // (-(-sg // 16) * 16 + 16)) == 8 and vg <= 64, (n, sg, sc, vg, oc)


@pytest.mark.skipif(not os.path.isdir(ROCM_INC), reason="HIP headers not available")
def test_division_free_tile_coordinates(tmp_path):
    exe = str(tmp_path / "shard_magic_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INC,
                    os.path.join(ROOT, "tests", "shard_magic_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout)
    print(rep)
    assert rep["div_cases"] > 4_000_000 and rep["div_mismatches"] == 0, rep
    assert rep["deal_cases"] > 1_000_000 and rep["deal_mismatches"] == 0, rep
