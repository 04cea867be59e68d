"""The XCD-band block map without runtime divisions (CPU-only, needs g++ and the HIP headers).

csrc/rt_kparams.h's xcd_band_block takes i / chunk and i % chunk through udiv_by_magic and the number of blocks in
whole rounds of 8 turns from the host (xcd_band_full).  tests/block_map_check.cpp compiles that header with g++ and
compares it with the formula the kernels used before, for every block of every launch of 1 to 3,000 blocks at twelve
turn sizes and of 20,000 random launches (nb < 2^22, chunk < 2^16), checks that each map is a bijection on [0, nb)
and that the host's `full` is nb / (8 chunk) * (8 chunk).

The random launches are not uniform: 63 of 64 draw nb below 2^14 (every 64th over the whole range below 2^22), so
that all blocks of 20,000 launches can be walked in seconds, and every other one draws chunk from [1, nb / 8], so that
nearly half of them have whole rounds to remap (8 chunk <= nb; an unweighted chunk < 2^16 mostly leaves `full` 0 and
the map the identity).  The twelve listed turn sizes carry the cases a launch can have.
"""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ROCM_INC = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "include")


@pytest.mark.skipif(not os.path.isdir(ROCM_INC) or not shutil.which("g++"), reason="g++ or the HIP headers not available")
def test_block_map_equals_the_divisions_it_replaced(tmp_path):
    exe = str(tmp_path / "block_map_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INC,
                    os.path.join(ROOT, "tests", "block_map_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout)
    print(rep)
    assert rep["listed_launches"] == 12 * 3000 and rep["random_launches"] == 20000, rep
    assert rep["cases"] > 12 * 3000 * 3001 // 2, rep
    assert rep["random_with_whole_rounds"] >= 9000, rep
    assert rep["mismatches"] == 0 and rep["full_mismatches"] == 0 and rep["not_bijective"] == 0, rep
