"""What librt_tracer.so is built from is said once, in csrc/Makefile (CPU-only, needs make and no
built artefact).

* The objects are the *.hip files present: a new translation unit is compiled and linked without being listed.
* The hashed set is a rule, not a list -- every *.hip and *.h of csrc/ in byte-sorted name order, then the Makefile, then
  include/rt_tracer.h -- and the Makefile and the package's kernel_sources() both apply it: name for name, in order.
* The package Makefile always asks csrc/Makefile, which knows the real dependencies: a library newer than every
  source still reaches the csrc make (which then finds nothing to do, or what the depfiles say).

On the commit before this file, all three fail: csrc/Makefile has no print-objs / print-hashed target (its lists were
written out by hand), the package has KERNEL_SOURCES in its own hand-written order, and the package Makefile's
prerequisite list -- which names neither rt_crossings.hip nor rt_cam_bound.h -- makes `make -n` print nothing for a
library newer than the files it lists.
"""
import os
import shutil
import subprocess

from conftest import PKG_DIR, ROOT, load_package
from hip_remarks import makefile_words

CSRC = os.path.join(PKG_DIR, "csrc")


def _present(*suffixes):
    return sorted(n for n in os.listdir(CSRC) if n.endswith(suffixes) and not n.startswith("."))


def test_objects_are_the_hip_files_present():
    hips = _present(".hip")
    assert len(hips) >= 12 and "rt_crossings.hip" in hips, hips
    assert makefile_words("print-objs") == [n[:-len(".hip")] + ".o" for n in hips]


def test_hashed_set_is_one_rule_on_both_sides():
    rule = _present(".hip", ".h") + ["Makefile", "../../include/rt_tracer.h"]
    hashed = makefile_words("print-hashed")
    assert hashed == rule
    assert "rt_cam_bound.h" in hashed and "rt_crossings.hip" in hashed and "rt_setup_div.h" in hashed
    mine = load_package().kernel_sources()
    real = [os.path.realpath(os.path.join(CSRC, n)) for n in hashed]
    assert [os.path.realpath(os.path.join(PKG_DIR, n)) for n in mine] == real
    assert all(os.path.isfile(p) for p in real)


def test_package_make_asks_csrc_even_when_the_library_is_newest(tmp_path):
    # a copy of the sources alone, with a library file newer than all of them
    pkg = tmp_path / "repo" / os.path.basename(PKG_DIR)
    shutil.copytree(PKG_DIR, pkg, ignore=shutil.ignore_patterns("*.o", "*.d", "*.so", "*.s", "__pycache__"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "repo" / "include")
    old = os.path.getmtime(pkg / "Makefile") - 3600.0
    for d, _, files in os.walk(tmp_path / "repo"):
        for n in files:
            os.utime(os.path.join(d, n), (old, old))
    (pkg / "librt_tracer.so").write_bytes(b"")
    r = subprocess.run(["make", "-n", "-C", str(pkg), "librt_tracer.so"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    assert "-C csrc" in r.stdout, r.stdout
    # ... and the csrc make it reaches would compile every unit of this object-less copy, rt_crossings among them
    assert "rt_crossings.hip" in r.stdout, r.stdout
