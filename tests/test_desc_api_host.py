"""The description-only half of the C ABI (csrc/rt_desc.cpp) under sanitizers, without a GPU:
tools/tables_check.cpp built as a stand-alone program with plain g++ and no HIP include path - that it builds is the proof that
rt_desc.h, rt_desc.cpp and rt_error.h need no HIP - with the address and undefined-behaviour sanitizers, and run once.  It calls
every export into heap buffers of exactly the reported sizes and of one entry less, re-points a held description after its
sources are freed, and runs the host half of rt_scene_update; it ends with a non-zero status on a sanitizer report or a failed
check of its own.  profiles/desc_api/sanitizer_run.txt is a recorded run."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rust_raytracer_amd", "csrc")
SOURCES = [os.path.join(REPO, "tools", "tables_check.cpp")] + [os.path.join(CSRC, f) for f in ("rt_desc.cpp", "rt_tables.cpp", "rt_compile.cpp", "rt_bvh.cpp")]


def test_description_entry_points_under_sanitizers(tmp_path):
    for name in ("rt_desc.h", "rt_desc.cpp", "rt_error.h"):
        for line in open(os.path.join(CSRC, name)):
            assert not (line.lstrip().startswith("#include") and "hip" in line), f"{name}: {line.strip()}"
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("no g++ to build tools/tables_check.cpp with")
    exe = tmp_path / "tables_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + SOURCES
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    recorded = open(os.path.join(REPO, "profiles", "desc_api", "sanitizer_run.txt")).read()
    assert r.stdout + "exit 0\n" == recorded
