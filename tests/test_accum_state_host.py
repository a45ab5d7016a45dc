"""The host arithmetic of the progressive accumulator (csrc/rt_accum_state.h) under sanitizers, without a
GPU: tools/accum_state_check.cpp built as a stand-alone program with plain g++ and no HIP include path - that it builds is the
proof that the header needs no HIP - with the address and undefined-behaviour sanitizers, and run once.  It checks state blobs
in heap buffers of exactly their length (round trip, every wrong length, single and paired corruptions of the header and the
adaptive parameter block, the per-pixel replica-count rule), the segment schedule of an adaptive render against brute force,
the parameter checks of rt_accum_set_adaptive and the noise formula; it ends with a non-zero status on a sanitizer report or a
failed check of its own.  The decision points it prints are compared with adaptive_ref.decision_points, which was written
independently.  profiles/accum_split/sanitizer_run.txt is a recorded run."""
import os
import re
import shutil
import subprocess

import pytest

import adaptive_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rust_raytracer_amd", "csrc")


def test_accumulator_host_arithmetic_under_sanitizers(tmp_path):
    for name in ("rt_accum_state.h", "rt_tables.h", "rt_error.h"):
        for line in open(os.path.join(CSRC, name)):
            assert not (line.lstrip().startswith("#include") and "hip" in line), f"{name}: {line.strip()}"
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("no g++ to build tools/accum_state_check.cpp with")
    exe = tmp_path / "accum_state_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
           os.path.join(REPO, "tools", "accum_state_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    shown = re.findall(r"^decision points T=(\d+) min_replicas=(\d+) check_interval=(\d+):(.*)$", r.stdout, flags=re.M)
    assert [tuple(map(int, s[:3])) for s in shown] == [(6, 2, 2), (12, 3, 4), (4, 4, 1)]
    for T, mn, iv, points in shown:
        assert [int(x) for x in points.split()] == adaptive_ref.decision_points(int(T), int(mn), int(iv))
    recorded = open(os.path.join(REPO, "profiles", "accum_split", "sanitizer_run.txt")).read()
    assert r.stdout + "exit 0\n" == recorded
