"""The ambient-occlusion bake without a GPU: the C ABI is declared and exported, api.RtBakeResult and
api.RtBakeParams have the header's layout, `rtrace --ao` is checked while the command line is read, and the reference the GPU
tests hold the kernel to (tests/bake_ref.py) draws what it says: unit directions in the normal's hemisphere with the cosine
density's mean."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bake_ref
from rust_raytracer_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rt_mi355.h")
RTRACE = os.path.join(REPO, "rust_raytracer_amd", "rtrace")
ENTRY_POINTS = ("rt_bake_visibility", "rt_bake_visibility_device", "rt_bake_visibility_hits_device", "rt_bake_stats")
AO_MESSAGE = "Ambient occlusion must be <samples>[:<max_distance>]"


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    lib = C.CDLL(api.DEVICE_LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert hasattr(C.CDLL(api.HOST_LIB_PATH), "rth_ao")
    for method in ("bake_visibility", "bake_visibility_device", "bake_visibility_hits_device", "bake_stats"):
        assert callable(getattr(api.DeviceScene, method))


def test_result_dtype_layout():
    r = api.RtBakeResult
    assert r.itemsize == 32
    assert r.fields["visibility"][1] == 0 and r.fields["bent"][1] == 8
    assert r.fields["visibility"][0] == np.dtype("<f8") and r.fields["bent"][0].shape == (3,)


def test_layouts_match_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler to check the header with")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(RtBakeParams), '
                   "offsetof(RtBakeParams, samples), offsetof(RtBakeParams, precision), offsetof(RtBakeParams, seed), "
                   "offsetof(RtBakeParams, bias), offsetof(RtBakeParams, max_distance), offsetof(RtBakeParams, _reserved), "
                   "sizeof(RtBakeResult), offsetof(RtBakeResult, visibility), offsetof(RtBakeResult, bent), "
                   "offsetof(RtRayHit, pos), offsetof(RtRayHit, normal), offsetof(RtRayHit, flags)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    m, r, h = api.RtBakeParams, api.RtBakeResult, api.RtRayHit
    assert out == [C.sizeof(m), m.samples.offset, m.precision.offset, m.seed.offset, m.bias.offset, m.max_distance.offset,
                   m._reserved.offset, r.itemsize, r.fields["visibility"][1], r.fields["bent"][1],
                   h.fields["pos"][1], h.fields["normal"][1], h.fields["flags"][1]]
    assert out[:7] == [48, 0, 4, 8, 16, 24, 32]      # the header's own statement of RtBakeParams
    assert out[7:] == [32, 0, 8, 8, 32, 84]          # RtBakeResult; where the hits variant reads pos, normal and flags


def test_default_params():
    p = api.RtBakeParams.defaults()
    assert (p.samples, p.precision, p.seed, p.bias, p.max_distance) == (64, api.RT_PRECISION_F64, 0, 1e-3, float("inf"))
    assert list(p._reserved) == [0] * 4
    assert api.RtBakeParams.defaults(samples=7, seed=3).samples == 7


def test_argument_errors_need_no_device():
    lib = api.load_device_lib()
    buf = (C.c_double * 16)()
    assert lib.rt_bake_visibility(None, 1, buf, buf, None, buf) == api.RT_E_INVALID
    assert b"NULL scene" in lib.rt_last_error()
    assert lib.rt_bake_visibility_device(None, 1, buf, buf, None, buf, None) == api.RT_E_INVALID
    assert lib.rt_bake_visibility_hits_device(None, 1, buf, None, buf, None) == api.RT_E_INVALID
    assert lib.rt_bake_stats(None, None) == api.RT_E_INVALID


@pytest.mark.parametrize("flag, want", [("--ao=64", (64, float("inf"))), ("--ao=1", (1, float("inf"))), ("--ao=4096:2.5", (4096, 2.5)),
                                        ("--ao=256:1e3", (256, 1000.0))])
def test_ao_flag_accepted(flag, want):
    assert api.HostScene(["scenes/cornell", "-w=16", "-s=4", flag]).ao == want
    assert api.HostScene(["scenes/cornell", "-w=16", "-s=4"]).ao == (0, float("inf"))


@pytest.mark.parametrize("flags", [["--ao=0"], ["--ao=5000"], ["--ao=64:-1"], ["--ao=x"], ["--ao=64:"], ["--ao=64:0"], ["--ao=64:nan"],
                                   ["--ao=-3"], ["--ao=6.5"]])
def test_ao_flag_refused(flags):
    with pytest.raises(api.RtError) as e:
        api.HostScene(["scenes/cornell", "-w=16", "-s=4"] + flags)
    assert AO_MESSAGE in str(e.value)


@pytest.mark.parametrize("flags, message", [
    (["--ao=0"], AO_MESSAGE), (["--ao=5000"], AO_MESSAGE), (["--ao=64:-1"], AO_MESSAGE), (["--ao=x"], AO_MESSAGE),
    (["--ao=64", "--gpus=2"], "cannot be combined with --gpus > 1"),
    (["--ao=64", "--progressive=2"], "cannot be combined with --gpus > 1, --progressive"),
    (["--ao=64", "--pick=1,1"], "--pick"),
])
def test_rtrace_rejects_bad_ao_flags_before_touching_a_device(tmp_path, flags, message):
    r = subprocess.run([RTRACE, os.path.join(REPO, "scenes", "cornell"), "-w=16", "-s=4"] + flags, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert message in r.stderr
    assert "Rendering" not in r.stdout
    assert not (tmp_path / "out_ao.png").exists() and not (tmp_path / "out.png").exists()


# ---- the reference itself ----
NORMALS = [(0.0, 1.0, 0.0), (0.0, 0.0, -2.5), (0.95, 0.1, -0.2), (-1.0, 2.0, 3.0)]   # both branches of onb_from_vec (|w.x| > 0.9), not unit length


@pytest.mark.parametrize("normal", NORMALS)
def test_reference_directions(normal):
    n = np.array(normal)
    unit = n / np.linalg.norm(n)
    d = np.array([bake_ref.direction(bake_ref.SEED, 5, s, n) for s in range(4096)])
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 1e-15
    assert (d @ unit >= 0.0).all()
    # a cosine-weighted direction has mean (2/3) n: E[z] = E[sqrt(1 - r2)] = 2/3, E[x] = E[y] = 0; the standard error of a
    # component's mean over 4 096 samples is below 0.5 / 64 = 0.008
    assert np.abs(d.mean(axis=0) - (2.0 / 3.0) * unit).max() <= 0.05
    # streams differ by point and by seed
    assert not np.array_equal(d[0], bake_ref.direction(bake_ref.SEED, 6, 0, n))
    assert not np.array_equal(d[0], bake_ref.direction(bake_ref.SEED + 1, 5, 0, n))


def test_reference_bake_of_an_open_point_and_a_covered_one():
    """cornell: a point on the floor under the open room sees far within a short distance and nothing beyond the room."""
    c = bake_ref.cases("cornell")
    surf = c.cam_hits[c.cam_hits["klass"] == bake_ref.SURFACE]
    p, n = surf["pos"][:1], surf["normal"][:1]
    count, vis, bent = bake_ref.bake(c.hs.desc, p, n, 32, max_distance=1e-2)
    assert count[0] == 32 and vis[0] == 1.0 and np.linalg.norm(bent[0]) <= 1.0
    assert np.abs(bent[0] - np.mean([bake_ref.direction(bake_ref.SEED, 0, s, n[0]) for s in range(32)], axis=0)).max() <= 1e-15
    count, vis, bent = bake_ref.bake(c.hs.desc, p, n, 32, max_distance=float("inf"))
    assert count[0] < 32
