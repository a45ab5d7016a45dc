"""The irradiance bake without a GPU: the C ABI is declared and exported, the hit-record variant reads the
header's offsets, `rtrace --irradiance` is checked while the command line is read, the reference the GPU tests hold the
kernels to (tests/bake_irradiance_ref.py) draws what it says and is worth testing against, and the device's own code for a
sample's first ray - the WfGroupPoints branch of wf_new_sample, built for the host as a stand-alone program with the address
and undefined-behaviour sanitizers (tools/table_ray_host.cpp) - gives the reference's (o, d') bit for bit."""
import ctypes as C
import inspect
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bake_irradiance_ref as br
from rust_raytracer_amd import api
from rust_raytracer_amd import build as rt_build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rt_mi355.h")
RTRACE = os.path.join(REPO, "rust_raytracer_amd", "rtrace")
ENTRY_POINTS = ("rt_bake_irradiance", "rt_bake_irradiance_device", "rt_bake_irradiance_hits_device")


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    lib = C.CDLL(api.DEVICE_LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert hasattr(C.CDLL(api.HOST_LIB_PATH), "rth_irradiance")


def test_python_signatures():
    sig = inspect.signature(api.DeviceScene.bake_irradiance)
    assert list(sig.parameters) == ["self", "positions", "normals", "params"]
    sig = inspect.signature(api.DeviceScene.bake_irradiance_device)
    assert list(sig.parameters) == ["self", "n", "d_positions_ptr", "d_normals_ptr", "params", "d_out_ptr", "stream"]
    sig = inspect.signature(api.DeviceScene.bake_irradiance_hits_device)
    assert list(sig.parameters) == ["self", "n", "d_hits_ptr", "params", "d_out_ptr", "stream"]


def test_hit_record_layout_matches_the_header(tmp_path):
    """Where the hit-record variant reads: pos at 8, normal at 32, flags at 84, 96 bytes apart."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler to check the header with")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %u %u\\n", sizeof(RtRayHit), offsetof(RtRayHit, pos), offsetof(RtRayHit, normal), '
                   "offsetof(RtRayHit, flags), RT_RAY_HIT, RT_RAY_ENVIRONMENT); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    h = api.RtRayHit
    assert out == [96, 8, 32, 84, 1, 4]
    assert out[:4] == [h.itemsize, h.fields["pos"][1], h.fields["normal"][1], h.fields["flags"][1]]


def test_argument_errors_need_no_device():
    lib = api.load_device_lib()
    buf = (C.c_double * 16)()
    p = api.RtRenderParams()
    assert lib.rt_bake_irradiance(None, 1, buf, buf, C.byref(p), buf) == api.RT_E_INVALID
    assert b"rt_bake_irradiance: scene is NULL" in lib.rt_last_error()
    assert lib.rt_bake_irradiance_device(None, 1, buf, buf, C.byref(p), buf, None) == api.RT_E_INVALID
    assert b"rt_bake_irradiance_device: scene is NULL" in lib.rt_last_error()
    assert lib.rt_bake_irradiance_hits_device(None, 1, buf, C.byref(p), buf, None) == api.RT_E_INVALID
    assert b"rt_bake_irradiance_hits_device: scene is NULL" in lib.rt_last_error()


# ---- rtrace --irradiance ----
def test_irradiance_flag():
    assert api.HostScene(["scenes/cornell", "-w=8"]).irradiance is False
    assert api.HostScene(["scenes/cornell", "-w=8", "--irradiance"]).irradiance is True
    assert api.HostScene(["scenes/cornell", "-w=8", "--irradiance", "--denoise=2", "--light-groups", "--precision=f32"]).irradiance is True
    for other in ("--gpus=2", "--progressive=1", "--noise-threshold=0.1", "--pick=0,0", "--ao=4", "--probe=1,2,3"):
        with pytest.raises(api.RtError, match="--irradiance bakes the whole frame"):
            api.HostScene(["scenes/cornell", "-w=8", "--irradiance", other])


@pytest.mark.parametrize("scene, flags, message", [
    ("scenes/cornell", ["--gpus=2"], "cannot be combined with --gpus > 1"),
    ("scenes/cornell", ["--progressive=2"], "--progressive"),
    ("scenes/cornell", ["--pick=1,1"], "--pick"),
    ("scenes/cornell", ["--ao=16"], "--ao or --probe"),
    ("scenes/cornell", ["--probe=1,2,3"], "--ao or --probe"),
])
def test_rtrace_rejects_bad_irradiance_combinations_before_touching_a_device(tmp_path, scene, flags, message):
    r = subprocess.run([RTRACE, os.path.join(REPO, scene), "-w=16", "-s=4", "--irradiance"] + flags, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "--irradiance" in r.stderr and message in r.stderr
    assert "Rendering" not in r.stdout
    assert not (tmp_path / "out_irradiance.png").exists() and not (tmp_path / "out.png").exists()


# ---- the reference itself ----
NORMALS = [(0.0, 1.0, 0.0), (0.0, 0.0, -2.5), (0.95, 0.1, -0.2), (-1.0, 2.0, 3.0)]   # both branches of onb_from_vec (|w.x| > 0.9), not unit length


@pytest.mark.parametrize("normal", NORMALS)
def test_reference_directions(normal):
    """4 096 samples of point 5: S = 8 (64 strata) x T = 64."""
    s, t, i = 8, 64, 5
    n = np.array(normal)
    unit = n / np.linalg.norm(n)
    uu = np.array([[br.uniforms(br.SEED, tt, i, st % s, st // s, s) for st in range(s * s)] for tt in range(t)])   # (t, s * s, 2)
    for st in range(s * s):
        sx, sy = st % s, st // s
        assert (uu[:, st, 0] >= sx / s).all() and (uu[:, st, 0] <= (sx + 1) / s).all(), f"u1 outside the cell of stratum ({sx}, {sy})"
        assert (uu[:, st, 1] >= sy / s).all() and (uu[:, st, 1] <= (sy + 1) / s).all(), f"u2 outside the cell of stratum ({sx}, {sy})"
    d = np.array([br.direction(u1, u2, n) for u1, u2 in uu.reshape(-1, 2)])
    assert len(d) == 4096
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 1e-15
    assert (d @ unit >= 0.0).all()
    # a cosine-weighted direction has mean (2/3) n: E[z] = E[sqrt(1 - u2)] = 2/3, E[x] = E[y] = 0; the standard error of a
    # component's mean over 4 096 samples is below 0.5 / 64 = 0.008 (stratification only lowers it)
    assert np.abs(d.mean(axis=0) - (2.0 / 3.0) * unit).max() <= 0.05
    # the round trip through the camera moves a direction by roundings of the position's size, not more
    o = np.array([278.0, -1.25, 3.5])
    d1 = (o + d) - o
    assert np.abs(d1 - d).max() <= 2.0 ** -43 and (d1 != d).any()
    # streams differ by point, replica and seed
    assert br.uniforms(br.SEED, 0, i, 0, 0, s) != br.uniforms(br.SEED, 0, i + 1, 0, 0, s)
    assert br.uniforms(br.SEED, 0, i, 0, 0, s) != br.uniforms(br.SEED, 1, i, 0, 0, s)
    assert br.uniforms(br.SEED, 0, i, 0, 0, s) != br.uniforms(br.SEED + 1, 0, i, 0, 0, s)


# every case the GPU tests compare against the oracle (tests/test_gpu_bake_irradiance.py)
GPU_CASES = [(name, br.N, br.S, br.T) for name in br.SCENES] + [("cornell", 64, 8, 1), ("two_meshes", 64, 8, 1)]


@pytest.mark.parametrize("name,n,s,t", GPU_CASES)
def test_point_sets_are_not_vacuous(name, n, s, t):
    c = br.case(name, n, s, t)
    assert c.pos.shape == c.nrm.shape == (n, 3) and c.ref.shape == (n, 4)
    assert np.abs(np.linalg.norm(c.nrm, axis=1) - 1.0).max() <= 1e-12
    br.assert_not_vacuous(c)


def test_reference_is_keyed_by_the_global_index():
    """oracle_bake(points k.., first = k) = rows k.. of the whole reference: what chunking and 'point i alone' rely on."""
    c = br.case("cornell")
    part = br.oracle_bake(c.hs.desc, c.params, c.pos[30:], c.nrm[30:], first=30)
    assert part.tobytes() == c.ref[30:].tobytes()
    moved = br.oracle_bake(c.hs.desc, c.params, c.pos[30:31], c.nrm[30:31], first=0)
    assert moved.tobytes() != c.ref[30:31].tobytes()


# ---- the device's code for the first ray, on the host, under sanitizers ----
@pytest.mark.parametrize("stride", [24, 96])
def test_device_code_on_the_host_gives_the_reference_rays(tmp_path, stride):
    """tools/table_ray_host.cpp: wf_new_sample<double, WfGroupPoints<double>> compiled for the host (sanitizers on the host side
    only; the program touches no GPU).  Points: cornell's and two_meshes', as plain arrays and as hit records, at index 5 onwards."""
    exe = tmp_path / "table_ray_host"
    cmd = [rt_build.hipcc_path(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-I" + os.path.join(REPO, "include"), "-o", str(exe), os.path.join(REPO, "tools", "table_ray_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    first = 5
    for name in ("cornell", "two_meshes"):
        c = br.case(name)
        if stride == 24:
            data = c.pos.tobytes() + c.nrm.tobytes()
        else:
            hits = np.zeros(c.n, dtype=api.RtRayHit)
            hits["pos"], hits["normal"], hits["flags"] = c.pos, c.nrm, 1
            data = hits.tobytes()
        (tmp_path / "in.bin").write_bytes(struct.pack("<QIIQII", c.seed, c.s, c.t, first, c.n, stride) + data)
        r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        got = np.fromfile(str(tmp_path / "out.bin")).reshape(-1, 6)
        want = br.first_rays(c.pos, c.nrm, c.s, c.t, c.seed, first)
        assert got.shape == want.shape == (c.n * c.t * c.s * c.s, 6)
        assert got.tobytes() == want.tobytes(), f"{name}: {int((got != want).any(axis=1).sum())} first rays differ"
