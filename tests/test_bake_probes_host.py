"""The SH probe bake without a GPU: the C ABI is declared and exported, argument errors need no device,
`rtrace --sh-probe` is checked while the command line is read, the reference the GPU tests hold the kernels to
(tests/bake_probes_ref.py) draws what it says and is worth testing against, api.probe_grid is the grid numpy gives, and the
device's own code for a sample's first ray and SH weights - the WfGroupProbes branch of wf_new_sample and what k_wf_resolve_sh
evaluates per sample, built for the host as a stand-alone program with the address and undefined-behaviour sanitizers
(tools/table_ray_host.cpp) - gives the reference's (o, d') and the nine Y_k bit for bit."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bake_probes_ref as bp
from rust_raytracer_amd import api
from rust_raytracer_amd import build as rt_build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rt_mi355.h")
RTRACE = os.path.join(REPO, "rust_raytracer_amd", "rtrace")
ENTRY_POINTS = ("rt_bake_probes", "rt_bake_probes_device", "rt_sh_irradiance", "rt_sh_irradiance_device")


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert "RT_MI355_ABI_VERSION 2 " in text   # additions only: the version stands
    lib = C.CDLL(api.DEVICE_LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert hasattr(C.CDLL(api.HOST_LIB_PATH), "rth_sh_probes")


def test_python_signatures():
    sig = inspect.signature(api.DeviceScene.bake_probes)
    assert list(sig.parameters) == ["self", "positions", "params"]
    sig = inspect.signature(api.DeviceScene.bake_probes_device)
    assert list(sig.parameters) == ["self", "n", "d_positions_ptr", "params", "d_out_ptr", "stream"]
    sig = inspect.signature(api.sh_irradiance)
    assert list(sig.parameters) == ["sh", "probe", "normals", "device"] and sig.parameters["device"].default == 0
    sig = inspect.signature(api.probe_grid)
    assert list(sig.parameters) == ["lo", "hi", "counts"]


def test_argument_errors_need_no_device():
    lib = api.load_device_lib()
    buf = (C.c_double * 64)()
    idx = (C.c_uint32 * 4)(0, 1, 5, 0)
    p = api.RtRenderParams()
    assert lib.rt_bake_probes(None, 1, buf, C.byref(p), buf) == api.RT_E_INVALID
    assert b"rt_bake_probes: scene is NULL" in lib.rt_last_error()
    assert lib.rt_bake_probes_device(None, 1, buf, C.byref(p), buf, None) == api.RT_E_INVALID
    assert b"rt_bake_probes_device: scene is NULL" in lib.rt_last_error()
    out = np.full((4, 4), 7.0)
    assert lib.rt_sh_irradiance(0, None, 2, idx, buf, 4, out.ctypes.data) == api.RT_E_INVALID
    assert b"rt_sh_irradiance: NULL argument" in lib.rt_last_error()
    assert lib.rt_sh_irradiance(0, buf, 2, idx, buf, 4, out.ctypes.data) == api.RT_E_INVALID   # probe[2] = 5 >= 2
    assert b"probe[2] = 5" in lib.rt_last_error()
    assert lib.rt_sh_irradiance(0, buf, 2, idx, buf, 2 ** 31, out.ctypes.data) == api.RT_E_INVALID
    assert lib.rt_sh_irradiance_device(0, buf, 2, None, buf, 4, out.ctypes.data, None) == api.RT_E_INVALID
    assert b"rt_sh_irradiance_device: NULL argument" in lib.rt_last_error()
    assert (out == 7.0).all()
    assert lib.rt_sh_irradiance(0, None, 0, None, None, 0, None) == api.RT_OK   # m = 0 is a no-op
    with pytest.raises(ValueError):
        api.sh_irradiance(np.zeros((2, 9, 3)), [0], [0.0, 1.0, 0.0])
    with pytest.raises(ValueError):
        api.sh_irradiance(np.zeros((2, 9, 4)), [-1], [0.0, 1.0, 0.0])
    with pytest.raises(api.RtError, match=r"probe\[1\] = 2"):
        api.sh_irradiance(np.zeros((2, 9, 4)), [1, 2], [0.0, 1.0, 0.0])


# ---- api.probe_grid ----
def test_probe_grid_against_numpy():
    lo, hi, counts = (-1.0, 0.5, 10.0), (3.0, 2.5, 16.0), (4, 1, 3)
    g = api.probe_grid(lo, hi, counts)
    assert g.shape == (12, 3) and g.dtype == np.float64 and g.flags["C_CONTIGUOUS"]
    want = np.array([[lo[a] + (hi[a] - lo[a]) * ((i[a] + 0.5) / counts[a]) for a in range(3)]
                     for i in ((ix, iy, iz) for iz in range(counts[2]) for iy in range(counts[1]) for ix in range(counts[0]))])
    assert g.tobytes() == want.tobytes()
    assert (g[1] - g[0] == (1.0, 0.0, 0.0)).all() and (g[4] - g[0] == (0.0, 0.0, 2.0)).all()   # x fastest, then y (one cell), then z
    assert (g > np.array(lo)).all() and (g < np.array(hi)).all()                                # cell centres, not corners
    assert api.probe_grid(lo, hi, (1, 1, 1)).tolist() == [[1.0, 1.5, 13.0]]
    for bad in ((0, 1, 1), (1, 1), (1.5, 1, 1)):
        with pytest.raises(ValueError):
            api.probe_grid(lo, hi, bad)


# ---- rtrace --sh-probe ----
def test_sh_probe_flag():
    assert api.HostScene(["scenes/cornell", "-w=8"]).sh_probes.shape == (0, 3)
    hs = api.HostScene(["scenes/cornell", "-w=8", "--sh-probe=278,273,-100"])
    assert hs.sh_probes.tolist() == [[278.0, 273.0, -100.0]]
    hs = api.HostScene(["scenes/cornell", "-w=8", "--sh-probe=1,2,3:-0.5,1e2,7:0,0,0", "--precision=f32", "--light-groups", "--denoise=2"])
    assert hs.sh_probes.tolist() == [[1.0, 2.0, 3.0], [-0.5, 100.0, 7.0], [0.0, 0.0, 0.0]]
    for bad in ("--sh-probe=1,2", "--sh-probe=1,2,3:", "--sh-probe=1,2,x", "--sh-probe=1,2,inf", "--sh-probe=1,2,3:4,5"):
        with pytest.raises(api.RtError, match="SH probes must be a list of positions"):
            api.HostScene(["scenes/cornell", "-w=8", bad])
    for other in ("--gpus=2", "--progressive=1", "--noise-threshold=0.1", "--pick=0,0", "--ao=4", "--probe=1,2,3", "--irradiance",
                  "--pipeline=mega"):
        with pytest.raises(api.RtError, match="--sh-probe bakes probes"):
            api.HostScene(["scenes/cornell", "-w=8", "--sh-probe=1,2,3", other])


@pytest.mark.parametrize("flags, message", [
    (["--gpus=2"], "cannot be combined with --gpus > 1"),
    (["--progressive=2"], "--progressive"),
    (["--pick=1,1"], "--pick"),
    (["--ao=16"], "--ao"),
    (["--probe=1,2,3"], "--probe"),
    (["--irradiance"], "--irradiance"),
    (["--sequence=scenes/cornell"], "--sequence"),
    (["--max-depth=0"], "depth of at least 1"),
])
def test_rtrace_rejects_bad_sh_probe_combinations_before_touching_a_device(tmp_path, flags, message):
    r = subprocess.run([RTRACE, os.path.join(REPO, "scenes/cornell"), "-w=16", "-s=4", "--sh-probe=278,273,-100"] + flags, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "--sh-probe" in r.stderr and message in r.stderr
    assert "SH probe 0" not in r.stdout and "no HIP device" not in r.stderr
    assert not (tmp_path / "out.png").exists()


# ---- the reference itself ----
def test_reference_directions_and_basis():
    """4 096 samples of probe 5: S = 8 (64 strata) x T = 64."""
    s, t, i = 8, 64, 5
    uu = np.array([[bp.uniforms(bp.SEED, tt, i, st % s, st // s, s) for st in range(s * s)] for tt in range(t)])   # (t, s * s, 2)
    d = np.array([bp.direction(u1, u2) for u1, u2 in uu.reshape(-1, 2)])
    assert len(d) == 4096
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 1e-15
    assert d.tobytes() == bp.sample_dirs(1, s, t, bp.SEED, first=i).reshape(-1, 3).tobytes()
    # z = 1 - 2 u2 exactly as written; every octant is visited; the mean of a uniform direction is 0 (standard error of a
    # component's mean over 4 096 samples: sqrt(1/3) / 64 = 0.009; stratification only lowers it)
    assert (d[:, 2] == 1.0 - 2.0 * uu.reshape(-1, 2)[:, 1]).all()
    assert len({tuple(row) for row in (d > 0)}) == 8
    assert np.abs(d.mean(axis=0)).max() <= 0.05
    # the basis is orthonormal over the sphere: 4 pi * mean(Y_j Y_k) = delta_jk.  The largest variance of a product is below
    # max |Y_j Y_k|^2 <= (0.6308^2)^2 = 0.16, so 4 pi * the standard error is below 4 pi * 0.4 / 64 = 0.08
    y = np.array([bp.basis(v) for v in d])
    gram = 4.0 * np.pi * (y.T @ y) / len(y)
    assert np.abs(gram - np.eye(9)).max() <= 0.08
    assert (np.abs(y).max(axis=0) <= bp.Y_MAX * (1 + 1e-15)).all() and (np.abs(y).max(axis=0) >= 0.9 * bp.Y_MAX).all()
    # the poles and the equator of the closed forms
    assert bp.basis((0.0, 0.0, 1.0)).tolist() == [bp.C0, 0.0, bp.C1, 0.0, 0.0, 0.0, bp.C2B * 2.0, 0.0, 0.0]
    assert bp.basis((1.0, 0.0, 0.0)).tolist() == [bp.C0, 0.0, 0.0, bp.C1, 0.0, 0.0, -bp.C2B, 0.0, bp.C2C]
    assert bp.Y_MAX[6] == 2.0 * bp.C2B and bp.C2A == 2.0 * bp.C2C
    # streams differ by probe, replica and seed
    assert bp.uniforms(bp.SEED, 0, i, 0, 0, s) != bp.uniforms(bp.SEED, 0, i + 1, 0, 0, s)
    assert bp.uniforms(bp.SEED, 0, i, 0, 0, s) != bp.uniforms(bp.SEED, 1, i, 0, 0, s)
    assert bp.uniforms(bp.SEED, 0, i, 0, 0, s) != bp.uniforms(bp.SEED + 1, 0, i, 0, 0, s)


@pytest.mark.parametrize("name", bp.SCENES)
def test_probe_sets_are_not_vacuous(name):
    c = bp.case(name)
    assert c.pos.shape == (bp.N, 3) and c.ref.shape == (bp.N, 9, 4)
    bp.assert_not_vacuous(c)


def test_reference_is_keyed_by_the_global_index():
    """oracle_probes(probes k.., first = k) = rows k.. of the whole reference: what chunking and `first != 0` rely on."""
    c = bp.case("cornell")
    part = bp.oracle_probes(c.hs.desc, c.params, c.pos[30:], first=30)
    assert part.tobytes() == c.ref[30:].tobytes()
    moved = bp.oracle_probes(c.hs.desc, c.params, c.pos[30:], first=0)
    assert moved.tobytes() != c.ref[30:].tobytes()


# ---- the device's code for the first ray and the SH weights, on the host, under sanitizers ----
def test_device_code_on_the_host_gives_the_reference_rays_and_basis(tmp_path):
    """tools/table_ray_host.cpp: wf_new_sample<double, WfGroupProbes<double>> and the per-sample arithmetic of k_wf_resolve_sh
    compiled for the host (sanitizers on the host side only; the program touches no GPU).  Probes: cornell's and two_meshes', at
    index 5 onwards."""
    exe = tmp_path / "table_ray_host"
    cmd = [rt_build.hipcc_path(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-I" + os.path.join(REPO, "include"), "-o", str(exe), os.path.join(REPO, "tools", "table_ray_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    first = 5
    for name in ("cornell", "two_meshes"):
        c = bp.case(name)
        (tmp_path / "in.bin").write_bytes(struct.pack("<QIIQII", c.seed, c.s, c.t, first, c.n, 0) + c.pos.tobytes())
        r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        got = np.fromfile(str(tmp_path / "out.bin")).reshape(-1, 15)
        rays = bp.first_rays(c.pos, c.s, c.t, c.seed, first)
        ys = np.array([bp.basis(d) for d in bp.sample_dirs(c.n, c.s, c.t, c.seed, first).reshape(-1, 3)])
        assert got.shape == (c.n * c.t * c.s * c.s, 15)
        assert got[:, :6].tobytes() == rays.tobytes(), f"{name}: {int((got[:, :6] != rays).any(axis=1).sum())} first rays differ"
        assert got[:, 6:].tobytes() == np.ascontiguousarray(ys).tobytes(), f"{name}: {int((got[:, 6:] != ys).any(axis=1).sum())} bases differ"
