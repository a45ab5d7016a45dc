"""First-hit AOVs and the denoiser without a GPU: the C ABI is declared and exported, RtDenoiseParams has its ctypes
mirror's layout, argument errors come back before any device is touched, `rtrace --denoise` is checked while the command
line is read, and the numpy reference filter (tests/denoise_ref.py, which the GPU tests hold the kernels to) keeps its
defining properties."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref
from rust_raytracer_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rt_mi355.h")
RTRACE = os.path.join(REPO, "rust_raytracer_amd", "rtrace")
ENTRY_POINTS = ("rt_render_aov", "rt_render_aov_device", "rt_denoise_default_params", "rt_denoise", "rt_denoise_device",
                "rt_accum_estimate_denoised", "rt_accum_preview_denoised_rgb8")


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    lib = C.CDLL(api.DEVICE_LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    host = C.CDLL(api.HOST_LIB_PATH)
    assert hasattr(host, "rth_denoise")


def test_denoise_params_layout_matches_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler to check the header with")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(RtDenoiseParams), '
                   "offsetof(RtDenoiseParams, flags), offsetof(RtDenoiseParams, sigma_color), "
                   "offsetof(RtDenoiseParams, sigma_depth), offsetof(RtDenoiseParams, _reserved), "
                   "(size_t)RT_DENOISE_DEMODULATE); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    m = api.RtDenoiseParams
    assert out == [C.sizeof(m), m.flags.offset, m.sigma_color.offset, m.sigma_depth.offset, m._reserved.offset,
                   api.RT_DENOISE_DEMODULATE]


def test_default_params():
    dp = api.RtDenoiseParams.defaults()
    assert (dp.iterations, dp.aov_replicas, dp.flags) == (4, 1, api.RT_DENOISE_DEMODULATE)
    assert list(dp._reserved) == [0.0] * 4
    assert denoise_ref.params_of(dp) == denoise_ref.DEFAULTS


def test_argument_errors_need_no_device():
    lib = api.load_device_lib()
    hs = api.HostScene(["scenes/cornell", "-w=16", "-s=4"])
    buf = (C.c_double * 64)()
    assert lib.rt_render_aov(None, C.byref(hs.camera), C.byref(hs.params), 1, buf) == api.RT_E_INVALID
    assert lib.rt_render_aov_device(None, None, None, 1, None, None) == api.RT_E_INVALID
    assert lib.rt_denoise_default_params(None) == api.RT_E_INVALID
    assert lib.rt_denoise(0, None, buf, 4, 4, None, buf) == api.RT_E_INVALID
    assert lib.rt_denoise_device(0, buf, buf, 4, 4, None, None, None) == api.RT_E_INVALID
    dp = api.RtDenoiseParams.defaults(iterations=api.RT_DENOISE_MAX_ITERATIONS + 1)
    assert lib.rt_denoise(0, buf, buf, 1, 1, C.byref(dp), buf) == api.RT_E_INVALID
    assert b"iterations" in lib.rt_last_error()
    dp = api.RtDenoiseParams.defaults(sigma_depth=0.0)
    assert lib.rt_denoise(0, buf, buf, 1, 1, C.byref(dp), buf) == api.RT_E_INVALID
    assert b"sigma" in lib.rt_last_error()
    assert lib.rt_accum_estimate_denoised(None, None, buf) == api.RT_E_INVALID
    assert lib.rt_accum_preview_denoised_rgb8(None, None, buf) == api.RT_E_INVALID


def test_host_reports_denoise_flag():
    lib = api.load_host_lib()
    lib.rth_denoise.argtypes = [C.c_void_p]
    lib.rth_denoise.restype = C.c_uint32
    assert lib.rth_denoise(api.HostScene(["scenes/cornell", "-w=16", "-s=4", "--denoise=5"])._h) == 5
    assert lib.rth_denoise(api.HostScene(["scenes/cornell", "-w=16", "-s=4", "--denoise=5", "--progressive=2"])._h) == 5
    assert lib.rth_denoise(api.HostScene(["scenes/cornell", "-w=16", "-s=4"])._h) == 0


@pytest.mark.parametrize("flags, message", [
    (["--denoise=5", "--gpus=2"], "cannot be combined with --gpus > 1"),
    (["--denoise=x"], "Denoise iterations must be an integer from 1 to 16"),
    (["--denoise=0"], "Denoise iterations must be an integer from 1 to 16"),
    (["--denoise=17"], "Denoise iterations must be an integer from 1 to 16"),
])
def test_rtrace_rejects_bad_denoise_flags_before_touching_a_device(tmp_path, flags, message):
    r = subprocess.run([RTRACE, os.path.join(REPO, "scenes", "cornell"), "-w=16", "-s=4"] + flags, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert message in r.stderr
    assert "Rendering" not in r.stdout
    assert not (tmp_path / "out_denoised.png").exists()


# ---- the numpy reference filter ----------------------------------------------------------------------------------------

def guides(h, w, seed=0, const_albedo=None):
    rng = np.random.default_rng(seed)
    aov = np.zeros((h, w, 8))
    aov[..., 0:3] = rng.uniform(0.0, 1.0, (h, w, 3)) if const_albedo is None else const_albedo
    n = rng.normal(size=(h, w, 3))
    aov[..., 3:6] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    aov[..., 6] = rng.uniform(1.0, 5.0, (h, w))
    aov[..., 7] = 1.0
    return aov


def noisy(h, w, seed=1):
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 4))
    img[..., :3] = rng.exponential(1.0, (h, w, 3))
    return img


@pytest.mark.parametrize("n", [1, 3, 5])
def test_reference_keeps_a_constant_image_constant(n):
    h, w = 23, 37
    img = np.zeros((h, w, 4))
    img[..., :3] = [0.25, 1.5, 3.0]
    out = denoise_ref.denoise(img, guides(h, w), iterations=n, demodulate=False)  # any guides
    np.testing.assert_allclose(out, img, rtol=1e-13, atol=0)
    out = denoise_ref.denoise(img, guides(h, w, const_albedo=[0.5, 0.2, 0.0005]), iterations=n)  # one albedo: demodulated too
    np.testing.assert_allclose(out, img, rtol=1e-13, atol=0)


def test_reference_with_zero_iterations_is_the_identity():
    img = noisy(9, 11)
    img[2, 3, 1] = np.nan
    img[..., 3] = 0.5
    out = denoise_ref.denoise(img, guides(9, 11), iterations=0)
    assert out.tobytes() == img.tobytes()


def test_reference_smooths_noise_and_keeps_alpha():
    h, w = 32, 32
    img = noisy(h, w)
    img[..., 3] = 0.25
    aov = guides(h, w, const_albedo=[1.0, 1.0, 1.0])
    aov[..., 3:6] = [0.0, 0.0, 1.0]
    aov[..., 6] = 2.0
    out = denoise_ref.denoise(img, aov, iterations=3, sigma_color=10.0)
    assert out[..., :3].std() < 0.5 * img[..., :3].std()
    assert (out[..., 3] == 0.25).all()
    assert np.isfinite(out).all()


def test_reference_non_finite_handling():
    h, w = 16, 16
    img = noisy(h, w)
    aov = guides(h, w)
    img[5, 7, 0] = np.nan
    img[9, 2, :3] = np.inf
    out = denoise_ref.denoise(img, aov, iterations=4)
    finite_in = np.isfinite(img[..., :3]).all(-1)
    # no finite pixel becomes non-finite, and a non-finite one is filled from its finite taps (its colour weight is 1)
    assert np.isfinite(out[finite_in]).all()
    assert np.isfinite(out[5, 7]).all() and np.isfinite(out[9, 2]).all()
    # a pixel without a finite tap keeps its value: an image that is not finite anywhere stays as it is
    bad = np.full((6, 5, 4), np.nan)
    bad[..., 3] = 0.0
    out = denoise_ref.denoise(bad, guides(6, 5), iterations=2, demodulate=False)
    assert out.tobytes() == bad.tobytes()
    # a finite pixel whose own guides are NaN has no tap with a positive weight either
    aov2 = aov.copy()
    aov2[3, 3, 3:6] = np.nan
    out = denoise_ref.denoise(img, aov2, iterations=1, demodulate=False)
    assert out[3, 3].tobytes() == img[3, 3].tobytes()


def test_reference_respects_albedo_and_normal_edges():
    h, w = 16, 16
    img = np.zeros((h, w, 4))
    img[:, :8, :3] = 0.2
    img[:, 8:, :3] = 0.9
    aov = guides(h, w, const_albedo=[1.0, 1.0, 1.0])
    aov[..., 3:6] = [0.0, 1.0, 0.0]
    aov[:, 8:, 3:6] = [1.0, 0.0, 0.0]  # a normal edge where the colour jumps
    aov[..., 6] = 3.0
    out = denoise_ref.denoise(img, aov, iterations=5, sigma_color=100.0)
    np.testing.assert_allclose(out[..., :3], img[..., :3], rtol=1e-6)  # nothing leaks across the edge
