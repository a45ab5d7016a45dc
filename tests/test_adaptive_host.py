"""Adaptive sampling without a GPU: the C ABI is declared and exported, RtAdaptiveParams has one size in C and ctypes and
the existing structs keep theirs, argument errors come back before any device is touched, `rtrace` rejects bad adaptive
flags while it reads the command line, and the rule itself (tests/adaptive_ref.py) does what include/rt_mi355.h says: on
hand-made cases and on the CPU oracle's frames, where it has to reproduce the experiment of DESIGN.md section 11."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
from oracle import pyoracle
from rust_raytracer_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rt_mi355.h")
RTRACE = os.path.join(REPO, "rust_raytracer_amd", "rtrace")
ENTRY_POINTS = ("rt_adaptive_default_params", "rt_accum_set_adaptive", "rt_accum_active_pixels", "rt_accum_finished",
                "rt_accum_sample_counts", "rt_accum_noise")


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    lib = C.CDLL(api.DEVICE_LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert "RT_MI355_ABI_VERSION 2 " in text


def test_struct_sizes(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler to check the header with")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "rt_mi355.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d\\n", '
                   "sizeof(RtAdaptiveParams), sizeof(RtRenderParams), sizeof(RtRenderStats), sizeof(RtDenoiseParams), "
                   "sizeof(RtCameraDesc), RT_MI355_ABI_VERSION); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [64, 80, 152, 80, 168, 2]
    assert [C.sizeof(s) for s in (api.RtAdaptiveParams, api.RtRenderParams, api.RtRenderStats, api.RtDenoiseParams,
                                  api.RtCameraDesc)] == sizes[:5]


def test_defaults_and_argument_errors_need_no_device():
    lib = api.load_device_lib()
    ap = api.RtAdaptiveParams.defaults()
    assert (ap.threshold, ap.floor, ap.min_replicas, ap.check_interval, ap.radius) == (0.0, 0.01, 4, 2, 1)
    assert ap._reserved0 == 0 and list(ap._reserved) == [0.0] * 4
    assert {k: getattr(ap, k) for k in ar.DEFAULTS} == ar.DEFAULTS
    assert api.RtAdaptiveParams.defaults(threshold=0.1, radius=2).radius == 2
    assert lib.rt_adaptive_default_params(None) == api.RT_E_INVALID
    assert lib.rt_accum_set_adaptive(None, C.byref(ap)) == api.RT_E_INVALID
    assert b"NULL" in lib.rt_last_error()
    assert lib.rt_accum_active_pixels(None) == 0
    assert lib.rt_accum_finished(None) == 0
    assert lib.rt_accum_sample_counts(None, None) == api.RT_E_INVALID
    assert lib.rt_accum_noise(None, None) == api.RT_E_INVALID


@pytest.mark.parametrize("flags, message", [
    (["--noise-threshold=0"], "Noise threshold must be a number > 0"),
    (["--noise-threshold=-0.5"], "Noise threshold must be a number > 0"),
    (["--noise-threshold=abc"], "Noise threshold must be a number > 0"),
    (["--noise-threshold=0.1", "--adaptive-min=1"], "Adaptive minimum must be an integer >= 2"),
    (["--noise-threshold=0.1", "--adaptive-check=0"], "Adaptive check interval must be a positive integer"),
    (["--noise-threshold=0.1", "--adaptive-radius=5"], "Adaptive radius must be an integer from 0 to 4"),
    (["--adaptive-min=4"], "require --noise-threshold"),
    (["--adaptive-radius=1"], "require --noise-threshold"),
    (["--noise-threshold=0.1", "--gpus=2"], "cannot be combined with --gpus > 1"),
    (["--noise-threshold=0.1", "--pipeline=mega"], "cannot be combined with --pipeline=mega"),
    (["--noise-threshold=0.1", "--time-limit=10"], "--time-limit requires --checkpoint"),
])
def test_rtrace_rejects_bad_adaptive_flags_before_touching_a_device(tmp_path, flags, message):
    r = subprocess.run([RTRACE, os.path.join(REPO, "scenes", "cornell"), "-w=16", "-s=4"] + flags, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert message in r.stderr
    assert "Rendering" not in r.stdout  # nothing ran: the flags are checked while the command line is read


def test_host_reports_adaptive_flags():
    lib = api.load_host_lib()
    for name, res in (("rth_noise_threshold", C.c_double), ("rth_adaptive_min", C.c_int32), ("rth_adaptive_check", C.c_int32),
                      ("rth_adaptive_radius", C.c_int32), ("rth_progressive", C.c_uint32), ("rth_checkpoint", C.c_char_p)):
        getattr(lib, name).argtypes = [C.c_void_p]
        getattr(lib, name).restype = res
    hs = api.HostScene(["scenes/cornell", "-w=16", "-s=4", "--noise-threshold=0.25", "--adaptive-min=3", "--adaptive-check=5",
                        "--adaptive-radius=0", "--checkpoint=run.state"])  # a checkpoint needs no --progressive here
    assert lib.rth_noise_threshold(hs._h) == 0.25 and lib.rth_adaptive_min(hs._h) == 3
    assert lib.rth_adaptive_check(hs._h) == 5 and lib.rth_adaptive_radius(hs._h) == 0
    assert lib.rth_progressive(hs._h) == 0 and lib.rth_checkpoint(hs._h) == b"run.state"
    hs = api.HostScene(["scenes/cornell", "-w=16", "-s=4", "--noise-threshold=0.1"])
    assert lib.rth_noise_threshold(hs._h) == 0.1
    assert (lib.rth_adaptive_min(hs._h), lib.rth_adaptive_check(hs._h), lib.rth_adaptive_radius(hs._h)) == (-1, -1, -1)
    hs = api.HostScene(["scenes/cornell", "-w=16", "-s=4"])
    assert lib.rth_noise_threshold(hs._h) == 0.0


# ---- the rule on hand-made cases ----------------------------------------------------------------------------------

def test_decision_points():
    assert ar.decision_points(8, 2, 2) == [2, 4, 6]
    assert ar.decision_points(32, 4, 2) == list(range(4, 32, 2))
    assert ar.decision_points(10, 3, 4) == [3, 7]
    assert ar.decision_points(5, 4, 1) == [4]
    assert ar.decision_points(4, 4, 1) == []      # min_replicas >= T: no decision point
    assert ar.decision_points(7, 2, 100) == [2]


def grey(values):
    """(T, H, W) luminance-like values -> contributions whose luminance y = T * value (r = g = b)."""
    v = np.asarray(values, dtype=np.float64)
    return np.repeat(v[..., None], 3, axis=-1)


def test_one_noisy_pixel_holds_exactly_its_window():
    T = 4
    c = np.full((T, 5, 5), 0.25)
    c[:, 2, 2] = [0.0, 1.0, 0.0, 0.0]  # mean 0.25 like the others, but noisy
    for radius, held in ((0, 1), (1, 9), (2, 25)):
        sim = ar.simulate(grey(c), threshold=0.05, floor=0.01, min_replicas=2, check_interval=1, radius=radius)
        expect = np.full((5, 5), 2, dtype=np.uint32)
        expect[2 - radius:3 + radius, 2 - radius:3 + radius] = T
        np.testing.assert_array_equal(sim["n"], expect)
        assert int((sim["n"] == T).sum()) == held
        assert not sim["band"].any()
    # at the image border the window is clipped, not wrapped
    c = np.full((T, 5, 5), 0.25)
    c[:, 0, 4] = [0.0, 1.0, 0.0, 0.0]
    sim = ar.simulate(grey(c), threshold=0.05, floor=0.01, min_replicas=2, check_interval=1, radius=1)
    expect = np.full((5, 5), 2, dtype=np.uint32)
    expect[0:2, 3:5] = T
    np.testing.assert_array_equal(sim["n"], expect)


def test_a_nan_sum_never_stops_and_an_early_stop_never_meets_it():
    T = 6
    c = np.full((T, 3, 3), 0.5)
    c[0, 0, 0] = np.nan          # NaN from the first replica: never quiet
    c[3, 2, 2] = np.nan          # NaN in replica 3: the pixel has stopped at k = 2 already
    sim = ar.simulate(grey(c), threshold=0.1, floor=0.01, min_replicas=2, check_interval=2, radius=0)
    assert sim["n"][0, 0] == T and np.isnan(sim["sum"][0, 0]).all() and np.isnan(sim["s1"][0, 0])
    assert sim["n"][2, 2] == 2 and np.isfinite(sim["sum"][2, 2]).all()
    assert (np.delete(sim["n"].ravel(), 0) == 2).all()
    # with a window the NaN pixel holds its neighbours for good
    sim = ar.simulate(grey(c), threshold=0.1, floor=0.01, min_replicas=2, check_interval=2, radius=1)
    assert (sim["n"][:2, :2] == T).all() and sim["n"][0, 2] == 2
    assert not ar.quiet(np.array([np.nan]), np.array([1.0]), 4, 0.1, 0.01)[0]
    assert not ar.quiet(np.array([1.0]), np.array([np.nan]), 4, 0.1, 0.01)[0]


def test_stopped_pixels_do_not_hold_their_neighbours():
    # left column converges at k = 2; the middle column is noisy at k = 2 and quiet from k = 4 on; at k = 4 the stopped
    # left column's (noisy-looking, had it gone on) samples no longer matter
    T = 8
    c = np.full((T, 3, 3), 0.5)
    c[:, :, 1] = np.array([0.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5])[:, None]
    c[2:, :, 0] = np.array([0.0, 5.0, 0.0, 5.0, 0.0, 5.0])[:, None]  # never rendered: the column stops at k = 2
    sim = ar.simulate(grey(c), threshold=0.3, floor=0.01, min_replicas=2, check_interval=2, radius=0)
    assert (sim["n"][:, 0] == 2).all() and (sim["n"][:, 2] == 2).all()
    k_mid = int(sim["n"][0, 1])
    assert 2 < k_mid < T and (sim["n"][:, 1] == k_mid).all()
    # with radius 1 the middle column holds both neighbours at k = 2; all stop together later, and the sums are prefixes
    sim1 = ar.simulate(grey(c), threshold=0.3, floor=0.01, min_replicas=2, check_interval=2, radius=1)
    assert (sim1["n"][:, 2] > 2).all()
    for s in (sim, sim1):
        prefix = np.cumsum(grey(c), axis=0)
        idx = s["n"].astype(int) - 1
        got = np.take_along_axis(prefix, idx[None, ..., None].repeat(3, axis=-1), axis=0)[0]
        np.testing.assert_array_equal(s["sum"], got)
        assert set(np.unique(s["n"])) <= set(ar.decision_points(T, 2, 2)) | {T}


def test_moments_estimate_and_noise():
    T = 4
    rng = np.random.default_rng(3)
    c = rng.uniform(0, 1, (T, 2, 3, 3))
    sim = ar.simulate(c, threshold=1e-9, min_replicas=T)  # no decision point
    y = np.stack([ar.luminance(c[t], T) for t in range(T)])
    s1 = y[0] + y[1] + y[2] + y[3]
    s2 = y[0] * y[0] + y[1] * y[1] + y[2] * y[2] + y[3] * y[3]
    np.testing.assert_array_equal(sim["s1"], ((y[0] + y[1]) + y[2]) + y[3])
    np.testing.assert_allclose(sim["s1"], s1, rtol=1e-15)
    np.testing.assert_allclose(sim["s2"], s2, rtol=1e-15)
    assert (sim["n"] == T).all() and sim["active"].all()
    np.testing.assert_array_equal(ar.estimate(sim["sum"], sim["n"], T), sim["sum"])  # factor exactly 1
    half = ar.estimate(sim["sum"], np.full((2, 3), 2, dtype=np.uint32), T)
    np.testing.assert_array_equal(half, sim["sum"] * 2.0)
    # noise = standard error of the mean over (mean + floor), against numpy's own statistics
    want = np.std(y, axis=0, ddof=1) / np.sqrt(T) / (np.mean(y, axis=0) + 0.01)
    np.testing.assert_allclose(ar.noise(sim["s1"], sim["s2"], sim["n"], 0.01), want, rtol=1e-9)
    assert (ar.noise(sim["s1"], sim["s2"], np.ones((2, 3), dtype=np.uint32), 0.01) == 0.0).all()


# ---- the rule on the oracle's frames: the experiment of DESIGN.md section 11 ----------------------------------------

def oracle_contributions(args, T):
    """Per-replica contributions from the oracle: the frame of k replicas scaled by k / T is sum_k (the streams are
    keyed by the replica, not by T); differences of consecutive sums are the contributions."""
    hs = api.HostScene(args)
    assert hs.params.thread_count == T
    snaps = [np.zeros((hs.height, hs.width, 4))]
    for k in range(1, T + 1):
        p = hs.params.copy()
        p.thread_count = k
        frame, _ = pyoracle.render(hs.desc, hs.camera, p)
        snaps.append(frame * (k / T))
    return ar.contributions_from_snapshots(snaps), snaps[T]


@pytest.mark.parametrize("args, expect", [
    (["scenes/light_test", "-w=48", "-s=128", "-t=32", "--seed=42"],
     {0: (0.622, 0.467, 0.098), 1: (0.469, 0.602, 0.004), 2: (0.373, 0.683, 0.0)}),
    (["tests/scenes/texture_mix", "-w=48", "-s=128", "-t=32", "--seed=43"],
     {0: (0.618, 0.529, 0.087), 1: (0.438, 0.634, 0.001)}),
])
def test_rule_on_the_oracle_frames(args, expect):
    T, thr = 32, 0.1
    contrib, full = oracle_contributions(args, T)
    for radius, (stopped, rendered, over) in expect.items():
        sim = ar.simulate(contrib, threshold=thr, radius=radius)  # defaults otherwise
        q = ar.quality(ar.estimate(sim["sum"], sim["n"], T), full, sim["n"], T, thr)
        print(args[0], "radius", radius, q, "in the band:", int(sim["band"].sum()))
        # the table of DESIGN.md section 11, to the digits it prints
        assert abs(q["stopped"] - stopped) < 1e-3 and abs(q["rendered"] - rendered) < 1e-3 and abs(q["over"] - over) < 1e-3
        assert not sim["band"].any()
        assert set(np.unique(sim["n"])) <= set(ar.decision_points(T, 4, 2)) | {T}
        if radius == 0:
            assert q["over"] > 0.05   # why the window is part of the rule: per pixel it is unusable
        if radius == 1:               # the caps of the GPU quality test hold on the oracle's frames
            assert q["stopped"] >= 0.25 and q["rendered"] <= 0.80 and q["over"] <= 0.05
