"""Adaptive sampling (rt_accum_set_adaptive, include/rt_mi355.h) on the GPU.

The contract: without a decision point an adaptive accumulator gives rt_render's frame bit for bit; with decision points
every pixel's sum is, bit for bit, a plain accumulator's sum after n[p] replicas (the prefix property), n[p] is what the
numpy restatement of the rule (tests/adaptive_ref.py) predicts from those sums, and nothing in the state depends on how
the replicas were split into calls, grouped, pooled, compacted or saved and loaded in between."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
from rust_raytracer_amd import api

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTRACE = os.path.join(REPO, "rust_raytracer_amd", "rtrace")
MEGA, WAVE = api.RT_PIPELINE_MEGAKERNEL, api.RT_PIPELINE_WAVEFRONT

# -s=128 -t=8: 8 replicas of 4 x 4 strata
T = 8
SCENES = {
    "cornell": ["scenes/cornell", "-w=32", "-s=128", "-t=8", "--seed=31"],
    "light_test": ["scenes/light_test", "-w=32", "-s=128", "-t=8", "--seed=32"],                # mesh
    "smoke": ["tests/scenes/smoke", "-w=32", "-s=128", "-t=8", "--seed=33"],                    # mesh + volume: combined intersect kernel
    "texture_mix": ["tests/scenes/texture_mix", "-w=32", "-s=128", "-t=8", "--seed=34"],
    "zero_weight_nan": ["tests/scenes/zero_weight_nan", "-w=32", "-s=128", "-t=8", "--seed=35"],  # NaN pixels
}
# (threshold, radius) under which some, not all, pixels stop: mechanics, not quality, so the thresholds are large
CASES = [("cornell", 0.3, 0), ("cornell", 0.3, 1), ("light_test", 0.3, 0), ("light_test", 0.3, 1), ("smoke", 0.15, 0),
         ("smoke", 0.15, 1), ("texture_mix", 0.1, 0), ("texture_mix", 0.1, 1), ("zero_weight_nan", 0.3, 0)]
SPLITS = ([T], [1] * T, [3, 1, 4])


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_same_bits(a, b):
    assert a.shape == b.shape
    diff = bits(a) != bits(b)
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} doubles differ"


def mech(threshold, radius, **over):
    """The parameters of the mechanics tests: min_replicas 2, check_interval 2, floor 0.01."""
    kw = dict(threshold=threshold, radius=radius, min_replicas=2, check_interval=2, floor=0.01)
    kw.update(over)
    return api.RtAdaptiveParams.defaults(**kw)


def parse_v1(blob, h, w):
    assert blob[:8] == b"RTACCUM\0" and struct.unpack_from("<I", blob, 8)[0] == 1 and len(blob) == 48 + h * w * 32
    return np.frombuffer(blob, dtype=np.float64, offset=48).reshape(h, w, 4)


def parse_v2(blob, h, w):
    """Version-2 state: header, 32 bytes of parameters, sum, s1, s2 (f64), n (u32)."""
    np_ = h * w
    assert blob[:8] == b"RTACCUM\0" and struct.unpack_from("<I", blob, 8)[0] == 2
    assert len(blob) == 48 + 32 + np_ * (32 + 8 + 8 + 4)
    thr, floor, mn, ci, rad, zero = struct.unpack_from("<ddIIII", blob, 48)
    assert zero == 0
    off = 80
    total = np.frombuffer(blob, dtype=np.float64, count=np_ * 4, offset=off).reshape(h, w, 4)
    s1 = np.frombuffer(blob, dtype=np.float64, count=np_, offset=off + np_ * 32).reshape(h, w)
    s2 = np.frombuffer(blob, dtype=np.float64, count=np_, offset=off + np_ * 40).reshape(h, w)
    n = np.frombuffer(blob, dtype=np.uint32, count=np_, offset=off + np_ * 48).reshape(h, w)
    return dict(sum=total, s1=s1, s2=s2, n=n, k=struct.unpack_from("<I", blob, 28)[0],
                params=dict(threshold=thr, floor=floor, min_replicas=mn, check_interval=ci, radius=rad))


_snapshots = {}


def snapshots(name, precision=api.RT_PRECISION_F64):
    """sum_k (k = 0 .. T) of the plain accumulator, one replica per call: its version-1 blobs."""
    key = (name, precision)
    if key not in _snapshots:
        hs = api.HostScene(SCENES[name])
        p = hs.params.copy()
        p.precision = precision
        scene = api.DeviceScene(hs.desc, 0)
        pr = api.ProgressiveRender(scene, hs.camera, p)
        snaps = [np.zeros((hs.height, hs.width, 4))]
        for _ in range(T):
            pr.render(1)
            snaps.append(parse_v1(pr.save_state(), hs.height, hs.width).copy())
        pr.close()
        _snapshots[key] = np.stack(snaps)
    return _snapshots[key]


def adaptive_run(name, ap, split, precision=api.RT_PRECISION_F64, reload_after=()):
    """Renders `split` with an adaptive accumulator; after the calls listed in reload_after the state moves to a fresh
    scene and accumulator.  Returns (blob, samples reported per call, n after each call)."""
    hs = api.HostScene(SCENES[name])
    p = hs.params.copy()
    p.precision = precision
    scene = api.DeviceScene(hs.desc, 0)
    pr = api.ProgressiveRender(scene, hs.camera, p, adaptive=ap)
    samples, counts = [], [pr.sample_counts()]
    for i, n in enumerate(split):
        pr.render(n)
        samples.append(scene.stats().samples)
        counts.append(pr.sample_counts())
        if i in reload_after:
            blob = pr.save_state()
            active, done = pr.active_pixels, pr.replicas_done
            pr.close()
            hs = api.HostScene(SCENES[name])
            scene = api.DeviceScene(hs.desc, 0)
            pr = api.ProgressiveRender(scene, hs.camera, p, adaptive=ap)
            pr.load_state(blob)
            assert (pr.active_pixels, pr.replicas_done) == (active, done)
            assert pr.save_state() == blob
    blob = pr.save_state()
    pr.close()
    return blob, samples, counts


# ---- 1. no decision point: the plain frame -------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [api.RT_PRECISION_F64, api.RT_PRECISION_F32])
@pytest.mark.parametrize("name", ["light_test", "zero_weight_nan"])
def test_without_a_decision_point_every_split_is_the_one_shot_frame(dev, name, precision):
    hs = api.HostScene(SCENES[name])
    p = hs.params.copy()
    p.precision = precision
    scene = api.DeviceScene(hs.desc, 0)
    one = scene.render(hs.camera, p)
    for min_replicas in (T, T + 5):
        ap = mech(0.3, 1, min_replicas=min_replicas)
        for split in SPLITS:
            pr = api.ProgressiveRender(scene, hs.camera, p, adaptive=ap)
            for n in split:
                pr.render(n)
                assert pr.active_pixels == (hs.width * hs.height if pr.replicas_done < T else 0)
            assert pr.replicas_done == T and pr.finished
            assert_same_bits(pr.estimate(), one)
            assert (pr.sample_counts() == T).all()
            pr.close()


# ---- 2. + 3. the prefix property and the rule ------------------------------------------------------------------------

@pytest.mark.parametrize("name, threshold, radius", CASES)
def test_prefix_property_and_the_rule(dev, name, threshold, radius):
    snaps = snapshots(name)
    h, w = snaps.shape[1:3]
    ap = mech(threshold, radius)
    blob, _, _ = adaptive_run(name, ap, [T])
    st = parse_v2(blob, h, w)
    assert st["params"] == ar.params_of(ap)
    n = st["n"]
    D = ar.decision_points(T, 2, 2)
    stopped = float((n < T).mean())
    print(f"{name} {threshold} / {radius}: {stopped:.1%} stopped, n histogram {dict(zip(*np.unique(n, return_counts=True)))}")
    assert 0.10 <= stopped <= 0.95, "the case must stop some pixels, not all"
    assert set(np.unique(n)) <= set(D) | {T}
    for k in (2, 4, 8):
        assert (n == k).any(), f"no pixel at n = {k}"
    # prefix property: sum[p] is the plain accumulator's sum after n[p] replicas, bit for bit
    want = np.take_along_axis(snaps, n.astype(np.int64)[None, ..., None].repeat(4, axis=-1), axis=0)[0]
    assert_same_bits(st["sum"], want)
    nan = np.isnan(st["sum"][..., :3]).any(axis=-1)
    assert (n[nan] == T).all(), "a pixel whose sum holds a NaN never stops"
    if name == "zero_weight_nan":
        plain_nan = np.isnan(snaps[T][..., :3]).any(axis=-1)
        escaped = plain_nan & ~nan  # stopped before their first NaN sample: expected, counted
        print(f"zero_weight_nan: {int(plain_nan.sum())} NaN pixels in the plain frame, {int(escaped.sum())} stopped before their first NaN")
        assert plain_nan.sum() > 500 and (n[escaped] < T).all()
    # the rule: n as adaptive_ref predicts from the snapshots
    sim = ar.simulate(ar.contributions_from_snapshots(snaps), **ar.params_of(ap))
    exempt = sim["exempt"]
    print(f"exempt (1e-9 band and their windows): {int(exempt.sum())} of {exempt.size}")
    assert exempt.mean() <= 0.005
    np.testing.assert_array_equal(n[~exempt], sim["n"][~exempt])
    same = n == sim["n"]
    for key in ("s1", "s2"):
        a, b = st[key][same], sim[key][same]
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        fin = ~np.isnan(b)
        np.testing.assert_allclose(a[fin], b[fin], rtol=1e-9, atol=0)


def test_noise_image_counts_and_estimate(dev):
    name, ap = "texture_mix", mech(0.1, 1)
    hs = api.HostScene(SCENES[name])
    scene = api.DeviceScene(hs.desc, 0)
    pr = api.ProgressiveRender(scene, hs.camera, hs.params, adaptive=ap)
    with pytest.raises(api.RtError):
        pr.estimate()  # k = 0
    assert (pr.noise() == 0.0).all() and (pr.sample_counts() == 0).all()
    pr.render(1)
    assert (pr.noise() == 0.0).all()  # n < 2
    pr.render(4)
    st = parse_v2(pr.save_state(), hs.height, hs.width)
    assert st["k"] == 5 and 0 < pr.active_pixels < hs.width * hs.height and not pr.finished
    np.testing.assert_array_equal(pr.sample_counts(), st["n"])
    want = ar.noise(st["s1"], st["s2"], st["n"], ap.floor)
    got = pr.noise()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-9, atol=0)
    # estimate == sum * (T / n), exactly, on a partly stopped frame; previews and denoised previews run on it
    assert_same_bits(pr.estimate(), ar.estimate(st["sum"], st["n"], T))
    est = pr.estimate()
    rgb = pr.preview_rgb8()
    host = api.tonemap_rgb8(est)
    assert rgb.shape == host.shape and np.abs(rgb.astype(int) - host.astype(int)).max() <= 1
    dn = pr.estimate_denoised()
    assert dn.shape == est.shape and not np.array_equal(dn, est)
    assert pr.preview_rgb8_denoised().shape == rgb.shape
    assert_same_bits(pr.estimate(), est)  # the previews leave the state alone
    pr.render(T)
    assert pr.finished and pr.replicas_done == T and pr.active_pixels == 0
    final = parse_v2(pr.save_state(), hs.height, hs.width)
    assert_same_bits(pr.estimate(), ar.estimate(final["sum"], final["n"], T))
    full = final["n"] == T
    assert_same_bits(pr.estimate()[full], final["sum"][full])  # factor exactly 1


# ---- 4. independence ---------------------------------------------------------------------------------------------------

def test_state_does_not_depend_on_splits_reloads_groups_pool_or_compaction(dev, monkeypatch):
    name, ap = "light_test", mech(0.3, 1)
    ref, samples, counts = adaptive_run(name, ap, [T])
    hs = api.HostScene(SCENES[name])
    n = parse_v2(ref, hs.height, hs.width)["n"]
    assert 0.10 <= (n < T).mean() <= 0.95
    assert samples == [16 * int(n.sum())]  # S^2 times the replicas really rendered
    for split in SPLITS[1:] + ([2, 2, 2, 2], [5, 3]):
        blob, samples, counts = adaptive_run(name, ap, split)
        assert blob == ref, split
        for i in range(len(split)):  # stats().samples of each call: what it really rendered
            assert samples[i] == 16 * int((counts[i + 1].astype(np.int64) - counts[i]).sum()), (split, i)
    # save -> new scene and accumulator -> load: at a decision point (k = 2, 4), between two (k = 3), repeatedly
    assert adaptive_run(name, ap, [2, 6], reload_after=(0,))[0] == ref
    assert adaptive_run(name, ap, [3, 5], reload_after=(0,))[0] == ref
    assert adaptive_run(name, ap, [1, 3, 1, 3], reload_after=(0, 1, 2, 3))[0] == ref
    # one replica per group and a pool smaller than a replica
    monkeypatch.setenv("RT_WF_SAMPLE_GB", "0")
    assert adaptive_run(name, ap, [T])[0] == ref
    monkeypatch.setenv("RT_WF_POOL", "3000")
    assert adaptive_run(name, ap, [3, 5])[0] == ref
    monkeypatch.delenv("RT_WF_POOL")
    monkeypatch.delenv("RT_WF_SAMPLE_GB")
    # tail compaction at every chance, and never
    monkeypatch.setenv("RT_WF_COMPACT", "1")
    monkeypatch.setenv("RT_WF_COMPACT_MIN", "1")
    monkeypatch.setenv("RT_WF_COMPACT_PCT", "75")
    assert adaptive_run(name, ap, [T])[0] == ref
    monkeypatch.setenv("RT_WF_COMPACT", "0")
    assert adaptive_run(name, ap, [4, 4])[0] == ref


@pytest.mark.parametrize("name", ["smoke", "texture_mix"])
def test_f32_state_is_independent_and_a_prefix_within_f32(dev, name):
    f32 = api.RT_PRECISION_F32
    ap = mech(0.15 if name == "smoke" else 0.1, 0)
    ref, _, _ = adaptive_run(name, ap, [T], precision=f32)
    for split in SPLITS[1:]:
        assert adaptive_run(name, ap, split, precision=f32)[0] == ref
    assert adaptive_run(name, ap, [3, 5], precision=f32, reload_after=(0,))[0] == ref
    snaps = snapshots(name, f32)
    st = parse_v2(ref, *snaps.shape[1:3])
    assert 0.10 <= (st["n"] < T).mean() <= 0.95
    want = np.take_along_axis(snaps, st["n"].astype(np.int64)[None, ..., None].repeat(4, axis=-1), axis=0)[0]
    assert_same_bits(st["sum"], want)


# ---- 5. a finished accumulator ---------------------------------------------------------------------------------------------

def test_render_on_a_finished_accumulator_is_a_no_op(dev):
    hs = api.HostScene(SCENES["cornell"])
    scene = api.DeviceScene(hs.desc, 0)
    pr = api.ProgressiveRender(scene, hs.camera, hs.params, adaptive=mech(1e6, 0))  # everything is quiet at k = 2
    assert pr.render(T) == 2
    assert pr.finished and pr.active_pixels == 0 and (pr.sample_counts() == 2).all()
    assert scene.stats().samples == hs.width * hs.height * 16 * 2
    blob = pr.save_state()
    assert pr.render(T) == 2 and scene.stats().samples == 0
    assert pr.save_state() == blob
    p2 = hs.params.copy()
    p2.thread_count = 2
    # sum_2 * (8 / 2) is the frame of two replicas: the factors are powers of two, so bit for bit
    assert_same_bits(pr.estimate(), scene.render(hs.camera, p2))
    # a finished state loads as finished
    pr2 = api.ProgressiveRender(scene, hs.camera, hs.params, adaptive=mech(1e6, 0))
    pr2.load_state(blob)
    assert pr2.finished and pr2.active_pixels == 0 and pr2.render(1) == 2 and pr2.save_state() == blob


# ---- 6. refusals -----------------------------------------------------------------------------------------------------

def test_refusals(dev):
    hs = api.HostScene(SCENES["cornell"])
    scene = api.DeviceScene(hs.desc, 0)

    def refused(params, ap, status, words):
        with pytest.raises(api.RtError) as e:
            api.ProgressiveRender(scene, hs.camera, params, adaptive=ap)
        assert e.value.status == status and any(x in str(e.value) for x in words), str(e.value)

    p = hs.params.copy()
    p.band_rows, p.n_parts, p.part = 4, 2, 0
    refused(p, mech(0.3, 1), api.RT_E_INVALID, ["row partition"])
    p = hs.params.copy()
    p.max_depth = 0
    refused(p, mech(0.3, 1), api.RT_E_UNSUPPORTED, ["max_depth"])
    for kw, word in ((dict(threshold=0.0), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(threshold=-1.0), "threshold"),
                     (dict(floor=0.0), "floor"), (dict(min_replicas=1), "min_replicas"), (dict(check_interval=0), "check_interval"),
                     (dict(radius=5), "radius")):
        args = dict(threshold=0.3, radius=1)
        args.update(kw)
        refused(hs.params, mech(**args), api.RT_E_INVALID, [word])
    refused(hs.params, api.RtAdaptiveParams.defaults(), api.RT_E_INVALID, ["threshold"])  # it has no default
    # only before the first replica and before a state is loaded
    plain = api.ProgressiveRender(scene, hs.camera, hs.params)
    plain.render(1)
    v1 = plain.save_state()
    assert struct.unpack_from("<I", v1, 8)[0] == 1 and len(v1) == 48 + hs.width * hs.height * 32  # still version 1
    ap = mech(0.3, 1)
    assert dev.rt_accum_set_adaptive(plain._h, C.byref(ap)) == api.RT_E_INVALID
    fresh = api.ProgressiveRender(scene, hs.camera, hs.params)
    fresh.load_state(v1)  # loads as before
    assert fresh.replicas_done == 1
    assert dev.rt_accum_set_adaptive(fresh._h, C.byref(ap)) == api.RT_E_INVALID
    with pytest.raises(api.RtError):
        fresh.noise()  # a plain accumulator keeps no moments
    assert (fresh.sample_counts() == 1).all() and fresh.active_pixels == hs.width * hs.height and not fresh.finished
    # megakernel / collect_stats on an adaptive accumulator's render: refused, the accumulator unchanged
    pr = api.ProgressiveRender(scene, hs.camera, hs.params, adaptive=ap)
    pr.render(3)
    before = pr.save_state()
    for kw, word in ((dict(pipeline=MEGA), "MEGAKERNEL"), (dict(collect_stats=True), "collect_stats")):
        with pytest.raises(api.RtError) as e:
            pr.render(1, **kw)
        assert e.value.status == api.RT_E_UNSUPPORTED and word in str(e.value), str(e.value)
        assert pr.replicas_done == 3 and pr.save_state() == before
    # blobs of the other kind, and other parameters, are refused
    for target, data, word in ((pr, v1, "version"), (fresh, before, "version"),
                               (api.ProgressiveRender(scene, hs.camera, hs.params, adaptive=mech(0.3, 0)), before, "adaptive parameter"),
                               (pr, before[:-4], "truncated")):
        k, state = target.replicas_done, target.save_state()
        with pytest.raises(api.RtError) as e:
            target.load_state(data)
        assert e.value.status == api.RT_E_INVALID and word in str(e.value), str(e.value)
        assert target.replicas_done == k and target.save_state() == state
    pr.load_state(before)
    pr.render(T)
    assert pr.finished


# ---- 7. quality ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [["scenes/light_test", "-w=48", "-s=128", "-t=32", "--seed=42"],
                                  ["tests/scenes/texture_mix", "-w=48", "-s=128", "-t=32", "--seed=43"]])
def test_quality_at_the_defaults(dev, args):
    threshold = 0.1
    hs = api.HostScene(args)
    assert hs.params.thread_count == 32
    scene = api.DeviceScene(hs.desc, 0)
    full = scene.render(hs.camera, hs.params)
    pr = api.ProgressiveRender(scene, hs.camera, hs.params, adaptive=api.RtAdaptiveParams.defaults(threshold=threshold))
    while not pr.finished:
        pr.render(5)
    n = pr.sample_counts()
    q = ar.quality(pr.estimate(), full, n, 32, threshold)
    print(args[0], q)
    assert q["stopped"] >= 0.25 and q["rendered"] <= 0.80 and q["over"] <= 0.05


# ---- 8. rtrace ---------------------------------------------------------------------------------------------------------

def run_rtrace(args, cwd):
    return subprocess.run([RTRACE] + args, cwd=cwd, capture_output=True, text=True, timeout=600)


def test_rtrace_noise_threshold_end_to_end(dev, tmp_path):
    args = [os.path.join(REPO, "scenes", "light_test"), "-w=40", "-s=128", "-t=8", "--seed=41"]
    flags = ["--noise-threshold=0.3", "--adaptive-min=2", "--adaptive-check=2", "--adaptive-radius=1"]
    for sub in ("plain", "adapt", "ckpt", "dn"):
        (tmp_path / sub).mkdir()
    r = run_rtrace(args, str(tmp_path / "plain"))
    assert r.returncode == 0, r.stderr
    assert "Adaptive" not in r.stdout and not (tmp_path / "plain" / "out_samples.png").exists()
    r = run_rtrace(args + flags, str(tmp_path / "adapt"))
    assert r.returncode == 0, r.stderr
    assert "Pass 1: 2/8 replicas in" in r.stdout  # passes of check_interval replicas
    line = [x for x in r.stdout.splitlines() if x.startswith("Adaptive: ")]
    assert len(line) == 1, r.stdout
    rendered, total, stopped, pixels = [int(x) for x in line[0].replace("/", " ").split() if x.isdigit()]
    h = api.HostScene(args).height
    assert pixels == 40 * h and total == pixels * 128 and 0 < stopped < pixels and pixels * 32 <= rendered < total
    out = (tmp_path / "adapt" / "out.png").read_bytes()
    assert out != (tmp_path / "plain" / "out.png").read_bytes()
    samples_png = (tmp_path / "adapt" / "out_samples.png").read_bytes()
    grey = api.load_image(str(tmp_path / "adapt" / "out_samples.png"))
    assert grey.shape[:2] == (h, 40) and len(np.unique(grey[..., 0])) > 1
    # stopped by the clock after the first pass, resumed by a new process: the same files
    ck = str(tmp_path / "ckpt" / "state.bin")
    r = run_rtrace(args + flags + ["--checkpoint=" + ck, "--time-limit=0"], str(tmp_path / "ckpt"))
    assert r.returncode == 0, r.stderr
    assert "Pass 1: 2/8" in r.stdout and "Pass 2" not in r.stdout and "Stopped at 2/8 replicas" in r.stdout
    assert struct.unpack_from("<I", open(ck, "rb").read(), 8)[0] == 2
    r = run_rtrace(args + flags + ["--checkpoint=" + ck], str(tmp_path / "ckpt"))
    assert r.returncode == 0, r.stderr
    assert "Resumed" in r.stdout and line[0] in r.stdout
    assert (tmp_path / "ckpt" / "out.png").read_bytes() == out
    assert (tmp_path / "ckpt" / "out_samples.png").read_bytes() == samples_png
    # a larger pass size and the denoiser: the same frame again
    r = run_rtrace(args + flags + ["--progressive=3", "--denoise=2"], str(tmp_path / "dn"))
    assert r.returncode == 0, r.stderr
    assert "Pass 1: 3/8" in r.stdout and line[0] in r.stdout
    assert (tmp_path / "dn" / "out.png").read_bytes() == out and (tmp_path / "dn" / "out_denoised.png").exists()
