"""Progressive, resumable rendering (rt_accum_*, include/rt_mi355.h) on the GPU.

The frame is the ordered sum of per-replica means and every random stream is keyed by (seed, replica, pixel, stratum),
so the replicas [0, T) rendered in any number of calls must give the one-shot frame BIT FOR BIT (compared as uint64 so
NaN pixels count too): every split, both pipelines, replica groups, tail compaction, f32, a row partition.  The estimate
at k < T is the frame rendered with thread_count = k, at the oracle bar of test_gpu_parity.  States move between
processes and are refused when they belong to another frame."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle
from rust_raytracer_amd import api

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTRACE = os.path.join(REPO, "rust_raytracer_amd", "rtrace")
MEGA, WAVE = api.RT_PIPELINE_MEGAKERNEL, api.RT_PIPELINE_WAVEFRONT

# -s=80 -t=5: 5 replicas of 4 x 4 strata
SCENES = {
    "cornell": ["scenes/cornell", "-w=32", "-s=80", "-t=5", "--seed=31"],
    "light_test": ["scenes/light_test", "-w=40", "-s=80", "-t=5", "--seed=32"],                # mesh
    "smoke": ["tests/scenes/smoke", "-w=32", "-s=80", "-t=5", "--seed=33"],                    # mesh + volume: combined intersect kernel
    "zero_weight_nan": ["tests/scenes/zero_weight_nan", "-w=32", "-s=80", "-t=5", "--seed=34"],  # NaN pixels
    "texture_mix": ["tests/scenes/texture_mix", "-w=32", "-s=80", "-t=5", "--seed=35"],
}
T = 5
SPLITS = ([T], [1] * T, [1, T - 3, 2])


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


def progressive(scene, hs, p, split, pipelines=None):
    pr = api.ProgressiveRender(scene, hs.camera, p)
    for i, n in enumerate(split):
        pr.render(n, pipeline=None if pipelines is None else pipelines[i])
    assert pr.replicas_done == p.thread_count
    out = pr.estimate()
    pr.close()
    return out


def with_pipeline(params, pipeline):
    p = params.copy()
    p.pipeline = pipeline
    return p


@pytest.mark.parametrize("pipeline", ["mega", "wavefront"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_split_is_the_one_shot_frame(dev, name, pipeline):
    hs = api.HostScene(SCENES[name])
    assert hs.params.thread_count == T
    scene = api.DeviceScene(hs.desc, 0)
    p = with_pipeline(hs.params, MEGA if pipeline == "mega" else WAVE)
    one = scene.render(hs.camera, p)
    if name == "zero_weight_nan":
        assert np.isnan(one[..., :3]).any()
    for split in SPLITS:
        assert_same_bits(progressive(scene, hs, p, split), one)


def test_forced_groups_compaction_and_pipeline_switch(dev, monkeypatch):
    hs = api.HostScene(SCENES["light_test"])
    scene = api.DeviceScene(hs.desc, 0)
    one = scene.render(hs.camera, with_pipeline(hs.params, WAVE))
    # mega -> wavefront in the middle of the frame, and back
    assert_same_bits(progressive(scene, hs, hs.params, [2, 3], [MEGA, WAVE]), one)
    assert_same_bits(progressive(scene, hs, hs.params, [1, 3, 1], [WAVE, MEGA, WAVE]), one)
    # one replica per group and a pool smaller than a replica (as test_replica_groups_forced)
    monkeypatch.setenv("RT_WF_SAMPLE_GB", "0")
    monkeypatch.setenv("RT_WF_POOL", "3000")
    p = with_pipeline(hs.params, WAVE)
    pr = api.ProgressiveRender(scene, hs.camera, p)
    for n in (1, 3, 1):
        pr.render(n)
        assert scene.stats().n_replica_groups == n
    assert_same_bits(pr.estimate(), one)
    monkeypatch.delenv("RT_WF_POOL")
    monkeypatch.delenv("RT_WF_SAMPLE_GB")
    # tail compaction at every chance
    monkeypatch.setenv("RT_WF_COMPACT", "1")
    monkeypatch.setenv("RT_WF_COMPACT_MIN", "1")
    monkeypatch.setenv("RT_WF_COMPACT_PCT", "75")
    pr = api.ProgressiveRender(scene, hs.camera, p)
    compactions = 0
    for n in (2, 1, 2):
        pr.render(n)
        compactions += scene.stats().n_tail_compactions
    assert compactions > 0
    assert_same_bits(pr.estimate(), one)


@pytest.mark.parametrize("pipeline", ["mega", "wavefront"])
def test_f32_matches_f32_one_shot(dev, pipeline):
    hs = api.HostScene(SCENES["light_test"])
    scene = api.DeviceScene(hs.desc, 0)
    p = with_pipeline(hs.params, MEGA if pipeline == "mega" else WAVE)
    p.precision = api.RT_PRECISION_F32
    one = scene.render(hs.camera, p)
    assert_same_bits(progressive(scene, hs, p, [1, T - 3, 2]), one)


def test_banded_partition_part(dev):
    hs = api.HostScene(SCENES["cornell"])
    scene = api.DeviceScene(hs.desc, 0)
    p = hs.params.copy()
    p.band_rows, p.n_parts, p.part = 4, 3, 0
    full = scene.render(hs.camera, hs.params)
    for pipeline in (MEGA, WAVE):
        q = with_pipeline(p, pipeline)
        part = progressive(scene, hs, q, [2, 3])
        assert_same_bits(part, scene.render(hs.camera, q))
        assert_same_bits(part, full[api.owned_rows(hs.height, p)])


def assert_f64_parity(gpu, ref):  # the bar of tests/test_gpu_parity.py
    a, b = gpu[..., :3], ref[..., :3]
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    fin = ~np.isnan(b)
    err = np.abs(a[fin] - b[fin])
    bad = err > np.maximum(1e-12 * np.abs(b[fin]), 1e-15)
    assert not bad.any(), f"{bad.mean():.4%} of values differ by more than 1e-12 relative (max abs err {err.max():.3e})"
    assert np.all(gpu[..., 3] == 0.0)


@pytest.mark.parametrize("name", ["cornell", "zero_weight_nan"])
def test_estimate_is_the_frame_of_k_replicas(dev, name):
    hs = api.HostScene(SCENES[name])
    scene = api.DeviceScene(hs.desc, 0)
    pr = api.ProgressiveRender(scene, hs.camera, hs.params)
    with pytest.raises(api.RtError):
        pr.estimate()  # k = 0: no estimate
    for k in (1, 3):
        pr.render(k - pr.replicas_done)
        p = hs.params.copy()
        p.thread_count = k
        ref, _ = pyoracle.render(hs.desc, hs.camera, p)
        assert_f64_parity(pr.estimate(), ref)
    pr.render(T)
    assert_same_bits(pr.estimate(), scene.render(hs.camera, hs.params))


def test_state_resumes_in_a_fresh_scene(dev):
    hs = api.HostScene(SCENES["light_test"])
    scene = api.DeviceScene(hs.desc, 0)
    one = scene.render(hs.camera, hs.params)
    pr = api.ProgressiveRender(scene, hs.camera, hs.params)
    pr.render(2)
    blob = pr.save_state()
    assert len(blob) == 48 + hs.height * hs.width * 32 and blob[:8] == b"RTACCUM\0"
    hs2 = api.HostScene(SCENES["light_test"])
    scene2 = api.DeviceScene(hs2.desc, 0)
    pr2 = api.ProgressiveRender(scene2, hs2.camera, hs2.params)
    pr2.load_state(blob)
    assert pr2.replicas_done == 2
    pr2.render(1, pipeline=MEGA)
    pr2.render(10, pipeline=WAVE)
    assert_same_bits(pr2.estimate(), one)


def test_state_mismatches_are_refused(dev):
    hs = api.HostScene(SCENES["cornell"])
    scene = api.DeviceScene(hs.desc, 0)
    pr = api.ProgressiveRender(scene, hs.camera, hs.params)
    pr.render(2)
    blob = pr.save_state()

    def refused(target_scene, camera, params, data, words):
        t = api.ProgressiveRender(target_scene, camera, params)
        t.render(1)
        before = bits(t.estimate()).copy()
        with pytest.raises(api.RtError) as e:
            t.load_state(data)
        assert e.value.status == api.RT_E_INVALID
        assert any(w in str(e.value) for w in words), str(e.value)
        assert t.replicas_done == 1
        np.testing.assert_array_equal(bits(t.estimate()), before)

    p = hs.params.copy()
    p.seed += 1
    refused(scene, hs.camera, p, blob, ["parameter"])
    cam = api.RtCameraDesc()
    C.memmove(C.byref(cam), C.byref(hs.camera), C.sizeof(cam))
    cam.position[0] += 0.25
    refused(scene, cam, hs.params, blob, ["camera"])
    p = hs.params.copy()
    p.thread_count = T + 1
    refused(scene, hs.camera, p, blob, ["thread_count"])
    p = hs.params.copy()
    p.precision = api.RT_PRECISION_F32
    refused(scene, hs.camera, p, blob, ["precision"])
    other = api.HostScene(["scenes/light_test", "-w=32", "-s=80", "-t=5", "--seed=31"])
    refused(api.DeviceScene(other.desc, 0), hs.camera, hs.params, blob, ["scene"])
    refused(scene, hs.camera, hs.params, blob[:-8], ["truncated"])
    refused(scene, hs.camera, hs.params, blob[:20], ["truncated"])
    refused(scene, hs.camera, hs.params, b"X" + blob[1:], ["magic"])
    # and the untouched blob still loads
    t = api.ProgressiveRender(scene, hs.camera, hs.params)
    t.load_state(blob)
    assert t.replicas_done == 2


def test_isolation_clamping_tail_flag_and_stats(dev, monkeypatch):
    monkeypatch.setenv("RT_WF_SAMPLE_GB", "0")  # the scene's scratch (w.acc, sample_L) is in use by every render
    hs = api.HostScene(SCENES["light_test"])
    scene = api.DeviceScene(hs.desc, 0)
    p = with_pipeline(hs.params, WAVE)
    one = scene.render(hs.camera, p)
    other = hs.params.copy()
    other.seed += 7
    other.thread_count = 3
    flag = C.c_int32(0)
    dev.rt_scene_set_tail_flag(scene._h, C.addressof(flag))
    try:
        pr = api.ProgressiveRender(scene, hs.camera, p)
        assert pr.render(0) == 0
        assert flag.value == 1
        flag.value = 0
        pr.render(2)
        assert flag.value == 1
        npix = hs.width * hs.height
        st = scene.stats()
        assert st.samples == npix * 16 * 2 and st.n_replica_groups == 2
        for q in (with_pipeline(other, WAVE), with_pipeline(other, MEGA)):
            scene.render(hs.camera, q)  # frames of another seed through the same scene in between
        flag.value = 0
        assert pr.render(1, pipeline=MEGA) == 3
        assert flag.value == 1
        assert scene.stats().samples == npix * 16
        scene.render(hs.camera, with_pipeline(other, WAVE))
        assert pr.render(100) == T  # clamped to T - k
        assert scene.stats().samples == npix * 16 * 2
        assert pr.render(100) == T
        assert_same_bits(pr.estimate(), one)
        with pytest.raises(api.RtError):  # params may change pipeline and collect_stats only
            q = p.copy()
            q.max_depth += 1
            pr._check(dev.rt_accum_render(pr._h, 1, C.byref(q), None))
    finally:
        dev.rt_scene_set_tail_flag(scene._h, None)


def host_near_integer(rgba):
    """Channels where the host's x * 255.999 before truncation lies within 1e-9 of an integer in (0, 255): only
    there may the last bit of pow decide the byte."""
    kin = np.array([[0.59719, 0.35458, 0.04823], [0.07600, 0.90834, 0.01566], [0.02840, 0.13383, 0.83777]])
    kout = np.array([[1.60475, -0.53108, -0.07367], [-0.10208, 1.10813, -0.00605], [-0.00327, -0.07276, 1.07602]])
    p = rgba.reshape(-1, 4)
    with np.errstate(all="ignore"):
        c = [kin[r, 0] * p[:, 0] + kin[r, 1] * p[:, 1] + kin[r, 2] * p[:, 2] + 0.0 * p[:, 3] for r in range(3)]
        f = [(x * (x + 0.0245786) - 0.000090537) / (x * (x * 0.983729 + 0.4329510) + 0.238081) for x in c]
        near = []
        for r in range(3):
            o = kout[r, 0] * f[0] + kout[r, 1] * f[1] + kout[r, 2] * f[2] + 0.0 * 0.0
            x = np.where(o < 0.0, 0.0, np.where(o > 1.0, 1.0, o))
            s = np.where(x < 0.0031308, x * 12.92, np.power(x, 1.0 / 2.4) * 1.055 - 0.055)
            q = s * 255.999
            near.append((q > 0) & (q < 255) & (np.abs(q - np.round(q)) < 1e-9))
    return np.stack(near, axis=1).reshape(rgba.shape[:-1] + (3,))


DEVICE_TONEMAP_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.init()  # torch's runtime first, as bench.py does
rgba = np.load(sys.argv[1])
d_in = torch.from_numpy(rgba).to("cuda:0")
d_out = torch.zeros(rgba.shape[:2] + (3,), dtype=torch.uint8, device="cuda:0")
torch.cuda.synchronize()
sys.path.insert(0, sys.argv[3])
from rust_raytracer_amd import api
api.tonemap_rgb8_device(d_in.data_ptr(), rgba.shape[1], rgba.shape[0], d_out.data_ptr(), device=0)
np.save(sys.argv[2], d_out.cpu().numpy())
"""


def device_tonemap(rgba, tmp_path):
    """rt_tonemap_rgb8_device on device buffers (torch allocates them, in a process of its own)."""
    src, dst = str(tmp_path / "rgba.npy"), str(tmp_path / "rgb.npy")
    np.save(src, np.ascontiguousarray(rgba))
    r = subprocess.run([sys.executable, "-c", DEVICE_TONEMAP_CHILD, src, dst, REPO], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(dst)


def preview_of_frame(scene, hs, rgba):
    """rt_accum_preview_rgb8 of an arbitrary frame: a state blob of a finished accumulator (k = T, factor 1) with `rgba`
    as its sums."""
    pr = api.ProgressiveRender(scene, hs.camera, hs.params)
    pr.render(hs.params.thread_count)
    blob = pr.save_state()
    assert rgba.shape == (hs.height, hs.width, 4)
    pr.load_state(blob[:48] + np.ascontiguousarray(rgba, dtype=np.float64).tobytes())
    return pr.preview_rgb8()


def assert_tonemap_equal(dev_bytes, rgba):
    host = api.tonemap_rgb8(rgba)
    near = host_near_integer(rgba)
    diff = (dev_bytes != host) & ~near
    assert not diff.any(), f"{int(diff.sum())} channels differ from the host output stage ({int(near.sum())} near an integer)"


def test_device_tonemap_matches_host(dev, tmp_path):
    hs = api.HostScene(["scenes/cornell", "-w=64", "-r=1.3333333333333333", "-s=2", "-t=2", "--max-depth=2", "--seed=36"])
    h, w = hs.height, hs.width
    rng = np.random.default_rng(5)
    special = np.array([np.nan, np.inf, -np.inf, -1.0, -1e-3, 0.0, 1e-6, 1.0, 1e6, 0.5, 2.0, 0.25])
    knee = np.geomspace(1e-4, 2e-2, 400)  # the ACES output crosses the 0.0031308 knee in here
    vals = np.concatenate([special, knee, rng.uniform(0, 4, 2000), rng.exponential(0.3, 2000)])
    rgba = np.zeros((h, w, 4))
    rgba[..., :3] = rng.choice(vals, size=(h, w, 3))
    rgba[0, :len(special), :3] = special[:, None]           # every special value on every channel at once
    rgba[1, :64, :3] = knee[::6][:64, None]                   # grey ramp across the knee
    scene = api.DeviceScene(hs.desc, 0)
    assert_tonemap_equal(preview_of_frame(scene, hs, rgba), rgba)
    assert_tonemap_equal(device_tonemap(rgba, tmp_path), rgba)
    # rendered estimates through rt_accum_preview_rgb8 (the estimate is formed inside the tonemap kernel)
    hs = api.HostScene(SCENES["zero_weight_nan"])
    scene = api.DeviceScene(hs.desc, 0)
    pr = api.ProgressiveRender(scene, hs.camera, hs.params)
    for n in (2, 3):
        pr.render(n)
        est = pr.estimate()
        assert_tonemap_equal(pr.preview_rgb8(), est)
    assert_tonemap_equal(device_tonemap(est, tmp_path), est)


def run_rtrace(args, cwd):
    return subprocess.run([RTRACE] + args, cwd=cwd, capture_output=True, text=True, timeout=600)


def test_rtrace_progressive_checkpoint_resume(dev, tmp_path):
    args = [os.path.join(REPO, "scenes", "light_test"), "-w=40", "-s=80", "-t=5", "--seed=41"]
    for sub in ("plain", "prog", "ckpt", "seed"):
        (tmp_path / sub).mkdir()
    r = run_rtrace(args, str(tmp_path / "plain"))
    assert r.returncode == 0, r.stderr
    plain = (tmp_path / "plain" / "out.png").read_bytes()
    r = run_rtrace(args + ["--progressive=3"], str(tmp_path / "prog"))
    assert r.returncode == 0, r.stderr
    assert "Pass 1: 3/5 replicas in" in r.stdout and "Pass 2: 5/5 replicas in" in r.stdout
    assert (tmp_path / "prog" / "out.png").read_bytes() == plain
    ck = str(tmp_path / "ckpt" / "state.bin")
    r = run_rtrace(args + ["--progressive=3", "--checkpoint=" + ck, "--time-limit=0"], str(tmp_path / "ckpt"))
    assert r.returncode == 0, r.stderr
    assert "Pass 1: 3/5" in r.stdout and "Pass 2" not in r.stdout and "Stopped at 3/5 replicas" in r.stdout
    assert os.path.exists(ck) and not os.path.exists(ck + ".tmp")
    assert (tmp_path / "ckpt" / "out.png").read_bytes() != plain  # the preview of 3 replicas
    r = run_rtrace(args + ["--progressive=3", "--checkpoint=" + ck], str(tmp_path / "ckpt"))  # a new process
    assert r.returncode == 0, r.stderr
    assert "Resumed" in r.stdout and "Pass 1: 5/5" in r.stdout
    assert (tmp_path / "ckpt" / "out.png").read_bytes() == plain
    other = [a if not a.startswith("--seed=") else "--seed=42" for a in args]
    r = run_rtrace(other + ["--progressive=3", "--checkpoint=" + ck], str(tmp_path / "seed"))
    assert r.returncode == 1
    assert "mismatch" in r.stderr and "state.bin" in r.stderr
    assert not (tmp_path / "seed" / "out.png").exists()
