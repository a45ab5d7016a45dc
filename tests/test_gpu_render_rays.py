"""rt_render_rays on the GPU (include/rt_mi355.h): radiance along caller-supplied rays.

The f64 yardstick is the CPU oracle with the zero-delta camera of every ray (tests/render_rays_ref.py; its ray sets are checked
for being worth testing in tests/test_render_rays_host.py), at the project's 1e-12 bar; everything about the shape of a run -
chunks, pool size, replica groups, tail compaction, kernel variants, the number of rays - must leave every bit alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ray_query_cases as rq
import render_rays_ref as rr
import scene_update_cases as su
from rust_raytracer_amd import api
from test_gpu_parity import assert_f64_parity

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTRACE = os.path.join(REPO, "rust_raytracer_amd", "rtrace")
F32 = api.RT_PRECISION_F32


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. f64 against the oracle ----
@pytest.mark.parametrize("name", rr.SCENES)
def test_f64_matches_the_oracle(dev, name):
    """n = 37: the last wave is partial.  smoke: volumes (k_wf_intersect<VOL>), texture_mix: the interpreter form of k_wf_shade."""
    c = rr.case(name)
    scene = api.DeviceScene(c.hs.desc, 0)
    got = scene.render_rays(c.o, c.d, c.params)
    assert got.shape == (c.n, 4)
    err = np.abs(got[:, :3] - c.ref[:, :3])
    print(f"{name}: max abs err {err.max():.3e}, {int((got[:, :3] != c.ref[:, :3]).sum())} of {3 * c.n} values differ in any bit")
    assert_f64_parity(got, c.ref)
    st = scene.stats()
    assert st.samples == c.n * c.t * c.s * c.s and st.pipeline_used == api.RT_PIPELINE_WAVEFRONT
    scene.close()


# ---- 2. independence of the run shape ----
@pytest.mark.parametrize("name", ["cornell", "two_meshes"])
def test_answers_do_not_depend_on_the_shape_of_the_run(dev, name, monkeypatch):
    c = rr.case(name)
    scene = api.DeviceScene(c.hs.desc, 0)
    first = scene.render_rays(c.o, c.d, c.params)
    assert_f64_parity(first, c.ref)
    groups0 = scene.stats().n_replica_groups

    def again(what, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = scene.render_rays(c.o, c.d, c.params)
        st = scene.stats()
        for k in env:
            monkeypatch.delenv(k)
        assert same_bits(got, first), f"{what}: {int((got != first).any(axis=1).sum())} rays differ"
        assert st.samples == c.n * c.t * c.s * c.s
        return st

    again("chunks of 7 rays", RT_RAYS_CHUNK="7")                 # chunk boundaries, global keys
    # 37 * 12 = 444 samples through 256 slots: the rest starts inside k_wf_shade, the table's second reader
    st = again("a pool of 256 slots", RT_WF_POOL="256")
    assert st.n_iterations > 1
    again("a pool of 64 slots, chunks of 5", RT_WF_POOL="64", RT_RAYS_CHUNK="5")
    st = again("one replica per group", RT_WF_SAMPLE_GB="0")
    assert st.n_replica_groups == c.t > groups0
    again("no tail compaction", RT_WF_COMPACT="0")
    again("tail compaction from 8 paths on", RT_WF_COMPACT_MIN="8", RT_WF_POOL="256")
    for lds in ("1", "0"):                                       # the lds forms of k_wf_prims / k_wf_shade
        again(f"RT_LDS_TABLES={lds}", RT_LDS_TABLES=lds)
        again(f"RT_LDS_TABLES={lds}, combined intersect kernel", RT_LDS_TABLES=lds, RT_WF_SPLIT="0")
    again("a staged prefix", RT_LDS_SHADE_PREFIX="1", RT_LDS_BUDGET="4096")
    again("k_wf_prims stand-alone", RT_WF_FUSE="0")
    again("k_wf_prims inside k_wf_shade", RT_WF_FUSE="2")
    # n = 1, and ray i alone at its own index: the rays before it replaced by another ray
    one = scene.render_rays(c.o[:1], c.d[:1], c.params)
    assert same_bits(one, first[:1])
    for i in (1, 17, c.n - 1):
        o, d = np.repeat(c.o[i:i + 1], i + 1, axis=0), np.repeat(c.d[i:i + 1], i + 1, axis=0)
        o[:i], d[:i] = c.o[0], (0.0, 1.0, 0.0)
        got = scene.render_rays(o, d, c.params)
        assert same_bits(got[i], first[i]), f"ray {i} alone"
    # a ray whose value depends on its streams (the oracle's differs under another seed), under another index: other samples
    seeded = (rr.case(name, seed=rr.SEED_B).ref[:, :3] != c.ref[:, :3]).any(axis=1) & (np.arange(c.n) > 0)
    lit = int(np.argmax(seeded))
    assert seeded[lit]
    assert not same_bits(scene.render_rays(c.o[lit:lit + 1], c.d[lit:lit + 1], c.params)[0], first[lit])
    scene.close()


# ---- 3. the camera's own rays ----
@pytest.mark.parametrize("name", ["cornell", "nested_transform"])
def test_the_cameras_own_rays_give_the_frame(dev, name):
    """S = T = 1, no aperture: pixel i's only sample is keyed (seed, 0, i, 0) and sent along get_ray's ray, so the table of those
    rays gives rt_render's frame bit for bit."""
    cs = rq.cases(name)
    hs = cs.hs
    assert hs.camera.has_aperture == 0
    p = rr.params_for(hs, 1, 1, 31)
    scene = api.DeviceScene(hs.desc, 0)
    frame = scene.render(hs.camera, p)
    got = scene.render_rays(cs.cam_o, cs.cam_d, p)
    assert same_bits(got, frame.reshape(-1, 4))
    assert (frame[..., :3] != 0).any()
    scene.close()


# ---- 4. host and device variants, the stream ----
def test_device_variant_equals_the_host_variant(dev):
    import torch
    c = rr.case("cornell")
    scene = api.DeviceScene(c.hs.desc, 0)
    host = scene.render_rays(c.o, c.d, c.params)
    d_o, d_d = torch.from_numpy(c.o).cuda(), torch.from_numpy(c.d).cuda()
    d_out = torch.full((c.n, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    scene.render_rays_device(c.n, d_o.data_ptr(), d_d.data_ptr(), c.params, d_out.data_ptr())
    assert same_bits(d_out.cpu().numpy(), host)
    stream = torch.cuda.Stream()
    d_out.fill_(7.0)
    torch.cuda.synchronize()
    scene.render_rays_device(c.n, d_o.data_ptr(), d_d.data_ptr(), c.params, d_out.data_ptr(), stream=stream.cuda_stream)
    assert same_bits(d_out.cpu().numpy(), host)
    scene.close()


# ---- 5. f32 against the oracle's f64 values ----
@pytest.mark.parametrize("name", ["cornell", "two_meshes"])
def test_f32_is_statistically_equivalent(dev, name):
    """The bar of test_gpu_parity.test_f32_is_statistically_equivalent, on 256 rays x 64 spp."""
    c = rr.case(name, 256, 2, 16)
    p = c.params.copy()
    p.precision = F32
    scene = api.DeviceScene(c.hs.desc, 0)
    got = scene.render_rays(c.o, c.d, p)
    a, b = got[:, :3], c.ref[:, :3]
    close = np.abs(a - b) <= np.maximum(0.05 * np.abs(b), 0.02)
    print(f"{name}: f32 mean {a.mean():.6f}, f64 mean {b.mean():.6f} ({abs(a.mean() - b.mean()) / b.mean():.4%} apart), "
          f"{close.mean():.3%} of values close")
    assert not np.isnan(a).any()
    assert (a != b).any()   # f32 arithmetic cannot give the f64 bits: the f32 kernels ran
    assert abs(a.mean() - b.mean()) <= 0.01 * b.mean()
    assert close.mean() >= 0.95, f"only {close.mean():.3%} of f32 values are close to the f64 oracle"
    assert (got[:, 3] == 0).all()
    scene.close()


# ---- 6. after an update ----
def test_after_an_update_the_answers_are_a_fresh_scenes(dev, tmp_path):
    c = rr.case("two_meshes")
    before = su.two_meshes_variant(tmp_path, "before", numeric=False)
    after = su.two_meshes_variant(tmp_path, "after", numeric=True)
    scene = api.DeviceScene(before.desc, 0)
    old = scene.render_rays(c.o, c.d, c.params)
    scene.update(after.desc)
    got = scene.render_rays(c.o, c.d, c.params)
    fresh_scene = api.DeviceScene(after.desc, 0)
    fresh = fresh_scene.render_rays(c.o, c.d, c.params)
    assert same_bits(got, fresh)
    assert not same_bits(got, old)
    scene.close()
    fresh_scene.close()


# ---- 7. errors ----
def test_errors_name_the_field_and_leave_the_output_alone(dev):
    import torch
    c = rr.case("cornell")
    live0 = api.live_resources()
    scene = api.DeviceScene(c.hs.desc, 0)
    lib, h = scene._lib, scene._h
    n = c.n
    out = np.full((n, 4), 7.0)
    d_o, d_d = torch.from_numpy(c.o).cuda(), torch.from_numpy(c.d).cuda()
    d_out = torch.full((n, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def both(status, field, n_=n, o=True, d=True, res=True, **changes):
        p = c.params.copy()
        for k, v in changes.items():
            setattr(p, k, v)
        st = lib.rt_render_rays(h, n_, c.o.ctypes.data if o else None, c.d.ctypes.data if d else None, C.byref(p), out.ctypes.data if res else None)
        msg = lib.rt_last_error().decode()
        assert st == status and field in msg and "rt_render_rays:" in msg, (st, msg)
        st = lib.rt_render_rays_device(h, n_, C.c_void_p(d_o.data_ptr() if o else None), C.c_void_p(d_d.data_ptr() if d else None), C.byref(p),
                                       C.c_void_p(d_out.data_ptr() if res else None), None)
        msg = lib.rt_last_error().decode()
        assert st == status and field in msg and "rt_render_rays_device:" in msg, (st, msg)
        assert (out == 7.0).all() and bool((d_out == 7.0).all())

    both(api.RT_E_INVALID, "origins", o=False)
    both(api.RT_E_INVALID, "dirs", d=False)
    both(api.RT_E_INVALID, "rgba_out", res=False)
    both(api.RT_E_INVALID, "n must be below 2^31", n_=2 ** 31)
    both(api.RT_E_INVALID, "n must be below 2^31", n_=2 ** 40)
    both(api.RT_E_INVALID, "n_parts", band_rows=1, n_parts=2, part=0)
    both(api.RT_E_INVALID, "precision", precision=2)
    both(api.RT_E_INVALID, "sqrt_spt", sqrt_spt=0)
    both(api.RT_E_INVALID, "thread_count", thread_count=0)
    both(api.RT_E_UNSUPPORTED, "RT_PIPELINE_MEGAKERNEL", pipeline=api.RT_PIPELINE_MEGAKERNEL)
    both(api.RT_E_UNSUPPORTED, "collect_stats", collect_stats=1)
    both(api.RT_E_UNSUPPORTED, "max_depth", max_depth=0)
    with pytest.raises(api.RtError, match="origins"):
        scene.render_rays_device(n, 0, d_d.data_ptr(), c.params, d_out.data_ptr())
    # n = 0 is a no-op, arrays or not; then the call works, with either pipeline value that runs the wavefront scheduler
    p = c.params.copy()
    assert lib.rt_render_rays(h, 0, None, None, C.byref(p), None) == api.RT_OK
    assert scene.render_rays(np.zeros((0, 3)), np.zeros((0, 3)), p).shape == (0, 4)
    assert (out == 7.0).all()
    good = scene.render_rays(c.o, c.d, p)
    p.pipeline = api.RT_PIPELINE_WAVEFRONT
    assert same_bits(scene.render_rays(c.o, c.d, p), good)
    live = api.live_resources()
    assert live[0] > live0[0] and live[1] > live0[1]
    scene.close()
    assert api.live_resources() == live0


# ---- 8. rtrace --probe ----
def test_rtrace_probe(dev, tmp_path):
    """`rtrace scenes/cornell --probe=278,278,278:32 -s=4` (a point in the open middle of the box: outside the tall block, whose
    footprint stays 121 - 117 units away, and the glass ball) writes out_probe.png = the tone-mapped render_rays of
    api.probe_rays, and no out.png."""
    args = [os.path.join(REPO, "scenes", "cornell"), "--probe=278,278,278:32", "-s=4", "--seed=5"]
    r = subprocess.run([RTRACE] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "no pixel filter" in r.stdout
    assert not (tmp_path / "out.png").exists()
    hs = api.HostScene(args)
    assert hs.probe == (32, (278.0, 278.0, 278.0))
    o, d = api.probe_rays(hs.probe[1], 32, 16)
    scene = api.DeviceScene(hs.desc, 0)
    want = scene.render_rays(o, d, hs.params).reshape(16, 32, 4)
    scene.close()
    # row 0 looks up at pi / 32 from the zenith: 277 units below the light, 27 units off its centre, inside its 65 x 52.5 half extents
    assert (want[0, :, :3] == 15.0).all()
    assert len(np.unique(api.tonemap_rgb8(want).reshape(-1, 3), axis=0)) > 16   # and the rest is a picture, not a constant
    api.save_png(str(tmp_path / "want.png"), want)
    assert (tmp_path / "out_probe.png").read_bytes() == (tmp_path / "want.png").read_bytes()
