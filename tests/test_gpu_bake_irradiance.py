"""rt_bake_irradiance on the GPU (include/rt_mi355.h): path-traced, cosine-weighted radiance at surface points.

The f64 yardstick is the CPU oracle sample by sample (tests/bake_irradiance_ref.py: the direction restated in numpy, the
reference's camera returning it, pyoracle.trace_sample; its point sets are checked for being worth testing in
tests/test_bake_irradiance_host.py), at the project's 1e-12 bar; everything about the shape of a run - chunks, pool size,
replica groups, tail compaction, kernel variants, the number of points - must leave every bit alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bake_irradiance_ref as br
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
@pytest.mark.parametrize("name", br.SCENES)
def test_f64_matches_the_oracle(dev, name):
    """n = 37: the last wave is partial.  smoke: volumes (k_wf_intersect<VOL>), texture_mix: the interpreter form of k_wf_shade."""
    c = br.case(name)
    scene = api.DeviceScene(c.hs.desc, 0)
    got = scene.bake_irradiance(c.pos, c.nrm, c.params)
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
    c = br.case(name)
    scene = api.DeviceScene(c.hs.desc, 0)
    first = scene.bake_irradiance(c.pos, c.nrm, c.params)
    assert_f64_parity(first, c.ref)
    groups0 = scene.stats().n_replica_groups

    def again(what, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = scene.bake_irradiance(c.pos, c.nrm, c.params)
        st = scene.stats()
        for k in env:
            monkeypatch.delenv(k)
        assert same_bits(got, first), f"{what}: {int((got != first).any(axis=1).sum())} points differ"
        assert st.samples == c.n * c.t * c.s * c.s
        return st

    again("chunks of 7 points", RT_RAYS_CHUNK="7")               # chunk boundaries, global keys
    # 37 * 12 = 444 samples through 256 slots: the rest starts inside k_wf_shade, the points' second reader
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
    again("k_wf_prims stand-alone", RT_WF_FUSE="0")
    again("k_wf_prims inside k_wf_shade", RT_WF_FUSE="2")
    again("k_wf_prims inside k_wf_shade, restarts there", RT_WF_FUSE="2", RT_WF_POOL="256")
    # n = 1, and point i alone at its own index: the points before it replaced by another point
    one = scene.bake_irradiance(c.pos[:1], c.nrm[:1], c.params)
    assert same_bits(one, first[:1])
    for i in (1, 17, c.n - 1):
        p, nr = np.repeat(c.pos[i:i + 1], i + 1, axis=0), np.repeat(c.nrm[i:i + 1], i + 1, axis=0)
        p[:i], nr[:i] = c.pos[0], (0.0, 1.0, 0.0)
        got = scene.bake_irradiance(p, nr, c.params)
        assert same_bits(got[i], first[i]), f"point {i} alone"
    # a point whose value depends on its streams (the oracle's differs under another seed), under another index: other samples
    seeded = (br.case(name, seed=br.SEED_B).ref[:, :3] != c.ref[:, :3]).any(axis=1) & (np.arange(c.n) > 0)
    lit = int(np.argmax(seeded))
    assert seeded[lit]
    assert not same_bits(scene.bake_irradiance(c.pos[lit:lit + 1], c.nrm[lit:lit + 1], c.params)[0], first[lit])
    scene.close()


# ---- 3. cross-check without the oracle ----
@pytest.mark.parametrize("name", ["cornell", "smoke"])
def test_one_sample_per_point_equals_render_rays_along_the_restated_ray(dev, name):
    """S = T = 1: point i's only sample is keyed (seed, 0, i, 0) on both sides; rt_render_rays drops the two draws the bake forms
    its direction from, so along d' = (o + d) - o restated in numpy it must give the bake's bits.  n = 1 000: several waves."""
    n = 1000
    pos, nrm = br.point_set(name, n)   # the walk wraps round: a hit comes back under other indices, i.e. with other directions
    hs = rq.cases(name).hs
    p = rr.params_for(hs, 1, 1, br.SEED)
    rays = br.first_rays(pos, nrm, 1, 1, br.SEED)
    scene = api.DeviceScene(hs.desc, 0)
    baked = scene.bake_irradiance(pos, nrm, p)
    along = scene.render_rays(np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:]), p)
    assert same_bits(rays[:, :3], pos)
    assert same_bits(baked, along), f"{int((baked != along).any(axis=1).sum())} of {n} points differ"
    # one path per point: how many find light is the scene's business; the comparison must only not be one of zeros with zeros
    lit = baked[(baked[:, :3] != 0).any(axis=1)]
    print(f"{name}: {len(lit)} of {n} points carry radiance")
    assert np.isfinite(baked).all() and len(lit) > 0 and len({r.tobytes() for r in lit}) > 1
    scene.close()


# ---- 4. variants ----
def test_device_variant_equals_the_host_variant(dev):
    import torch
    c = br.case("cornell")
    scene = api.DeviceScene(c.hs.desc, 0)
    host = scene.bake_irradiance(c.pos, c.nrm, c.params)
    d_p, d_n = torch.from_numpy(c.pos).cuda(), torch.from_numpy(c.nrm).cuda()
    d_out = torch.full((c.n, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    scene.bake_irradiance_device(c.n, d_p.data_ptr(), d_n.data_ptr(), c.params, d_out.data_ptr())
    assert same_bits(d_out.cpu().numpy(), host)
    stream = torch.cuda.Stream()
    d_out.fill_(7.0)
    torch.cuda.synchronize()
    scene.bake_irradiance_device(c.n, d_p.data_ptr(), d_n.data_ptr(), c.params, d_out.data_ptr(), stream=stream.cuda_stream)
    assert same_bits(d_out.cpu().numpy(), host)
    # a single normal, and a single position, broadcast
    up = scene.bake_irradiance(c.pos, c.nrm[0], c.params)
    assert same_bits(up, scene.bake_irradiance(c.pos, np.repeat(c.nrm[:1], c.n, axis=0), c.params))
    assert scene.bake_irradiance(c.pos[0], c.nrm, c.params).shape == (c.n, 4)
    scene.close()


@pytest.mark.parametrize("name", ["two_meshes", "sun_sky"])
def test_hits_variant(dev, name, monkeypatch):
    """The records of trace_rays on the camera's rays: surface records give what the array variant gives for their pos and normal
    under the same index; misses (two_meshes) and environment hits (sun_sky) give (0, 0, 0, 0) exactly."""
    import torch
    cs = rq.cases(name)
    n = len(cs.cam_o)
    p = rr.params_for(cs.hs, 2, 2, br.SEED)
    scene = api.DeviceScene(cs.hs.desc, 0)
    d_o, d_d = torch.from_numpy(cs.cam_o).cuda(), torch.from_numpy(cs.cam_d).cuda()
    d_hits = torch.zeros(n * api.RtRayHit.itemsize, dtype=torch.uint8, device="cuda")
    d_out = torch.full((n, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    scene.trace_rays_device(n, d_o.data_ptr(), d_d.data_ptr(), d_hits.data_ptr())
    scene.bake_irradiance_hits_device(n, d_hits.data_ptr(), p, d_out.data_ptr())
    got = d_out.cpu().numpy()
    hits = d_hits.cpu().numpy().view(api.RtRayHit)
    surface = rq.klass_of(hits) == rq.SURFACE
    assert surface.any() and (~surface).any()
    if name == "sun_sky":
        assert (rq.klass_of(hits) == rq.ENVIRONMENT).any()
    assert (got[~surface] == 0.0).all() and not np.signbit(got[~surface]).any()
    arrays = scene.bake_irradiance(np.ascontiguousarray(hits["pos"]), np.ascontiguousarray(hits["normal"]), p)
    assert same_bits(got[surface], arrays[surface])
    assert np.isfinite(got).all() and (got[surface][:, :3] != 0).any()
    assert scene.stats().samples == n * 4 * 2
    monkeypatch.setenv("RT_RAYS_CHUNK", "100")   # chunks: the records, the flags and the output move together
    d_out.fill_(7.0)
    torch.cuda.synchronize()
    scene.bake_irradiance_hits_device(n, d_hits.data_ptr(), p, d_out.data_ptr())
    assert same_bits(d_out.cpu().numpy(), got)
    scene.close()


# ---- 5. after an update ----
def test_after_an_update_the_answers_are_a_fresh_scenes(dev, tmp_path):
    c = br.case("two_meshes")
    before = su.two_meshes_variant(tmp_path, "before", numeric=False)
    after = su.two_meshes_variant(tmp_path, "after", numeric=True)
    scene = api.DeviceScene(before.desc, 0)
    old = scene.bake_irradiance(c.pos, c.nrm, c.params)
    scene.update(after.desc)
    got = scene.bake_irradiance(c.pos, c.nrm, c.params)
    fresh_scene = api.DeviceScene(after.desc, 0)
    fresh = fresh_scene.bake_irradiance(c.pos, c.nrm, c.params)
    assert same_bits(got, fresh)
    assert not same_bits(got, old)
    scene.close()
    fresh_scene.close()


# ---- 6. no side effects ----
def test_a_bake_leaves_the_scene_and_refusals_leave_the_output(dev):
    import torch
    c = br.case("cornell")
    live0 = api.live_resources()
    scene = api.DeviceScene(c.hs.desc, 0)
    lib, h = scene._lib, scene._h
    frame_params = rr.params_for(c.hs, 2, 2, 5)
    frame = scene.render(c.hs.camera, frame_params)
    good = scene.bake_irradiance(c.pos, c.nrm, c.params)
    assert same_bits(scene.render(c.hs.camera, frame_params), frame)
    n = c.n
    out = np.full((n, 4), 7.0)
    d_p, d_n = torch.from_numpy(c.pos).cuda(), torch.from_numpy(c.nrm).cuda()
    d_hits = torch.zeros(n * api.RtRayHit.itemsize, dtype=torch.uint8, device="cuda")
    d_out = torch.full((n, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def all_three(status, field, n_=n, pos=True, nrm=True, res=True, **changes):
        p = c.params.copy()
        for k, v in changes.items():
            setattr(p, k, v)
        st = lib.rt_bake_irradiance(h, n_, c.pos.ctypes.data if pos else None, c.nrm.ctypes.data if nrm else None, C.byref(p),
                                    out.ctypes.data if res else None)
        msg = lib.rt_last_error().decode()
        assert st == status and field in msg and "rt_bake_irradiance:" in msg, (st, msg)
        st = lib.rt_bake_irradiance_device(h, n_, C.c_void_p(d_p.data_ptr() if pos else None), C.c_void_p(d_n.data_ptr() if nrm else None),
                                           C.byref(p), C.c_void_p(d_out.data_ptr() if res else None), None)
        msg = lib.rt_last_error().decode()
        assert st == status and field in msg and "rt_bake_irradiance_device:" in msg, (st, msg)
        if pos and nrm:   # the hits variant has one input array, checked below
            st = lib.rt_bake_irradiance_hits_device(h, n_, C.c_void_p(d_hits.data_ptr()), C.byref(p), C.c_void_p(d_out.data_ptr() if res else None), None)
            msg = lib.rt_last_error().decode()
            assert st == status and field in msg and "rt_bake_irradiance_hits_device:" in msg, (st, msg)
        assert (out == 7.0).all() and bool((d_out == 7.0).all())

    all_three(api.RT_E_INVALID, "positions", pos=False)
    all_three(api.RT_E_INVALID, "normals", nrm=False)
    all_three(api.RT_E_INVALID, "rgba_out", res=False)
    all_three(api.RT_E_INVALID, "n must be below 2^31", n_=2 ** 31)
    all_three(api.RT_E_INVALID, "n must be below 2^31", n_=2 ** 40)
    all_three(api.RT_E_INVALID, "n_parts", band_rows=1, n_parts=2, part=0)
    all_three(api.RT_E_INVALID, "precision", precision=2)
    all_three(api.RT_E_INVALID, "sqrt_spt", sqrt_spt=0)
    all_three(api.RT_E_INVALID, "thread_count", thread_count=0)
    all_three(api.RT_E_UNSUPPORTED, "RT_PIPELINE_MEGAKERNEL", pipeline=api.RT_PIPELINE_MEGAKERNEL)
    all_three(api.RT_E_UNSUPPORTED, "collect_stats", collect_stats=1)
    all_three(api.RT_E_UNSUPPORTED, "max_depth", max_depth=0)
    with pytest.raises(api.RtError, match="hits"):
        scene.bake_irradiance_hits_device(n, 0, c.params, d_out.data_ptr())
    with pytest.raises(api.RtError, match="positions"):
        scene.bake_irradiance_device(n, 0, d_n.data_ptr(), c.params, d_out.data_ptr())
    assert bool((d_out == 7.0).all())
    # n = 0 is a no-op, arrays or not; then the call works, with either pipeline value that runs the wavefront scheduler
    p = c.params.copy()
    assert lib.rt_bake_irradiance(h, 0, None, None, C.byref(p), None) == api.RT_OK
    assert lib.rt_bake_irradiance_hits_device(h, 0, None, C.byref(p), None, None) == api.RT_OK
    assert scene.bake_irradiance(np.zeros((0, 3)), np.zeros((0, 3)), p).shape == (0, 4)
    assert (out == 7.0).all()
    p.pipeline = api.RT_PIPELINE_WAVEFRONT
    assert same_bits(scene.bake_irradiance(c.pos, c.nrm, p), good)
    assert same_bits(scene.render(c.hs.camera, frame_params), frame)
    # a zero and a non-finite normal are not errors; the points beside them keep their answers
    nrm = c.nrm.copy()
    nrm[3], nrm[4] = 0.0, (np.nan, 1.0, np.inf)
    odd = scene.bake_irradiance(c.pos, nrm, c.params)
    keep = np.ones(n, dtype=bool)
    keep[3:5] = False
    assert same_bits(odd[keep], good[keep]) and (odd[:, 3] == 0).all()
    scene.close()
    assert api.live_resources() == live0


# ---- 7. f32 against the oracle's f64 values ----
@pytest.mark.parametrize("name", ["cornell", "two_meshes"])
def test_f32_is_statistically_equivalent(dev, name):
    """The bar of test_gpu_parity.test_f32_is_statistically_equivalent, on 64 points x 64 paths (S = 8, T = 1)."""
    c = br.case(name, 64, 8, 1)
    p = c.params.copy()
    p.precision = F32
    scene = api.DeviceScene(c.hs.desc, 0)
    got = scene.bake_irradiance(c.pos, c.nrm, p)
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


# ---- 8. rtrace --irradiance ----
def test_rtrace_irradiance(dev, tmp_path):
    """`rtrace --irradiance -s=2`: out.png and the console lines are those of a run without the flag but for one more line, and
    out_irradiance.png is the output stage of out.png applied to bake_irradiance_hits_device on the trace_rays records of the
    pixel-centre rays (the --pick ray of every pixel, row-major) with the run's parameters; black where a ray finds no surface."""
    import torch
    args = [os.path.join(REPO, "tests", "scenes", "two_meshes"), "-w=24", "-s=2", "--seed=31"]
    outs = {}
    for sub, extra in (("plain", []), ("irr", ["--irradiance"])):
        (tmp_path / sub).mkdir()
        r = subprocess.run([RTRACE] + args + extra, cwd=str(tmp_path / sub), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[sub] = r.stdout
    assert (tmp_path / "irr" / "out.png").read_bytes() == (tmp_path / "plain" / "out.png").read_bytes()
    assert not (tmp_path / "plain" / "out_irradiance.png").exists()
    timeless = lambda text: [re.sub(r"\d+\.\d+(ns|µs|ms|s)", "<t>", ln) for ln in text.splitlines()]
    plain, with_irr = timeless(outs["plain"]), timeless(outs["irr"])
    extra_lines = [ln for ln in with_irr if ln.startswith("Irradiance:")]
    assert len(extra_lines) == 1 and [ln for ln in with_irr if not ln.startswith("Irradiance:")] == plain
    hs = api.HostScene(args + ["--irradiance"])
    assert hs.irradiance
    cam = hs.camera
    W, H = cam.image_width, cam.image_height
    n = W * H
    v = lambda a: np.array(list(a))
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    cam_d = np.ascontiguousarray((v(cam.first_pixel) + x[..., None] * v(cam.pixel_delta_u) + y[..., None] * v(cam.pixel_delta_v) - v(cam.position)).reshape(-1, 3))
    cam_o = np.broadcast_to(v(cam.position), cam_d.shape).copy()
    scene = api.DeviceScene(hs.desc, 0)
    d_o, d_d = torch.from_numpy(cam_o).cuda(), torch.from_numpy(cam_d).cuda()
    d_hits = torch.zeros(n * api.RtRayHit.itemsize, dtype=torch.uint8, device="cuda")
    d_out = torch.full((n, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    scene.trace_rays_device(n, d_o.data_ptr(), d_d.data_ptr(), d_hits.data_ptr())
    p = hs.params.copy()
    p.pipeline, p.collect_stats = api.RT_PIPELINE_AUTO, 0
    scene.bake_irradiance_hits_device(n, d_hits.data_ptr(), p, d_out.data_ptr())
    want = d_out.cpu().numpy().reshape(H, W, 4)
    surface = (rq.klass_of(d_hits.cpu().numpy().view(api.RtRayHit)) == rq.SURFACE).reshape(H, W)
    scene.close()
    assert surface.any() and (~surface).any() and (want[~surface] == 0).all()
    assert len(np.unique(api.tonemap_rgb8(want).reshape(-1, 3), axis=0)) > 16   # a picture, not a constant
    api.save_png(str(tmp_path / "want.png"), want)
    assert (tmp_path / "irr" / "out_irradiance.png").read_bytes() == (tmp_path / "want.png").read_bytes()
    img = api.load_image(str(tmp_path / "irr" / "out_irradiance.png"))
    assert (img[~surface] == 0).all()
    # a scene with volumes is refused before anything is rendered
    (tmp_path / "vol").mkdir()
    r = subprocess.run([RTRACE, os.path.join(REPO, "tests", "scenes", "smoke"), "-w=16", "-s=2", "--irradiance"], cwd=str(tmp_path / "vol"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "--irradiance does not support scenes with volumes" in r.stderr
    assert "finished" not in r.stdout and not (tmp_path / "vol" / "out.png").exists()
