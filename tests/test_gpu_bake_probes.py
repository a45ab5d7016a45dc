"""rt_bake_probes and rt_sh_irradiance on the GPU (include/rt_mi355.h): SH radiance probes in free space.

The f64 yardstick is the CPU oracle sample by sample (tests/bake_probes_ref.py: the direction and the basis restated in numpy,
the reference's camera returning the first ray, pyoracle.trace_sample; its probe sets are checked for being worth testing in
tests/test_bake_probes_host.py), at 1e-12 of a probe's largest coefficient; a constant sky gives a closed form with no oracle
tracing at all; and everything about the shape of a run - chunks, pool size, replica groups, tail compaction - must leave every
bit alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bake_probes_ref as bp
import render_rays_ref as rr
import scene_update_cases as su
from rust_raytracer_amd import api

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


def assert_probe_parity(got, ref, rel=1e-12):
    """Every value within `rel` of the probe's largest coefficient (a probe whose reference is all zero must be all zero)."""
    assert got.shape == ref.shape and np.isfinite(got).all()
    scale = np.abs(ref[:, :, :3]).max(axis=(1, 2))
    err = np.abs(got[:, :, :3] - ref[:, :, :3]).max(axis=(1, 2))
    bad = err > rel * scale
    assert not bad.any(), f"{int(bad.sum())} of {len(ref)} probes beyond {rel} of their largest coefficient (worst ratio {np.max(err[bad] / np.maximum(scale[bad], 1e-300)):.3e})"
    assert (got[:, :, 3] == 0).all()


def sh_irradiance_numpy(sh, probe, normals):
    """rt_sh_irradiance restated: (values (m, 4), sum of the absolute terms (m, 3), the bands 1-2 part (m, 3))."""
    out, mag, rest = np.zeros((len(probe), 4)), np.zeros((len(probe), 3)), np.zeros((len(probe), 3))
    for j, (p, nr) in enumerate(zip(probe, normals)):
        nr = np.asarray(nr, dtype=np.float64)
        w = nr / np.sqrt(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2])
        y = bp.basis(w)
        a = sh[p]
        for c in range(3):
            band1 = (a[1, c] * y[1] + a[2, c] * y[2]) + a[3, c] * y[3]
            band2 = (((a[4, c] * y[4] + a[5, c] * y[5]) + a[6, c] * y[6]) + a[7, c] * y[7]) + a[8, c] * y[8]
            out[j, c] = (4.0 * np.pi) * ((a[0, c] * y[0] + (2.0 / 3.0) * band1) + 0.25 * band2)
            rest[j, c] = (4.0 * np.pi) * ((2.0 / 3.0) * band1 + 0.25 * band2)
            mag[j, c] = (4.0 * np.pi) * (abs(a[0, c] * y[0]) + (2.0 / 3.0) * np.abs(a[1:4, c] * y[1:4]).sum() + 0.25 * np.abs(a[4:, c] * y[4:]).sum())
    return out, mag, rest


# ---- 1. f64 against the oracle ----
@pytest.mark.parametrize("name", bp.SCENES)
def test_f64_matches_the_oracle(dev, name):
    """n = 37: the last wave is partial.  smoke: volumes (k_wf_intersect<VOL>), texture_mix: the interpreter form of k_wf_shade."""
    c = bp.case(name)
    scene = api.DeviceScene(c.hs.desc, 0)
    got = scene.bake_probes(c.pos, c.params)
    assert got.shape == (c.n, 9, 4)
    scale = np.maximum(np.abs(c.ref[:, :, :3]).max(axis=(1, 2)), 1e-300)
    err = np.abs(got[:, :, :3] - c.ref[:, :, :3]).max(axis=(1, 2))
    print(f"{name}: worst error / largest coefficient of the probe {np.max(err / scale):.3e}, "
          f"{int((got[:, :, :3] != c.ref[:, :, :3]).sum())} of {27 * c.n} values differ in any bit")
    assert_probe_parity(got, c.ref)
    bp.assert_band_bound(got, 1e-12)
    st = scene.stats()
    assert st.samples == c.n * c.t * c.s * c.s and st.pipeline_used == api.RT_PIPELINE_WAVEFRONT
    scene.close()


# ---- 2. a closed form: no oracle tracing ----
def test_constant_sky_gives_the_ordered_sums_of_the_basis(dev):
    """tests/scenes/sky_only: every path returns (0.5, 1, 2) exactly, so out[i][k] is the ordered numpy sum of Y_k(d_s) * L, and
    rt_sh_irradiance of it at any normal is L up to what bands 1-8 of a finite sample keep: that remainder is computed, not guessed.
    n = 70: two blocks of 64 probes in k_wf_resolve_sh, the second ragged."""
    hs = api.HostScene(["tests/scenes/sky_only", "-w=8"])
    n, s, t = 70, 4, 2
    p = rr.params_for(hs, s, t, bp.SEED)
    pos = api.probe_grid((-3.0, 0.5, 10.0), (4.0, 2.5, 11.0), (7, 5, 2))
    assert len(pos) == n
    L = np.array([0.5, 1.0, 2.0])
    dirs = bp.sample_dirs(n, s, t, bp.SEED)
    want = bp.ordered_sums(dirs, np.broadcast_to(L, dirs.shape), s, t)
    scene = api.DeviceScene(hs.desc, 0)
    got = scene.bake_probes(pos, p)
    err = np.abs(got - want).max()
    print(f"sky_only: max abs err {err:.3e}, {int((got != want).sum())} of {got.size} values differ in any bit")
    assert_probe_parity(got, want, rel=1e-13)
    # f32: the same closed form with the f32 directions is not restated; the f64 one bounds it loosely - and must not be equalled
    p32 = p.copy()
    p32.precision = F32
    got32 = scene.bake_probes(pos, p32)
    assert np.isfinite(got32).all() and not same_bits(got32, got)
    # band 0 is float(Y0) * L whatever the directions: the constant's rounding, 2^-24 relative, and a few f64 ulps of the sums
    assert (np.abs(got32[:, 0, :3] - bp.C0 * L) <= (2.0 ** -24 + 1e-14) * bp.C0 * L).all()
    bp.assert_band_bound(got32, 1e-5)
    scene.close()
    # lighting: 4 pi Y0 Y0 = 1, so band 0 alone gives L; the rest is the Monte-Carlo error of bands 1-8, taken from numpy
    rng = np.random.default_rng(5)
    m = 300
    probe = rng.integers(0, n, size=m)
    normals = rng.normal(size=(m, 3)) * rng.uniform(0.1, 10.0, size=(m, 1))
    lit = api.sh_irradiance(got, probe, normals)
    ref, mag, rest = sh_irradiance_numpy(want, probe, normals)
    assert np.abs(lit[:, :3] - ref[:, :3]).max() <= 1e-12 and (lit[:, 3] == 0).all()
    print(f"sky_only: irradiance / L - 1 within {np.abs(lit[:, :3] / L - 1).max():.3e}; numpy's bands 1-8 give {np.abs(rest / L).max():.3e}")
    assert (np.abs(lit[:, :3] - L) <= np.abs(rest) + 1e-12 * mag).all()


# ---- 3. cross-check without the oracle ----
@pytest.mark.parametrize("name", ["cornell", "smoke"])
def test_one_sample_per_probe_equals_render_rays_along_the_restated_ray(dev, name):
    """S = T = 1: probe i's only sample is keyed (seed, 0, i, 0) on both sides; rt_render_rays drops the two draws the bake forms
    its direction from, so along d' = (o + d) - o restated in numpy it gives L_i, and out[i][k] = fl(Y_k(d_i) * L_i) bit for bit.
    n = 1 000: several waves."""
    n = 1000
    pos = bp.probe_set(name, n)   # the walk wraps round: a position comes back under other indices, i.e. with other directions
    hs = bp.rq.cases(name).hs
    p = rr.params_for(hs, 1, 1, bp.SEED)
    dirs = bp.sample_dirs(n, 1, 1, bp.SEED).reshape(n, 3)
    rays = bp.first_rays(pos, 1, 1, bp.SEED)
    assert same_bits(rays[:, :3], pos) and same_bits(rays[:, 3:], (pos + dirs) - pos)
    scene = api.DeviceScene(hs.desc, 0)
    baked = scene.bake_probes(pos, p)
    along = scene.render_rays(np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:]), p)
    y = np.array([bp.basis(d) for d in dirs])
    want = np.zeros((n, 9, 4))
    want[:, :, :3] = 0.0 + (0.0 + y[:, :, None] * along[:, None, :3]) / 1.0   # the resolve's additions to +0.0 (a -0.0 product becomes +0.0)
    assert same_bits(baked, want), f"{int((baked != want).any(axis=(1, 2)).sum())} of {n} probes differ"
    lit = along[(along[:, :3] != 0).any(axis=1)]
    print(f"{name}: {len(lit)} of {n} probes carry radiance")
    assert np.isfinite(baked).all() and len(lit) > 0 and len({r.tobytes() for r in lit}) > 1
    scene.close()


# ---- 4. independence of the run shape ----
@pytest.mark.parametrize("name", ["cornell", "two_meshes"])
def test_answers_do_not_depend_on_the_shape_of_the_run(dev, name, monkeypatch):
    c = bp.case(name)
    scene = api.DeviceScene(c.hs.desc, 0)
    first = scene.bake_probes(c.pos, c.params)
    assert_probe_parity(first, c.ref)
    groups0 = scene.stats().n_replica_groups

    def again(what, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = scene.bake_probes(c.pos, c.params)
        st = scene.stats()
        for k in env:
            monkeypatch.delenv(k)
        assert same_bits(got, first), f"{what}: {int((got != first).any(axis=(1, 2)).sum())} probes differ"
        assert st.samples == c.n * c.t * c.s * c.s
        return st

    again("chunks of 16 probes", RT_RAYS_CHUNK="16")             # three chunks, the last of 5: chunk boundaries, global keys
    # 37 * 12 = 444 samples through 64 slots: most first rays are formed in k_wf_shade's restart, not in k_wf_generate
    st = again("a pool of 64 slots", RT_WF_POOL="64")
    assert st.n_iterations > 1
    again("a pool of 64 slots, chunks of 16", RT_WF_POOL="64", RT_RAYS_CHUNK="16")
    st = again("one replica per group", RT_WF_SAMPLE_GB="0")     # the 27 running sums per probe between groups
    assert st.n_replica_groups == c.t > groups0
    again("one replica per group, chunks of 16", RT_WF_SAMPLE_GB="0", RT_RAYS_CHUNK="16")
    again("no tail compaction", RT_WF_COMPACT="0")
    st = again("tail compaction from 8 paths on", RT_WF_COMPACT_MIN="8", RT_WF_POOL="256")
    again("k_wf_prims stand-alone", RT_WF_FUSE="0")
    again("k_wf_prims inside k_wf_shade, restarts there", RT_WF_FUSE="2", RT_WF_POOL="64")
    # first != 0: a chunk that begins at probe 30 is keyed 30, 31, ... and equals the reference of those probes; the same
    # positions baked alone are probes 0, 1, ...: other streams
    monkeypatch.setenv("RT_RAYS_CHUNK", "30")
    chunked = scene.bake_probes(c.pos, c.params)
    monkeypatch.delenv("RT_RAYS_CHUNK")
    assert same_bits(chunked, first)
    assert_probe_parity(chunked[30:], c.ref[30:])
    alone = scene.bake_probes(c.pos[30:], c.params)
    changed = (alone[:, :, :3] != first[30:, :, :3]).any(axis=(1, 2))
    lit = (first[30:, :, :3] != 0).any(axis=(1, 2))   # a probe that carries radiance weights it by its own directions: bands 1-2 move with the streams
    assert lit.any() and changed[lit].all()
    assert same_bits(scene.bake_probes(c.pos[:1], c.params), first[:1])   # n = 1
    scene.close()


# ---- 5. variants ----
def test_device_variant_equals_the_host_variant(dev):
    import torch
    c = bp.case("cornell")
    scene = api.DeviceScene(c.hs.desc, 0)
    host = scene.bake_probes(c.pos, c.params)
    d_p = torch.from_numpy(c.pos).cuda()
    d_out = torch.full((c.n, 9, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    scene.bake_probes_device(c.n, d_p.data_ptr(), c.params, d_out.data_ptr())
    assert same_bits(d_out.cpu().numpy(), host)
    stream = torch.cuda.Stream()
    d_out.fill_(7.0)
    torch.cuda.synchronize()
    scene.bake_probes_device(c.n, d_p.data_ptr(), c.params, d_out.data_ptr(), stream=stream.cuda_stream)
    assert same_bits(d_out.cpu().numpy(), host)
    assert same_bits(scene.bake_probes(c.pos[3], c.params), scene.bake_probes(c.pos[3:4], c.params))   # a single (3,) position is probe 0 of a call of one
    scene.close()


def test_after_an_update_the_answers_are_a_fresh_scenes(dev, tmp_path):
    c = bp.case("two_meshes")
    before = su.two_meshes_variant(tmp_path, "before", numeric=False)
    after = su.two_meshes_variant(tmp_path, "after", numeric=True)
    scene = api.DeviceScene(before.desc, 0)
    old = scene.bake_probes(c.pos, c.params)
    scene.update(after.desc)
    got = scene.bake_probes(c.pos, c.params)
    fresh_scene = api.DeviceScene(after.desc, 0)
    fresh = fresh_scene.bake_probes(c.pos, c.params)
    assert same_bits(got, fresh)
    assert not same_bits(got, old)
    scene.close()
    fresh_scene.close()


def test_a_bake_leaves_the_scene_and_refusals_leave_the_output(dev):
    import torch
    c = bp.case("cornell")
    live0 = api.live_resources()
    scene = api.DeviceScene(c.hs.desc, 0)
    lib, h = scene._lib, scene._h
    frame_params = rr.params_for(c.hs, 2, 2, 5)
    frame = scene.render(c.hs.camera, frame_params)
    good = scene.bake_probes(c.pos, c.params)
    assert same_bits(scene.render(c.hs.camera, frame_params), frame)
    n = c.n
    out = np.full((n, 9, 4), 7.0)
    d_p = torch.from_numpy(c.pos).cuda()
    d_out = torch.full((n, 9, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def both(status, field, n_=n, pos=True, res=True, **changes):
        p = c.params.copy()
        for k, v in changes.items():
            setattr(p, k, v)
        st = lib.rt_bake_probes(h, n_, c.pos.ctypes.data if pos else None, C.byref(p), out.ctypes.data if res else None)
        msg = lib.rt_last_error().decode()
        assert st == status and field in msg and "rt_bake_probes:" in msg, (st, msg)
        st = lib.rt_bake_probes_device(h, n_, C.c_void_p(d_p.data_ptr() if pos else None), C.byref(p), C.c_void_p(d_out.data_ptr() if res else None), None)
        msg = lib.rt_last_error().decode()
        assert st == status and field in msg and "rt_bake_probes_device:" in msg, (st, msg)
        assert (out == 7.0).all() and bool((d_out == 7.0).all())

    both(api.RT_E_INVALID, "positions", pos=False)
    both(api.RT_E_INVALID, "sh_out", res=False)
    both(api.RT_E_INVALID, "n must be below 2^31", n_=2 ** 31)
    both(api.RT_E_INVALID, "n must be below 2^31", n_=2 ** 40)
    both(api.RT_E_INVALID, "n_parts", band_rows=1, n_parts=2, part=0)
    both(api.RT_E_INVALID, "precision", precision=2)
    both(api.RT_E_INVALID, "sqrt_spt", sqrt_spt=0)
    both(api.RT_E_INVALID, "thread_count", thread_count=0)
    both(api.RT_E_UNSUPPORTED, "RT_PIPELINE_MEGAKERNEL", pipeline=api.RT_PIPELINE_MEGAKERNEL)
    both(api.RT_E_UNSUPPORTED, "collect_stats", collect_stats=1)
    both(api.RT_E_UNSUPPORTED, "max_depth", max_depth=0)
    with pytest.raises(api.RtError, match="positions"):
        scene.bake_probes_device(n, 0, c.params, d_out.data_ptr())
    assert bool((d_out == 7.0).all())
    # n = 0 is a no-op, arrays or not; then the call works, with either pipeline value that runs the wavefront scheduler
    p = c.params.copy()
    assert lib.rt_bake_probes(h, 0, None, C.byref(p), None) == api.RT_OK
    assert scene.bake_probes(np.zeros((0, 3)), p).shape == (0, 9, 4)
    assert (out == 7.0).all()
    p.pipeline = api.RT_PIPELINE_WAVEFRONT
    assert same_bits(scene.bake_probes(c.pos, p), good)
    assert same_bits(scene.render(c.hs.camera, frame_params), frame)
    scene.close()
    assert api.live_resources() == live0


# ---- 6. f32 against the oracle's f64 values ----
@pytest.mark.parametrize("name", ["cornell", "two_meshes"])
def test_f32_is_statistically_equivalent(dev, name):
    """Band 0 / Y0 is a mean radiance: the bar of test_gpu_bake_irradiance.test_f32_is_statistically_equivalent (no NaN, not the
    f64 bits, means within 1 %, 95 % of the values within max(5 %, 0.02)) on 64 probes x 64 paths (S = 8, T = 1).  Bands 1-8:
    finite and within (max |Y_k| / Y0) * out_0, which holds because L >= 0 (slack 1e-5: f32 roundings of Y and of the constants)."""
    c = bp.case(name, 64, 8, 1)
    p = c.params.copy()
    p.precision = F32
    scene = api.DeviceScene(c.hs.desc, 0)
    got = scene.bake_probes(c.pos, p)
    a, b = got[:, 0, :3] / bp.C0, c.ref[:, 0, :3] / bp.C0
    close = np.abs(a - b) <= np.maximum(0.05 * np.abs(b), 0.02)
    print(f"{name}: f32 mean {a.mean():.6f}, f64 mean {b.mean():.6f} ({abs(a.mean() - b.mean()) / b.mean():.4%} apart), "
          f"{close.mean():.3%} of values close")
    assert not np.isnan(a).any()
    assert (a != b).any()   # f32 arithmetic cannot give the f64 bits: the f32 kernels ran
    assert abs(a.mean() - b.mean()) <= 0.01 * b.mean()
    assert close.mean() >= 0.95, f"only {close.mean():.3%} of f32 values are close to the f64 oracle"
    assert np.isfinite(got).all() and (got[:, :, 3] == 0).all()
    bp.assert_band_bound(got, 1e-5)
    bp.assert_band_bound(c.ref, 1e-12)
    scene.close()


# ---- 7. rt_sh_irradiance_device ----
def test_sh_irradiance_device_against_numpy(dev):
    """Same order of operations as the header's formula, within 1e-14 of the sum of the absolute terms; an index out of range gives
    (0, 0, 0, 0) on the device variant and RT_E_INVALID, output untouched, on the host variant.  m = 300: two blocks."""
    import torch
    rng = np.random.default_rng(19)
    n, m = 5, 300
    sh = np.zeros((n, 9, 4))
    sh[:, :, :3] = rng.normal(size=(n, 9, 3)) * rng.uniform(0.01, 100.0, size=(n, 1, 1))
    probe = rng.integers(0, n, size=m).astype(np.uint32)
    normals = rng.normal(size=(m, 3)) * rng.uniform(1e-3, 1e3, size=(m, 1))
    normals[:3] = [(0.0, 0.0, 2.0), (-3.0, 0.0, 0.0), (0.0, 0.5, 0.0)]
    want, mag, _ = sh_irradiance_numpy(sh, probe, normals)
    host = api.sh_irradiance(sh, probe, normals)
    assert host.shape == (m, 4) and (host[:, 3] == 0).all()
    err = np.abs(host[:, :3] - want[:, :3])
    print(f"sh_irradiance: worst error / sum of absolute terms {np.max(err / mag):.3e}, {int((host != want).sum())} of {host.size} values differ in any bit")
    assert (err <= 1e-14 * mag).all()
    bad = probe.copy()
    bad[[7, 299]] = [n, 0xFFFFFFFF]
    d_sh, d_probe, d_n = torch.from_numpy(sh).cuda(), torch.from_numpy(bad.view(np.int32)).cuda(), torch.from_numpy(normals).cuda()
    d_out = torch.full((m, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    api.sh_irradiance_device(d_sh.data_ptr(), n, d_probe.data_ptr(), d_n.data_ptr(), m, d_out.data_ptr())
    got = d_out.cpu().numpy()
    keep = np.ones(m, dtype=bool)
    keep[[7, 299]] = False
    assert same_bits(got[keep], host[keep])
    assert (got[~keep] == 0).all() and not np.signbit(got[~keep]).any()
    out = np.full((m, 4), 7.0)
    lib = api.load_device_lib()
    assert lib.rt_sh_irradiance(0, sh.ctypes.data, n, bad.ctypes.data, normals.ctypes.data, m, out.ctypes.data) == api.RT_E_INVALID
    assert b"probe[7] = 5" in lib.rt_last_error() and (out == 7.0).all()
    # a single probe and a single normal broadcast
    assert same_bits(api.sh_irradiance(sh, 2, normals[:4]), api.sh_irradiance(sh, [2, 2, 2, 2], normals[:4]))
    assert api.sh_irradiance(sh, probe[:4], normals[0]).shape == (4, 4)


# ---- 8. rtrace --sh-probe ----
def test_rtrace_sh_probe(dev, tmp_path):
    """`rtrace --sh-probe=<p0>:<p1>` prints what bake_probes gives for those positions with the run's parameters (%.17g: every bit)
    and renders nothing."""
    args = [os.path.join(REPO, "scenes", "cornell"), "-w=24", "-s=64", "-t=2", "--seed=31", "--sh-probe=278,273,278:100.5,400,250"]
    r = subprocess.run([RTRACE] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not (tmp_path / "out.png").exists()
    hs = api.HostScene(args)
    assert hs.sh_probes.tolist() == [[278.0, 273.0, 278.0], [100.5, 400.0, 250.0]]
    p = hs.params.copy()
    p.pipeline, p.collect_stats = api.RT_PIPELINE_AUTO, 0
    p.band_rows, p.n_parts, p.part = 0, 0, 0
    scene = api.DeviceScene(hs.desc, 0)
    want = scene.bake_probes(hs.sh_probes, p)
    scene.close()
    rows = re.findall(r"^SH probe (\d+) coefficient (\d+): (\S+) (\S+) (\S+)$", r.stdout, re.M)
    assert len(rows) == 18 and [(int(i), int(k)) for i, k, *_ in rows] == [(i, k) for i in range(2) for k in range(9)]
    got = np.array([[float(x) for x in row[2:]] for row in rows]).reshape(2, 9, 3)
    assert same_bits(got, np.ascontiguousarray(want[:, :, :3]))
    assert p.sqrt_spt * p.sqrt_spt * p.thread_count >= 32   # inside the lit box: a probe of that many paths carries radiance
    assert (want[:, 0, :3] > 0).all() and (want[:, 1:, :3] != 0).any()
    assert len(re.findall(r"^SH probe \d+ at ", r.stdout, re.M)) == 2
