"""Every render mode of the wavefront driver on ONE scene object, one after the other.

A call of render_wavefront has one mode - frame, light groups, ray table, point table, dense or sparse adaptive pass - and all
of them share the scene's workspace: the two path pools, sample_L, sample_G, lg_table, acc, acc_g and the counters.  The tests
of each feature run their mode on a scene of its own; what they cannot see is a mode that leaves something behind for the next
one.  So: on one scene object

    1. a frame   2. a light-group render with 3 groups   3. rt_render_rays_device on 700 rays
    4. rt_bake_irradiance_device on the same 700 points   5. an adaptive accumulator until a sparse pass has run   6. the frame again

and the last frame equals the first bit for bit, and each of the six results equals, bit for bit, the same call on a freshly
created scene object of its own.  32 x 24 pixels, S = 2, T = 3, f64 and f32; a scene with mesh ops (k_wf_prims + k_wf_mesh) and
one without (k_wf_prims alone).  RT_WF_POOL=1024 with RT_WF_COMPACT_MIN=1: every group restarts paths inside k_wf_shade and its
tail compacts; RT_RAYS_CHUNK=256: the 700 table entries form three chunks, the last one partial.  The second case of each scene
adds RT_WF_SAMPLE_GB=0: one replica per group, three replica groups per call, which brings in acc and acc_g.

The adaptive threshold is the median of the noise image after the two replicas before the only decision point (measured once
per case by a probe accumulator on a scene of its own): with radius 0 the pixels at or below it stop and the others go on, so
the third replica is a sparse pass whatever the scene (where the median is 0 - more than half of the frame black - the black
pixels stop and the lit ones go on)."""
import numpy as np
import pytest

import render_rays_ref as rr
from rust_raytracer_amd import api

pytestmark = pytest.mark.gpu

W, H, S, T, N, SEED = 32, 24, 2, 3, 700, 31
SCENES = {"two_meshes": "tests/scenes/two_meshes", "cornell": "scenes/cornell"}   # with mesh ops / without
ENV = {"RT_WF_POOL": "1024", "RT_WF_COMPACT_MIN": "1", "RT_RAYS_CHUNK": "256"}


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


def table_call(scene, device_call, a, b, params):
    import torch
    d_a, d_b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    d_out = torch.full((len(a), 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    device_call(len(a), d_a.data_ptr(), d_b.data_ptr(), params, d_out.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def adaptive(threshold):
    return api.RtAdaptiveParams.defaults(threshold=threshold, radius=0, min_replicas=2, check_interval=1, floor=0.01)


class Case:
    def __init__(self, name, precision):
        self.hs = api.HostScene([SCENES[name], f"-w={W}", f"-r={W / H!r}", f"--seed={SEED}"])
        assert (self.hs.width, self.hs.height) == (W, H)
        assert (self.hs.desc.contents.n_meshes > 0) == (name == "two_meshes")
        self.params = rr.params_for(self.hs, S, T, SEED, precision)
        self.o, self.d = rr.ray_set(name, N)
        m = self.hs.desc.contents.n_materials
        self.groups = api.RtLightGroups.make(3, [k % 3 for k in range(m)], background_group=1, unlit_group=2)
        probe = api.DeviceScene(self.hs.desc, 0)
        pr = api.ProgressiveRender(probe, self.hs.camera, self.params, adaptive=adaptive(1e-300))
        pr.render(2)                                  # every pixel has its two replicas, whatever the decision after them
        self.threshold = max(float(np.nanmedian(pr.noise())), 1e-300)
        pr.close()
        probe.close()

    def frame(self, scene):
        out = scene.render(self.hs.camera, self.params)
        assert scene.stats().n_iterations > 1 and scene.stats().n_tail_compactions >= 1
        return out

    def light_groups(self, scene):
        return np.concatenate([a.reshape(-1) for a in scene.render_light_groups(self.hs.camera, self.params, self.groups)])

    def rays(self, scene):
        return table_call(scene, scene.render_rays_device, self.o, self.d, self.params)

    def bake(self, scene):
        return table_call(scene, scene.bake_irradiance_device, self.o, self.d, self.params)

    def adaptive(self, scene):
        pr = api.ProgressiveRender(scene, self.hs.camera, self.params, adaptive=adaptive(self.threshold))
        pr.render(2)                                  # dense passes, then the decision
        active = pr.active_pixels
        assert 0 < active < W * H, "the third replica must be a sparse pass"
        pr.render(1)
        assert scene.stats().samples == S * S * active
        blob = pr.save_state()
        pr.close()
        return np.frombuffer(blob, dtype=np.uint8)

    STEPS = ("frame", "light_groups", "rays", "bake", "adaptive", "frame")


@pytest.mark.parametrize("one_replica_per_group", [False, True], ids=["one_group", "three_groups"])
@pytest.mark.parametrize("precision", [api.RT_PRECISION_F64, api.RT_PRECISION_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(SCENES))
def test_modes_in_sequence_on_one_scene(dev, monkeypatch, name, precision, one_replica_per_group):
    for k, v in ENV.items():
        monkeypatch.setenv(k, v)
    if one_replica_per_group:
        monkeypatch.setenv("RT_WF_SAMPLE_GB", "0")
    c = Case(name, precision)
    shared = api.DeviceScene(c.hs.desc, 0)
    got = []
    for step in Case.STEPS:
        got.append(getattr(c, step)(shared))
        if step != "adaptive":
            assert shared.stats().n_replica_groups == (T if one_replica_per_group else 1) * (3 if step in ("rays", "bake") else 1)
    shared.close()
    assert got[5].tobytes() == got[0].tobytes(), "the frame after the other modes differs from the frame before them"
    assert np.isfinite(got[0]).all() and (got[0][..., :3] != 0).any() and (got[2][:, :3] != 0).any() and (got[3][:, :3] != 0).any()
    for i, step in enumerate(Case.STEPS):
        fresh = api.DeviceScene(c.hs.desc, 0)
        want = getattr(c, step)(fresh)
        fresh.close()
        assert got[i].shape == want.shape and got[i].tobytes() == want.tobytes(), f"step {i + 1} ({step}) differs from a fresh scene's"
