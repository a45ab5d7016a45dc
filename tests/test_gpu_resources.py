"""Who owns what on the device: after a scene and its accumulator are closed, nothing the library
allocated through HIP is left - device buffers, their bytes, pinned buffers, events and streams, as rt_debug_live_resources
counts them inside the library (the card's free memory would show other people's jobs).

One cycle per precision on scenes/light_test at 45 x 37 and 9 samples per pixel with a 4096-slot pool (as
tests/test_gpu_search_setup.py; the accumulator renders four replicas of them): both schedulers, chunked ray queries and a
bake from host arrays, a light-group render, an adaptive accumulator with a denoised preview, an update that moves the mesh.  Three cycles: a grow-only buffer that is
re-created without being released would show up on the second.  Everything here needs the GPU."""
import os

import numpy as np
import pytest

from rust_raytracer_amd import api
from ray_query_cases import camera_rays, host_scene
from scene_update_cases import displaced_obj

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = ["-w=45", "-r=1.2162", "-s=9", "--seed=52"]
F64, F32 = api.RT_PRECISION_F64, api.RT_PRECISION_F32


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


@pytest.fixture(scope="module")
def rays():
    o, d = camera_rays(host_scene("light_test"))
    assert len(o) == 384
    return o[:-7], d[:-7]  # 377 = 5 chunks of 64 and a ragged one of 57


@pytest.fixture(scope="module")
def moved(tmp_path_factory):
    """scenes/light_test with every vertex of its mesh displaced: same structure, new numbers."""
    tmp = tmp_path_factory.mktemp("resources")
    displaced_obj(os.path.join(REPO, "scenes", "resource", "monkey.obj"), tmp / "moved.obj")
    text = open(os.path.join(REPO, "scenes", "light_test")).read()
    assert "resource/monkey.obj" in text
    (tmp / "light_test_moved").write_text(text.replace("resource/monkey.obj", "moved.obj"))
    return api.HostScene([str(tmp / "light_test_moved")] + SIZE)


def cycle(hs, moved, rays, precision, baseline):
    scene = api.DeviceScene(hs.desc, 0)
    p = hs.params.copy()
    p.precision = precision
    for pipeline in (api.RT_PIPELINE_WAVEFRONT, api.RT_PIPELINE_MEGAKERNEL):
        p.pipeline = pipeline
        scene.render(hs.camera, p)
        assert scene.stats().pipeline_used == pipeline
    alive = api.live_resources()
    assert alive[0] > baseline[0] and alive[1] > baseline[1] and alive[2] > baseline[2] and alive[3] > baseline[3], "the counters count"
    o, d = rays
    hits = scene.trace_rays(o, d, precision=precision)
    assert scene.ray_query_stats().n_chunks == 6
    scene.occluded(o, d, 1e-3, 50.0, precision=precision)
    assert scene.ray_query_stats().n_chunks == 6
    surface = (hits["flags"] & api.RT_RAY_HIT) != 0
    assert surface.sum() > 64
    scene.bake_visibility(hits["pos"][surface], hits["normal"][surface], samples=4, precision=precision)
    assert scene.bake_stats().n_chunks == (int(surface.sum()) + 63) // 64
    p.pipeline = api.RT_PIPELINE_AUTO
    groups = api.light_groups_auto(hs.desc, 16, bool(p.has_background))
    scene.render_light_groups(hs.camera, p, groups)
    p.thread_count = 4  # replicas of the 9 strata: decisions after the second and the third (only the black background stops)
    acc = api.ProgressiveRender(scene, hs.camera, p, adaptive=api.RtAdaptiveParams.defaults(threshold=1e-3, min_replicas=2, check_interval=1))
    assert acc.render(4) == 4
    acc.preview_rgb8_denoised()
    assert scene.update(moved.desc)["n_meshes_refit"] == 1
    acc.close()
    scene.close()


def test_nothing_is_left_after_close(dev, monkeypatch, rays, moved):
    monkeypatch.setenv("RT_WF_POOL", "4096")
    monkeypatch.setenv("RT_RQ_CHUNK", "64")
    monkeypatch.setenv("RT_BAKE_CHUNK", "64")
    hs = api.HostScene(["scenes/light_test"] + SIZE)
    assert (hs.width, hs.height) == (45, 37)
    baseline = api.live_resources()
    for n in range(3):
        for precision in (F64, F32):
            cycle(hs, moved, rays, precision, baseline)
            assert api.live_resources() == baseline, f"cycle {n}, precision {precision}"


def test_refusals_allocate_nothing_that_stays(dev, monkeypatch):
    monkeypatch.setenv("RT_WF_POOL", "4096")
    baseline = api.live_resources()
    hs = api.HostScene(["scenes/light_test"] + SIZE)
    scene = api.DeviceScene(hs.desc, 0)
    scene.render(hs.camera, hs.params)
    before = api.live_resources()
    p = hs.params.copy()
    p.collect_stats = 1  # refused by the device variant, after the host variant has its frames on the device
    with pytest.raises(api.RtError) as e:
        scene.render_light_groups(hs.camera, p, api.light_groups_auto(hs.desc, 16, bool(p.has_background)))
    assert e.value.status == api.RT_E_UNSUPPORTED
    assert api.live_resources() == before
    scene.close()
    smoke = host_scene("smoke")
    assert api.scene_info(smoke.desc) & api.RT_SCENE_INFO_VOLUMES
    scene = api.DeviceScene(smoke.desc, 0)
    before = api.live_resources()
    with pytest.raises(api.RtError) as e:
        scene.trace_rays(np.zeros((2, 3)), np.ones((2, 3)))
    assert e.value.status == api.RT_E_UNSUPPORTED
    assert api.live_resources() == before
    scene.close()
    assert api.live_resources() == baseline
