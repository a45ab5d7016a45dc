"""The progressive accumulator as a client of the renderer (csrc/rt_accum.hip over csrc/rt_render.h):
one rt_accum_render call of an adaptive accumulator that renders three segments, with a tail flag set on the scene.

Cornell at 16 x 16, four samples a replica (S = 2), T = 6; min_replicas 2, check_interval 2, radius 0, so the decision points
are 2 and 4 and render(6) is the segments [0, 2), [2, 4), [4, 6).  The threshold is the median of the noise image after two
replicas (a probe accumulator on a scene of its own), so the pixels at or below it stop at k = 2 and the others go on.  During
the call the accumulator takes the flag off the scene, so that no segment's tail raises it, and puts it back; the call's end
raises it; the scene's stats are the sums over the segments; and the result does not depend on the split into calls."""
import ctypes as C

import numpy as np
import pytest

from rust_raytracer_amd import api

pytestmark = pytest.mark.gpu

W, S, T = 16, 2, 6
ARGS = ["scenes/cornell", f"-w={W}", "-r=1.0", f"-s={S * S * T}", f"-t={T}", "--seed=31"]


def test_one_adaptive_call_of_three_segments_keeps_the_scene_s_tail_flag_and_sums_its_stats():
    import torch
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    hs = api.HostScene(ARGS)
    p = hs.params
    assert (hs.width, hs.height, p.sqrt_spt, p.thread_count) == (W, W, S, T)

    def adaptive(threshold):
        return api.RtAdaptiveParams.defaults(threshold=threshold, radius=0, min_replicas=2, check_interval=2, floor=0.01)

    probe = api.DeviceScene(hs.desc, 0)
    pr = api.ProgressiveRender(probe, hs.camera, p, adaptive=adaptive(1e-300))
    pr.render(2)
    threshold = max(float(np.nanmedian(pr.noise())), 1e-300)
    pr.close()
    probe.close()

    scene = api.DeviceScene(hs.desc, 0)
    flag = C.c_int32(0)
    assert lib.rt_scene_set_tail_flag(scene._h, C.addressof(flag)) == api.RT_OK
    try:
        pr = api.ProgressiveRender(scene, hs.camera, p, adaptive=adaptive(threshold))
        flag.value = 0
        assert pr.render(T) == T                      # one call, three segments
        assert flag.value == 1, "the call's end does not release the tail flag"
        stats = scene.stats()
        counts = pr.sample_counts()
        assert (counts == 2).any() and (counts > 2).any(), "some pixels, not all, must stop at k = 2"
        assert stats.samples == S * S * int(counts.sum(dtype=np.uint64))
        assert stats.n_replica_groups >= 3
        got = pr.estimate()
        pr.close()
        # the scene holds the flag again: a plain render raises it
        d_out = torch.empty((W, W, 4), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        flag.value = 0
        scene.render_device(hs.camera, p, d_out.data_ptr())
        torch.cuda.synchronize()
        assert flag.value == 1, "the accumulator did not put the scene's tail flag back"
    finally:
        assert lib.rt_scene_set_tail_flag(scene._h, None) == api.RT_OK
    scene.close()

    other = api.DeviceScene(hs.desc, 0)               # no tail flag, the same replicas in three calls
    pr = api.ProgressiveRender(other, hs.camera, p, adaptive=adaptive(threshold))
    for _ in range(3):
        pr.render(2)
    want = pr.estimate()
    assert (pr.sample_counts() == counts).all()
    pr.close()
    other.close()
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
