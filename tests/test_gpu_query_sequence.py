"""Ray queries, point queries, the visibility bake and lightmaps in sequence on one scene, across an rt_scene_update.

Three of them share one piece of state in the scene: the op -> node and leaf slot -> triangle tables that the first of
rt_lightmap_texels, rt_closest_points and rt_trace_rays uploads, stamped with the scene's generation and uploaded again by the
first of them after an update.  rt_occluded and rt_bake_visibility_hits_device share the staging buffers with them but not
the tables.  tests/test_gpu_mode_sequence.py holds the render modes to this; here every result of a sequence must equal, byte
for byte, the same call made alone: before the update on a fresh scene, after it on a scene created from the first
description, updated, and then used for that single call.  The bytes must differ between before and after.

A limit of these inputs: the update moves vertices and keeps the topology, so op_node and tri_order are very likely the same
arrays before and after it, and a stale generation stamp of the tables alone would not show here; what shows is a call that
reads another subsystem's leftovers, the wrong scene tables, or tables that were never uploaded."""
import numpy as np
import pytest

import lightmap_ref as lr
from rust_raytracer_amd import api

pytestmark = pytest.mark.gpu

W, H = 32, 16
N = 256
TABLE_USERS = ("lightmap_texels", "closest_points", "trace_rays")
OTHERS = ("occluded", "bake_visibility_hits")


@pytest.fixture(scope="module", autouse=True)
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


def _inputs(desc, node):
    """256 rays from a sphere around the mesh's world box towards points inside it, 256 points in the box blown up by a half."""
    mesh = lr.Mesh(desc, node)
    world = mesh.positions
    for m4 in mesh.chain:
        world = lr._apply(m4, world, 1.0)
    lo, hi = world.min(axis=0), world.max(axis=0)
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    rng = np.random.default_rng(20)
    origins = centre + 3.0 * np.linalg.norm(half) * lr._unit(rng.standard_normal((N, 3)))
    dirs = centre + half * rng.uniform(-1, 1, (N, 3)) - origins
    points = centre + 1.5 * half * rng.uniform(-1, 1, (N, 3))
    return origins, dirs, points


def test_queries_in_every_order_across_an_update():
    import torch
    before_hs = lr.new_host_scene("sequence_a", lr.MONKEY1_BODY.format(obj=lr._rel(lr.MONKEY)), "$m")
    moved = lr.moved_obj(lr.MONKEY, "monkey_moved_sequence.obj")
    after_hs = lr.new_host_scene("sequence_b", lr.MONKEY1_BODY.format(obj=lr._rel(moved)), "$m")
    node = lr.mesh_nodes(before_hs.desc)[0]
    origins, dirs, points = _inputs(before_hs.desc, node)
    bp = api.RtBakeParams.defaults(samples=16, seed=3)
    records = {}  # state -> the map's records on the device: the bake's input, the same bytes for the sequences and the solo call

    def call(scene, name, state):
        if name == "lightmap_texels":
            return scene.lightmap_texels(node, W, H).tobytes()
        if name == "closest_points":
            return scene.closest_points(points).tobytes()
        if name == "trace_rays":
            return scene.trace_rays(origins, dirs).tobytes()
        if name == "occluded":
            return scene.occluded(origins, dirs).tobytes()
        d_out = torch.full((W * H * api.RtBakeResult.itemsize,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        scene.bake_visibility_hits_device(W * H, records[state].data_ptr(), d_out.data_ptr(), bp)
        return d_out.cpu().numpy().tobytes()

    def solo_scene(state):
        scene = api.DeviceScene(before_hs.desc, 0)
        if state == "after":
            assert scene.update(after_hs.desc)["n_meshes_refit"] == 1
        return scene

    solo = {}
    for state in ("before", "after"):
        for name in TABLE_USERS + OTHERS:
            scene = solo_scene(state)
            solo[state, name] = call(scene, name, state)
            scene.close()
            if name == "lightmap_texels":
                records[state] = torch.from_numpy(np.frombuffer(solo[state, name], dtype=np.uint8).copy()).cuda()
    for name in TABLE_USERS + OTHERS:
        assert solo["before", name] != solo["after", name], f"{name}: the update does not show in the result"

    def run(scene, order, state):
        for k, name in enumerate(order):
            for each in (name,) + (OTHERS if k == 1 else ()):
                assert call(scene, each, state) == solo[state, each], f"{each} in the order {order} {state} the update: not the call made alone"

    for r in range(3):
        scene = api.DeviceScene(before_hs.desc, 0)
        run(scene, TABLE_USERS[r:] + TABLE_USERS[:r], "before")
        assert scene.update(after_hs.desc)["n_meshes_refit"] == 1
        r = (r + 1) % 3
        run(scene, TABLE_USERS[r:] + TABLE_USERS[:r], "after")
        scene.close()
