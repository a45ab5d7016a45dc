"""rt_scene_tables_digest on the CPU: the digests of the seven mesh tables as the host derives them (rt_tables.cpp), which
is what DeviceScene<R>::build uploads (tests/test_gpu_scene_tables.py holds the device to them).  The entries, in the order
of DeviceScene.debug_mesh_digest: BvhNode, BvhNode4f, MeshNode4qc, TriRec, TriAttr, mesh_bounds, MeshOpRec; the eighth is 0."""
import ctypes as C
import os

import numpy as np
import pytest

from rust_raytracer_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPED = (0, 3, 4, 5, 6)   # tables in the kernels' arithmetic type


def mesh_scene(tmp_path, name, objs):
    """A scene of the meshes `objs` under a white sky (assets are named relative to the scene file)."""
    lines = ["@config aspect_ratio = 1"] + [f"m{i}: mesh {os.path.relpath(os.path.join(REPO, o), str(tmp_path))} (lambertian (constant 0.7,0.7,0.7))" for i, o in enumerate(objs)]
    lines += ["sky: sky (constant 1,1,1)", "world: list " + " ".join(f"$m{i}" for i in range(len(objs))) + " $sky", "lights: list $sky"]
    path = tmp_path / name
    path.write_text("\n".join(lines) + "\n")
    return api.HostScene([str(path), "-w=8", "-s=1"])


SCENES = {
    "cube": lambda tmp_path: mesh_scene(tmp_path, "cube", ["tests/scenes/cube.obj"]),
    "two_meshes": lambda tmp_path: api.HostScene(["tests/scenes/two_meshes", "-w=8", "-s=1"]),
    # two distinct meshes whose boxes, and so whose pads, differ (both meshes of two_meshes are the same file)
    "cube_and_monkey": lambda tmp_path: mesh_scene(tmp_path, "cube_and_monkey", ["tests/scenes/cube.obj", "scenes/resource/monkey_low.obj"]),
}


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_digest_repeats(tmp_path, name, f32):
    hs = SCENES[name](tmp_path)
    first = api.scene_tables_digest(hs.desc, f32)
    assert len(first) == 8 and first[7] == 0
    assert api.scene_tables_digest(hs.desc, f32) == first


@pytest.mark.parametrize("name", sorted(SCENES))
def test_precisions_differ_in_the_typed_tables(tmp_path, name):
    hs = SCENES[name](tmp_path)
    d64, d32 = api.scene_tables_digest(hs.desc, False), api.scene_tables_digest(hs.desc, True)
    for k in TYPED:
        assert d64[k] != d32[k], k
    assert d64[1] == d32[1]   # BvhNode4f is f32 for both types: the code guarantees this one
    # MeshNode4qc depends on the type through the cones' conditioning limits only (rt_bvh.cpp cone_limits): equal as long
    # as no triangle lies between the two limits, which holds for these well-shaped meshes
    assert d64[2] == d32[2]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_moved_positions_change_every_table(tmp_path, name, f32):
    hs, other = SCENES[name](tmp_path), SCENES["two_meshes"](tmp_path)
    before, other_before = api.scene_tables_digest(hs.desc, f32), api.scene_tables_digest(other.desc, f32)
    m = hs.desc.contents.meshes[0]
    pos = np.ctypeslib.as_array(m.positions, shape=(m.n_positions, 3))
    # TriAttr holds normals and uvs, which see the positions only through the leaf order: a move that gives another tree
    pos[:] = np.stack([pos[:, 2] * 1.7 + 0.3 * pos[:, 1], pos[:, 1] * 0.6, pos[:, 0] * 2.9], axis=1)
    after = api.scene_tables_digest(hs.desc, f32)
    for k in range(7):
        assert after[k] != before[k], k
    assert api.scene_tables_digest(other.desc, f32) == other_before


def test_null_arguments():
    lib = api.load_device_lib()
    out = (C.c_uint64 * 8)()
    hs = api.HostScene(["tests/scenes/two_meshes", "-w=8", "-s=1"])
    assert lib.rt_scene_tables_digest(None, 0, out) == api.RT_E_INVALID
    assert lib.rt_scene_tables_digest(hs.desc, 0, None) == api.RT_E_INVALID
    assert "rt_scene_tables_digest" in lib.rt_last_error().decode()
