"""k_wf_mesh on tables with slab-only axes (rt_bvh.cpp build_mesh_slab_axes; host side: tests/test_slab_axes.py) against the same
library with RT_SLAB_AXES=0, which derives the parent's words.  The kernels are the same: only the cone and slab words of inner
children without a back-face cone differ.  A slab only ever drops a child no triangle of which the ray can hit inside its box,
so with the slab step on (RT_WF_SLABS=1; the scenes of this file are below the size at which it is on by default)
 * the frame is the same bits with and without the axes, with the step off, and from the megakernel, in f64 and f32;
 * in f64 the axes only remove work: node visits and triangle tests no higher on any scene, node visits strictly lower on the
   cornell_dragon stand-in, whose top-level children have no cones;
 * in f32, where k_wf_mesh has no slab step, the counters are equal;
 * after an rt_scene_update that moves the knot's vertices non-rigidly, so that other axes are chosen, the MeshNode4qc table the
   refit kernels wrote equals the host builder's byte for byte and the frame equals a fresh scene's."""
import os
import subprocess

import numpy as np
import pytest

from rust_raytracer_amd import api
from scene_update_cases import displaced_obj
from test_gpu_mesh_slabs import PRECISIONS, SCENES, assert_same_bits, make_scene

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


def render(hs, prec, monkeypatch, slabs=1, axes=True, pipeline=api.RT_PIPELINE_WAVEFRONT, stats=True):
    p = hs.params.copy()
    p.pipeline = pipeline
    p.precision = PRECISIONS[prec]
    p.collect_stats = int(stats)
    monkeypatch.setenv("RT_WF_SLABS", str(slabs))
    if axes:
        monkeypatch.delenv("RT_SLAB_AXES", raising=False)
    else:
        monkeypatch.setenv("RT_SLAB_AXES", "0")
    scene = api.DeviceScene(hs.desc, 0)
    try:
        frame = scene.render(hs.camera, p)
        st = scene.stats()
        assert st.pipeline_used == pipeline
        return frame, st
    finally:
        scene.close()
        monkeypatch.delenv("RT_WF_SLABS", raising=False)
        monkeypatch.delenv("RT_SLAB_AXES", raising=False)


def slab_only(cones):
    q = cones[..., :3].astype(np.int64)
    l2 = (q * q).sum(axis=-1)
    return (cones[..., 3] == 127) & (l2 > 0) & (l2 <= 126 * 126)


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
@pytest.mark.parametrize("name", SCENES)
def test_same_frame_no_more_work(dev, tmp_path, monkeypatch, name, prec):
    hs = make_scene(name, tmp_path)
    on, st_on = render(hs, prec, monkeypatch)
    parent, st_parent = render(hs, prec, monkeypatch, axes=False)
    no_step, _ = render(hs, prec, monkeypatch, slabs=0, stats=False)
    mega, _ = render(hs, prec, monkeypatch, pipeline=api.RT_PIPELINE_MEGAKERNEL, stats=False)
    print(f"{name} {prec}: mesh rays {st_on.mesh_rays}, node visits {st_parent.node_visits} -> {st_on.node_visits}, "
          f"triangle tests {st_parent.tri_tests} -> {st_on.tri_tests}")
    assert_same_bits(on, parent, "slab axes vs RT_SLAB_AXES=0")
    assert_same_bits(on, no_step, "slab axes vs RT_WF_SLABS=0")
    assert_same_bits(on, mega, "wavefront vs megakernel")
    assert st_on.mesh_rays == st_parent.mesh_rays > 0
    if prec == "f32":   # no f32 form of the slab step: the words are not read
        assert (st_on.node_visits, st_on.tri_tests) == (st_parent.node_visits, st_parent.tri_tests)
    else:
        assert st_on.node_visits <= st_parent.node_visits and st_on.tri_tests <= st_parent.tri_tests
        if name == "stand_in":
            assert st_on.node_visits < st_parent.node_visits


def knot_scene(d, moved):
    """scenes/cornell_dragon with the 40 x 40 stand-in surface, as it is or with every vertex moved smoothly and non-rigidly."""
    d.mkdir(exist_ok=True)
    obj = d / "knot.obj"
    subprocess.run([os.path.join(REPO, "tools", "gen_dragon"), str(obj), "40", "40"], check=True)
    if moved:
        displaced_obj(obj, d / "moved.obj", amplitude=0.25)
    text = open(os.path.join(REPO, "scenes", "cornell_dragon")).read().replace("resource/dragon_high.obj", "moved.obj" if moved else "knot.obj")
    (d / "cornell_dragon").write_text(text)
    return api.HostScene([str(d / "cornell_dragon"), "-w=96", "-s=16", "--seed=42"])


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_axes_follow_a_scene_update(dev, tmp_path, monkeypatch, prec):
    f32 = prec == "f32"
    a, b = knot_scene(tmp_path / "a", False), knot_scene(tmp_path / "b", True)
    monkeypatch.delenv("RT_SLAB_AXES", raising=False)
    before, after = api.scene_refit_mesh(a.desc, a.desc, 0, f32), api.scene_refit_mesh(a.desc, b.desc, 0, f32)
    sb, sa = slab_only(before["cones"]), slab_only(after["cones"])
    assert sb.any() and sa.any()
    assert (sb != sa).any() or (before["cones"][sb & sa] != after["cones"][sb & sa]).any(), "the move leaves every axis choice as it was"
    monkeypatch.setenv("RT_WF_SLABS", "1")
    p = a.params.copy()
    p.pipeline = api.RT_PIPELINE_WAVEFRONT
    p.precision = PRECISIONS[prec]
    scene = api.DeviceScene(a.desc, 0)
    try:
        scene.render(a.camera, p)                       # this precision is on the device: the update runs the refit kernels
        assert scene.update(b.desc)["n_meshes_refit"] == 1
        np.testing.assert_array_equal(scene.debug_mesh(0, f32)["cones"], after["cones"])
        by_kernels = scene.debug_mesh_digest(f32)
        updated = scene.render(b.camera, p)
    finally:
        scene.close()
    host = api.DeviceScene(a.desc, 0)                   # updated before anything is on the device: the host builder's tables
    try:
        host.update(b.desc)
        by_host = host.debug_mesh_digest(f32)
    finally:
        host.close()
    names = ("BvhNode", "BvhNode4f", "MeshNode4qc", "TriRec", "TriAttr", "mesh_bounds", "MeshOpRec")
    assert dict(zip(names, by_kernels)) == dict(zip(names, by_host))
    fresh, _ = render(b, prec, monkeypatch, stats=False)
    fresh_parent, _ = render(b, prec, monkeypatch, axes=False, stats=False)
    assert_same_bits(updated, fresh, "updated vs fresh")
    assert_same_bits(updated, fresh_parent, "updated vs fresh with RT_SLAB_AXES=0")
