"""rt_scene_update on the GPU: a scene updated in place (mesh BVHs refitted by the kernels of rt_refit.hip, everything else
recompiled on the host) must behave as a scene freshly created from the new description.  Frames are compared bit for bit
("same bits": equal as uint64 everywhere, NaN pixels included) against a fresh DeviceScene, f64 frames against the oracle at
the bar of tests/test_gpu_parity.py, and the device's mesh tables against the refit on the CPU (api.scene_refit_mesh: the
reused tree with the new vertices, through the derivation of rt_tables.cpp that DeviceScene<R>::build uploads)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from rust_raytracer_amd import api
from scene_update_cases import (ATTR_CASE, GRID_CASES, MONKEY, REPO, displaced_obj, grid_host_scene, same_bits, smoke_variant, two_meshes_variant)

pytestmark = pytest.mark.gpu

PRECISIONS = {"f64": api.RT_PRECISION_F64, "f32": api.RT_PRECISION_F32}
PIPELINES = {"wavefront": api.RT_PIPELINE_WAVEFRONT, "megakernel": api.RT_PIPELINE_MEGAKERNEL}


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


def params_of(hs, prec="f64", pipe="wavefront", stats=False):
    p = hs.params.copy()
    p.precision = PRECISIONS[prec]
    p.pipeline = PIPELINES[pipe]
    p.collect_stats = int(stats)
    return p


def fresh_frame(hs, prec="f64", pipe="wavefront"):
    scene = api.DeviceScene(hs.desc, 0)
    try:
        return scene.render(hs.camera, params_of(hs, prec, pipe))
    finally:
        scene.close()


def assert_same_bits(a, b, what=""):
    assert a.shape == b.shape
    assert same_bits(a, b), f"{what}: {int((a.view(np.uint64) != b.view(np.uint64)).any(axis=2).sum())} pixels differ"


def assert_oracle(hs, frame):
    ref, _ = pyoracle.render(hs.desc, hs.camera, hs.params)
    a, b = frame[..., :3], ref[..., :3]
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    fin = ~np.isnan(b)
    assert (np.abs(a[fin] - b[fin]) <= np.maximum(1e-12 * np.abs(b[fin]), 1e-15)).all()   # the bar of tests/test_gpu_parity.py


def two_meshes(tmp_path=None):
    return api.HostScene(["tests/scenes/two_meshes", "-w=64", "-s=16", "--seed=32"])


# ---- G1 ----
@pytest.mark.parametrize("pipe", sorted(PIPELINES))
@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_transforms_and_materials_only(dev, tmp_path, prec, pipe):
    a, b = two_meshes(), two_meshes_variant(tmp_path, "numbers")
    scene = api.DeviceScene(a.desc, 0)
    first = scene.render(a.camera, params_of(a, prec, pipe))
    info = scene.update(b.desc)
    assert info["n_meshes_refit"] == 0 and info["n_triangles_refit"] == 0 and info["refit_kernel_ms"] == 0.0
    assert 0 < info["bytes_uploaded"] < 1 << 20
    frame = scene.render(b.camera, params_of(b, prec, pipe))
    scene.close()
    want = fresh_frame(b, prec, pipe)
    assert_same_bits(frame, want, "updated vs fresh")
    assert not same_bits(first, frame)
    if prec == "f64":
        assert_oracle(b, frame)


# ---- G2 ----
@pytest.mark.parametrize("prec", sorted(PRECISIONS))
@pytest.mark.parametrize("case", GRID_CASES + (ATTR_CASE,))
def test_deformed_mesh(dev, tmp_path, case, prec):
    a = grid_host_scene(tmp_path, "base", view=case)   # the camera of b: only the mesh differs
    b = grid_host_scene(tmp_path, case)
    scene = api.DeviceScene(a.desc, 0)
    before = scene.render(a.camera, params_of(a, prec))
    info = scene.update(b.desc)
    assert info["n_meshes_refit"] == 1 and info["n_triangles_refit"] == 1152 and info["refit_kernel_ms"] > 0.0
    frame = scene.render(b.camera, params_of(b, prec))
    scene.close()
    assert_same_bits(frame, fresh_frame(b, prec), "refitted vs fresh")
    if case == ATTR_CASE:
        assert not same_bits(before, frame)      # the new vertex normals are seen
    assert np.isfinite(frame[..., :3]).all() and frame[..., :3].max() > 0
    if prec == "f64" and case in ("phase", "fold_twist", "collapsed", ATTR_CASE):
        assert_oracle(b, frame)


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_cones_survive_the_refit_and_only_cull(dev, tmp_path, monkeypatch, prec):
    a, b = grid_host_scene(tmp_path, "base"), grid_host_scene(tmp_path, "phase")
    out = {}
    for side in ("off", "on"):
        if side == "off":
            monkeypatch.setenv("RT_WF_CONES", "0")
        else:
            monkeypatch.delenv("RT_WF_CONES", raising=False)
        scene = api.DeviceScene(a.desc, 0)
        scene.render(a.camera, params_of(a, prec))
        scene.update(b.desc)
        out[side] = (scene.render(b.camera, params_of(b, prec, stats=True)), scene.stats())
        scene.close()
    assert_same_bits(out["on"][0], out["off"][0], "cones on vs RT_WF_CONES=0")
    assert out["on"][1].mesh_rays == out["off"][1].mesh_rays > 0
    assert out["on"][1].tri_tests < out["off"][1].tri_tests


# ---- G3 ----
def assert_same_tables(got, want):
    for key in ("children", "cones", "order"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert (got["boxes"].view(np.uint32) == want["boxes"].view(np.uint32)).all(), "boxes"
    assert (got["tris"].view(np.uint64) == want["tris"].view(np.uint64)).all(), "tris"


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", ["phase", "fold_twist", "far", "collapsed", ATTR_CASE])
def test_device_tables_are_the_restatement(dev, tmp_path, case, f32):
    prec = "f32" if f32 else "f64"
    a, b = grid_host_scene(tmp_path, "base"), grid_host_scene(tmp_path, case)
    scene = api.DeviceScene(a.desc, 0)
    assert_same_tables(scene.debug_mesh(0, f32), api.scene_refit_mesh(a.desc, a.desc, 0, f32))   # a fresh scene: the builder's tables
    scene.update(b.desc)                                                                           # kernels, this precision
    assert_same_tables(scene.debug_mesh(0, f32), api.scene_refit_mesh(a.desc, b.desc, 0, f32))
    # every mesh table, all bytes: refitted by the kernels vs derived by the host builder from the same tree and vertices
    # (a scene updated before anything was on the device materialises through DeviceScene<R>::build)
    by_kernels = scene.debug_mesh_digest(f32)
    scene.close()
    host = api.DeviceScene(a.desc, 0)
    host.update(b.desc)
    by_host = host.debug_mesh_digest(f32)
    host.close()
    names = ("BvhNode", "BvhNode4f", "MeshNode4qc", "TriRec", "TriAttr", "mesh_bounds", "MeshOpRec", "updates")
    assert dict(zip(names, by_kernels)) == dict(zip(names, by_host)), prec


# ---- G4 ----
@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_one_of_two_meshes(dev, tmp_path, prec):
    displaced_obj(MONKEY, tmp_path / "moved.obj")
    a, b = two_meshes(), two_meshes_variant(tmp_path, "m2_moved", numeric=False, m2=tmp_path / "moved.obj")
    scene = api.DeviceScene(a.desc, 0)
    first = scene.render(a.camera, params_of(a, prec))
    info = scene.update(b.desc)
    assert info["n_meshes_refit"] == 1 and info["n_triangles_refit"] == b.desc.contents.meshes[1].n_triangles
    frame = scene.render(b.camera, params_of(b, prec))
    scene.close()
    assert_same_bits(frame, fresh_frame(b, prec), "refitted vs fresh")
    assert not same_bits(first, frame)


# ---- G5 ----
@pytest.mark.parametrize("pipe", sorted(PIPELINES))
def test_mesh_boundary_of_a_volume(dev, tmp_path, pipe):
    """tests/scenes/smoke: the combined intersect kernel and the megakernel read the BVH2 (BvhNode<R>)."""
    displaced_obj(MONKEY, tmp_path / "moved.obj", amplitude=0.1)
    a = api.HostScene(["tests/scenes/smoke", "-w=48", "-s=16", "--seed=5"])
    b = smoke_variant(tmp_path, "smoke_b", tmp_path / "moved.obj")
    for prec in sorted(PRECISIONS):
        scene = api.DeviceScene(a.desc, 0)
        scene.render(a.camera, params_of(a, prec, pipe))
        assert scene.update(b.desc)["n_meshes_refit"] == 1
        frame = scene.render(b.camera, params_of(b, prec, pipe))
        scene.close()
        assert_same_bits(frame, fresh_frame(b, prec, pipe), f"{prec} refitted vs fresh")
        if prec == "f64":
            assert_oracle(b, frame)


# ---- G6 ----
@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_no_drift(dev, tmp_path, prec):
    a, b, c = (grid_host_scene(tmp_path, k) for k in ("base", "fold_twist", "phase"))
    scene = api.DeviceScene(a.desc, 0)
    first = scene.render(a.camera, params_of(a, prec))
    scene.update(b.desc)
    scene.update(a.desc)
    assert_same_bits(scene.render(a.camera, params_of(a, prec)), first, "a -> b -> a")
    scene.update(b.desc)
    scene.update(c.desc)
    assert_same_bits(scene.render(c.camera, params_of(c, prec)), fresh_frame(c, prec), "a -> b -> a -> b -> c vs fresh c")
    scene.close()


# ---- G7 ----
def test_lazy_precision(dev, tmp_path):
    a, b = grid_host_scene(tmp_path, "base"), grid_host_scene(tmp_path, "phase")
    want = {prec: fresh_frame(b, prec) for prec in PRECISIONS}
    scene = api.DeviceScene(a.desc, 0)           # nothing on the device yet
    info = scene.update(b.desc)
    assert info["n_meshes_refit"] == 1 and info["refit_kernel_ms"] == 0.0
    for prec in ("f32", "f64"):
        assert_same_bits(scene.render(b.camera, params_of(b, prec)), want[prec], f"update first, then {prec}")
    scene.close()
    scene = api.DeviceScene(a.desc, 0)           # f64 only before the update: f32 is built from the updated host tables
    scene.render(a.camera, params_of(a, "f64"))
    assert scene.update(b.desc)["refit_kernel_ms"] > 0.0
    for prec in ("f32", "f64"):
        assert_same_bits(scene.render(b.camera, params_of(b, prec)), want[prec], f"f64, update, then {prec}")
    scene.close()


def test_both_precisions_on_the_device(dev, tmp_path):
    """f32 and f64 both materialised: the two typed refits run one after the other over the mesh's shared scratch."""
    a, b = grid_host_scene(tmp_path, "base"), grid_host_scene(tmp_path, "fold_twist")
    scene = api.DeviceScene(a.desc, 0)
    for prec in ("f32", "f64"):
        scene.render(a.camera, params_of(a, prec))
    assert scene.update(b.desc)["refit_kernel_ms"] > 0.0
    host = api.DeviceScene(a.desc, 0)             # tables derived by the host builder from the same tree and vertices
    host.update(b.desc)
    for prec in ("f64", "f32"):
        assert_same_bits(scene.render(b.camera, params_of(b, prec)), fresh_frame(b, prec), f"both on the device, {prec}")
        assert scene.debug_mesh_digest(prec == "f32") == host.debug_mesh_digest(prec == "f32"), prec
    scene.close()
    host.close()


# ---- G8 ----
def test_other_entry_points(dev, tmp_path):
    a, b = grid_host_scene(tmp_path, "base"), grid_host_scene(tmp_path, "phase")
    p = params_of(b)
    scene, fresh = api.DeviceScene(a.desc, 0), api.DeviceScene(b.desc, 0)
    scene.render(a.camera, params_of(a))
    scene.update(b.desc)
    assert same_bits(scene.render_aov(b.camera, p), fresh.render_aov(b.camera, p))
    groups = api.light_groups_auto(b.desc, has_background=bool(p.has_background))
    got, want = scene.render_light_groups(b.camera, p, groups), fresh.render_light_groups(b.camera, p, groups)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    frame = fresh.render(b.camera, p)
    prog = api.ProgressiveRender(scene, b.camera, p)
    while not prog.finished:
        prog.render(3)
    assert same_bits(prog.estimate(), frame)
    prog.close()
    rgb, trace = scene.trace_sample(b.camera, p, 0, 20, 20, 0, 0)
    rgb2, trace2 = fresh.trace_sample(b.camera, p, 0, 20, 20, 0, 0)
    keep = [c for c in range(17) if c != 6]      # column 6 is the triangle's leaf slot: the one thing that names the tree
    assert same_bits(rgb, rgb2) and same_bits(np.ascontiguousarray(trace[:, keep]), np.ascontiguousarray(trace2[:, keep]))
    scene.close()
    fresh.close()


# ---- G9 ----
def test_refusals_leave_the_scene_alone(dev, tmp_path):
    a = two_meshes()
    scene = api.DeviceScene(a.desc, 0)
    first = scene.render(a.camera, params_of(a))
    generation = scene.debug_mesh_digest()[7]
    bad = two_meshes()
    bad.desc.contents.meshes[0].n_triangles -= 1
    with pytest.raises(api.RtError) as e:
        scene.update(bad.desc)
    assert e.value.status == api.RT_E_INVALID and "meshes[0].n_triangles" in str(e.value)
    assert_same_bits(scene.render(a.camera, params_of(a)), first, "after a refused structure")
    proj = two_meshes()
    proj.desc.contents.transforms[0].m[12] = 0.25     # a projective last row
    with pytest.raises(api.RtError) as e:
        scene.update(proj.desc)
    assert e.value.status == api.RT_E_UNSUPPORTED
    with pytest.raises(api.RtError) as e:
        api.DeviceScene(proj.desc, 0)
    assert e.value.status == api.RT_E_UNSUPPORTED     # as rt_scene_create
    huge = two_meshes()
    huge.desc.contents.meshes[1].positions[4] = 1e38
    with pytest.raises(api.RtError) as e:
        scene.update(huge.desc)
    assert e.value.status == api.RT_E_UNSUPPORTED
    nan = two_meshes()
    nan.desc.contents.meshes[1].positions[4] = float("nan")     # in the middle of the array
    with pytest.raises(api.RtError) as e:
        scene.update(nan.desc)
    assert e.value.status == api.RT_E_UNSUPPORTED
    assert scene.debug_mesh_digest()[7] == generation
    assert_same_bits(scene.render(a.camera, params_of(a)), first, "after four refusals")
    # an accumulator does not outlive an update
    b = two_meshes_variant(tmp_path, "numbers")
    old = api.ProgressiveRender(scene, a.camera, params_of(a))
    old.render(2)
    scene.update(b.desc)
    for call in (lambda: old.render(1), old.estimate, old.save_state):
        with pytest.raises(api.RtError) as e:
            call()
        assert e.value.status == api.RT_E_INVALID and "the scene was updated after this accumulator was created" in str(e.value)
    old.close()
    new = api.ProgressiveRender(scene, b.camera, params_of(b))
    while not new.finished:
        new.render(4)
    assert_same_bits(new.estimate(), fresh_frame(b), "a new accumulator")
    new.close()
    scene.close()


# ---- G10 ----
def test_cli_sequence(dev, tmp_path):
    rtrace = os.path.join(REPO, "rust_raytracer_amd", "rtrace")
    b = two_meshes_variant(tmp_path, "numbers")
    b.close()
    flags = ["-w=48", "-s=16", "--seed=3"]
    seq, alone = tmp_path / "seq", tmp_path / "alone"
    seq.mkdir()
    alone.mkdir()
    a_path = os.path.join(REPO, "tests", "scenes", "two_meshes")
    r = subprocess.run([rtrace, a_path, f"--sequence={tmp_path / 'numbers'}"] + flags, cwd=seq, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "meshes refit" in r.stdout + r.stderr
    r = subprocess.run([rtrace, str(tmp_path / "numbers")] + flags, cwd=alone, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (seq / "out_0001.png").read_bytes() == (alone / "out.png").read_bytes()
    r = subprocess.run([rtrace, a_path, f"--sequence={tmp_path / 'numbers'}", "--gpus=2"] + flags, cwd=seq, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--sequence" in r.stdout + r.stderr
