"""k_wf_mesh with the back-face cone test (default) against the same library without it (RT_WF_CONES=0: every ray carries
the direction word that culls nothing).  A child is only skipped when the triangle test would have rejected every triangle
below it, so the two frames must be the same bits, NaN pixels included, whatever the mesh and its transform look like; the
counters must show that the test does cull - and that it does not for a mesh that hits back faces.  The oracle comparisons of
tests/test_gpu_parity.py (which run with the cones on) are the parity check proper; here the f64 frames of the meshes that
suite does not have are compared with the oracle as well."""
import numpy as np
import pytest

from oracle import pyoracle
from rust_raytracer_amd import api
from test_mesh_cones import degenerate_obj

pytestmark = pytest.mark.gpu

PRECISIONS = {"f64": api.RT_PRECISION_F64, "f32": api.RT_PRECISION_F32}


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


def render_both(hs, prec, monkeypatch, multi=False):
    """{"on" / "off": (frame, stats)} of the wavefront scheduler with counters, cones on (default) and RT_WF_CONES=0."""
    p = hs.params.copy()
    p.pipeline = api.RT_PIPELINE_WAVEFRONT
    p.precision = PRECISIONS[prec]
    p.collect_stats = 1
    if multi:
        monkeypatch.setenv("RT_WF_MESH_MULTI", "1")  # the general form of k_wf_mesh on a single-mesh scene
    out = {}
    for side in ("off", "on"):
        if side == "off":
            monkeypatch.setenv("RT_WF_CONES", "0")
        else:
            monkeypatch.delenv("RT_WF_CONES", raising=False)
        scene = api.DeviceScene(hs.desc, 0)
        frame = scene.render(hs.camera, p)
        st = scene.stats()
        out[side] = (frame, st)
        assert st.pipeline_used == api.RT_PIPELINE_WAVEFRONT and st.mesh_rays > 0 and st.tri_tests > 0
        scene.close()
    if multi:
        monkeypatch.delenv("RT_WF_MESH_MULTI")
    return out


def assert_same_bits(out):
    a, b = out["on"][0], out["off"][0]
    assert a.shape == b.shape
    assert (a.view(np.uint64) == b.view(np.uint64)).all(), \
        f"{int((a.view(np.uint64) != b.view(np.uint64)).any(axis=2).sum())} pixels differ between cones on and RT_WF_CONES=0"
    assert out["on"][1].mesh_rays == out["off"][1].mesh_rays


def assert_oracle(hs, frame):
    ref, _ = pyoracle.render(hs.desc, hs.camera, hs.params)
    a, b = frame[..., :3], ref[..., :3]
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    fin = ~np.isnan(b)
    assert (np.abs(a[fin] - b[fin]) <= np.maximum(1e-12 * np.abs(b[fin]), 1e-15)).all()   # the bar of tests/test_gpu_parity.py


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
@pytest.mark.parametrize("multi", [False, True])
def test_light_test_same_frame_less_work(dev, monkeypatch, prec, multi):
    hs = api.HostScene(["scenes/light_test", "-w=96", "-s=16", "--seed=31"])
    out = render_both(hs, prec, monkeypatch, multi=multi)
    assert_same_bits(out)
    on, off = out["on"][1], out["off"][1]
    print(f"light_test {prec} multi={multi}: node visits {off.node_visits} -> {on.node_visits}, triangle tests {off.tri_tests} -> {on.tri_tests}")
    assert on.tri_tests < off.tri_tests and on.node_visits < off.node_visits


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_two_meshes_same_frame(dev, monkeypatch, prec):
    hs = api.HostScene(["tests/scenes/two_meshes", "-w=64", "-s=16", "--seed=32"])
    out = render_both(hs, prec, monkeypatch)
    assert_same_bits(out)
    assert out["on"][1].tri_tests < out["off"][1].tri_tests


def bumpy_grid_obj(path, n, offset, scale, flat=False):
    """The mesh of test_quantised_bvh_nodes_on_awkward_meshes (tests/test_gpu_parity.py): an n x n grid of quads over
    [-1, 1]^2 with a sine bump, scaled per axis and moved."""
    lines = ["vt 0 0"]
    for j in range(n + 1):
        for i in range(n + 1):
            x, z = -1 + 2 * i / n, -1 + 2 * j / n
            y = 0.0 if flat else float(0.25 * np.sin(3.1 * x) * np.cos(2.3 * z) + 0.05 * np.sin(17 * x + 5 * z))
            lines.append(f"v {x * scale[0] + offset[0]!r} {y * scale[1] + offset[1]!r} {z * scale[2] + offset[2]!r}")
            lines.append("vn 0 1 0")
    idx = lambda i, j: j * (n + 1) + i + 1
    for j in range(n):
        for i in range(n):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            lines.append(f"f {a}/1/{a} {c}/1/{c} {b}/1/{b}")
            lines.append(f"f {a}/1/{a} {d}/1/{d} {c}/1/{c}")
    path.write_text("\n".join(lines) + "\n")


def grid_scene(tmp_path, obj_name, offset, s, cam, target, xform=None):
    lx, ly, lz = offset[0] - 0.5 * s, offset[1] + 2.0 * s, offset[2] - 0.5 * s
    scene = tmp_path / "scene"
    mesh = f"mesh {obj_name} (glossy (constant 0.7,0.6,0.3) (constant 0.3))"
    if xform:
        mesh = f"transform ({mesh}) {xform}"
    scene.write_text(f"@config output_width = 40\n@config aspect_ratio = 1\n@config focal_length = 40\n"
                     f"@config camera_pos = {cam}\n@config camera_target = {target}\n"
                     f"grid: {mesh}\n"
                     f"lamp: plane {lx!r},{ly!r},{lz!r} {s!r},0,0 0,0,{s!r} (emissive (constant 8,8,8)) backface\n"
                     f"sky: sky (constant 0.3,0.4,0.6)\nworld: list $grid $lamp $sky\nlights: list $lamp\n")
    return api.HostScene([str(scene), "-s=16", "--seed=21"])


AWKWARD = {
    "far_from_origin": ((1000.0, 0.0, -2000.0), (1.0, 1.0, 1.0), "1000,1.5,-1997", "1000,0,-2000"),
    "anisotropic": ((0.0, 0.0, 0.0), (50.0, 0.02, 1.0), "0,20,30", "0,0,0"),
    "flat": ((0.0, 0.25, 0.0), (1.0, 1.0, 1.0), "0,1.5,3", "0,0.25,0"),
    "tiny": ((0.0, 0.0, 0.0), (0.02, 0.02, 0.02), "0,0.03,0.06", "0,0,0"),
}


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
@pytest.mark.parametrize("case", sorted(AWKWARD))
def test_awkward_meshes_same_frame(dev, tmp_path, monkeypatch, case, prec):
    offset, scale, cam, target = AWKWARD[case]
    bumpy_grid_obj(tmp_path / "grid.obj", 24, offset, scale, flat=(case == "flat"))
    hs = grid_scene(tmp_path, "grid.obj", offset, max(scale), cam, target)
    assert_same_bits(render_both(hs, prec, monkeypatch))


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_degenerate_triangles_same_frame(dev, tmp_path, monkeypatch, prec):
    """A zero-area triangle, a sliver and two coincident triangles of opposite winding in a well-shaped mesh
    (tests/test_mesh_cones.py)."""
    degenerate_obj(tmp_path / "deg.obj")
    hs = grid_scene(tmp_path, "deg.obj", (0.0, 0.0, 0.0), 1.0, "0,1.5,3", "0,0,0")
    out = render_both(hs, prec, monkeypatch)
    assert_same_bits(out)
    if prec == "f64":
        assert_oracle(hs, out["on"][0])


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
@pytest.mark.parametrize("xform", ["s=3,0.5,1.5 ry=25 t=0.2,0.1,0", "s=1,-1,1 t=0,0.4,0", "s=-2,0.7,1 rx=20"])
def test_scaled_and_mirrored_mesh_same_frame(dev, tmp_path, monkeypatch, prec, xform):
    """Non-uniform scales and mirrorings: the winding seen in world space flips under a mirroring, the object-space
    test (and the cones, which live in object space) does not."""
    bumpy_grid_obj(tmp_path / "grid.obj", 24, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    hs = grid_scene(tmp_path, "grid.obj", (0.0, 0.5, 0.0), 2.0, "0,2.5,5", "0,0,0", xform=xform)
    out = render_both(hs, prec, monkeypatch)
    assert_same_bits(out)
    if prec == "f64":
        assert_oracle(hs, out["on"][0])


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
@pytest.mark.parametrize("multi", [False, True])
def test_mesh_that_hits_back_faces_is_never_culled(dev, tmp_path, monkeypatch, prec, multi):
    """RT_MESH_HIT_BACK_FACES tests |det|: no child may be skipped, so the counters are those of RT_WF_CONES=0; the frame
    is the oracle's, which honours the flag.  The mesh is the grid seen from its back (mirrored in y), where the flag decides
    whether the camera sees it at all."""
    bumpy_grid_obj(tmp_path / "grid.obj", 24, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    hs = grid_scene(tmp_path, "grid.obj", (0.0, 0.5, 0.0), 2.0, "0,2.5,5", "0,0,0", xform="s=1,-1,1 t=0,0.4,0")
    front_only, _ = pyoracle.render(hs.desc, hs.camera, hs.params)
    assert hs.desc.contents.n_meshes == 1
    hs.desc.contents.meshes[0].flags |= api.RT_MESH_HIT_BACK_FACES
    both_sides, _ = pyoracle.render(hs.desc, hs.camera, hs.params)
    assert (front_only != both_sides).any(axis=2).mean() > 0.1   # the flag matters in this scene
    out = render_both(hs, prec, monkeypatch, multi=multi)
    assert_same_bits(out)
    on, off = out["on"][1], out["off"][1]
    assert on.tri_tests == off.tri_tests and on.node_visits == off.node_visits
    if prec == "f64":
        assert_oracle(hs, out["on"][0])
