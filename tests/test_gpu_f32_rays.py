"""f32 ray hits on the GPU held to per-ray bounds against the CPU oracle (tests/f32_ray_bounds.py has the rule and its
derivation; tests/test_f32_ray_bounds_host.py shows that the rule fails what it must fail).

(a) the ray sets of tests/ray_query_cases.py on its eight oracle scenes;
(b) short directions: camera rays plus lifted follow-ups and the segments of two_meshes, light_test and sphere_field with every
    direction scaled by 2^-10 and 2^-20 - the triangle and quad tests compare a determinant proportional to |d| with an absolute
    constant, which in f32 used to be FLT_EPSILON.  At 2^-20 the oracle's hits fall below that old threshold and the parent's
    kernels lose them; at 2^-10 NONE of these scenes' hits does (asserted), so that half passes on the parent as well and
    checks only that the f32 answers do not depend on |d|;
(c) small units under a transform: a mesh in 0.02-unit coordinates placed with s=50 (object-space 2 area ~ 3.3e-6), as ray
    queries under every kernel plan and as an f32 render against the oracle;
(d) the megakernel's search (world_test<float>, resolve_hit<float>) vertex by vertex through rt_debug_trace_sample.
Every test prints its excused share and its ratios before it asserts, and asserts on the oracle's answers alone that it is
not vacuous."""
import numpy as np
import pytest

from oracle import pyoracle
from rust_raytracer_amd import api
from ray_query_cases import ENVIRONMENT, SURFACE, oracle_hits
import f32_ray_bounds as fb

pytestmark = pytest.mark.gpu

F32 = api.RT_PRECISION_F32
ORACLE_SCENES = ["cornell", "two_meshes", "nested_transform", "sun_sky", "sphere_field", "hollow_glass", "light_test", "texture_mix"]


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


_scenes = {}


def device_scene(rs):
    """One DeviceScene per description for the whole module (queries leave a scene as it was)."""
    key = id(rs.hs)
    if key not in _scenes:
        _scenes[key] = (rs.hs, api.DeviceScene(rs.hs.desc, 0))
    return _scenes[key][1]


def run_yardstick(rs):
    scene = device_scene(rs)
    got = scene.trace_rays(rs.o, rs.d, precision=F32)
    assert scene.ray_query_stats().precision == F32
    occ = scene.occluded(rs.seg_o, rs.seg_d, rs.seg_lo, rs.seg_hi, precision=F32)
    closest, segments = rs.closest(got), rs.occlusion(occ)
    print(closest.line())    # both lines before either assertion
    print(segments.line())
    closest.check(show=False)
    segments.check(show=False)
    return got, occ


# ---- (a) the existing ray sets ----
@pytest.mark.parametrize("name", ORACLE_SCENES)
def test_existing_scenes(dev, name):
    rs = fb.scene_set(name)
    rs.assert_not_vacuous(mesh=100 if name == "two_meshes" else 0)
    run_yardstick(rs)
    if name == "sun_sky":
        assert (rs.hits["klass"] == ENVIRONMENT).any()


# ---- (b) short directions ----
@pytest.mark.parametrize("log2_scale", [-10, -20])
@pytest.mark.parametrize("name", ["two_meshes", "light_test", "sphere_field"])
def test_short_directions(dev, name, log2_scale):
    rs = fb.short_set(name, log2_scale)
    rs.assert_not_vacuous(mesh={"two_meshes": 100, "light_test": 30, "sphere_field": 0}[name])
    tri, quad = rs.small_det_hits()
    if log2_scale == -10:
        # no hit of these scenes has a determinant below FLT_EPSILON at this scale: this half cannot see the old threshold (it
        # passes with FLT_EPSILON as well); what it holds is that the f32 answers are those of the unscaled rays
        assert (tri, quad) == (0, 0)
    # 2^-20, determinants below FLT_EPSILON: at least 100 mesh hits on two_meshes; light_test has 41 mesh hits at 24 pixels
    # (its oracle costs 4.5 ms a ray: a wider frame would take this test beyond a few seconds), all of them; sphere_field has
    # no mesh (it holds sphere_test to the same rays) but some quads
    elif name == "two_meshes":
        assert tri >= 100
    elif name == "light_test":
        assert tri == rs.mesh_hits() >= 30
    else:
        assert quad >= 10
    run_yardstick(rs)


# ---- (c) small units under a transform ----
def test_scaled_grid_queries(dev, monkeypatch):
    rs = fb.grid_set()
    assert len(rs.o) == 881 and len(rs.seg_o) == 305
    rs.assert_not_vacuous(mesh=300)
    assert rs.small_det_hits()[0] >= 100
    got, occ = run_yardstick(rs)
    scene = device_scene(rs)
    for switch in ("RT_WF_SPLIT=0", "RT_WF_GROUPS=0", "RT_WF_NODES=0", "RT_WF_MESH_MULTI=1"):
        key, value = switch.split("=")
        monkeypatch.setenv(key, value)
        assert scene.trace_rays(rs.o, rs.d, precision=F32).tobytes() == got.tobytes(), switch
        np.testing.assert_array_equal(scene.occluded(rs.seg_o, rs.seg_d, rs.seg_lo, rs.seg_hi, precision=F32), occ)
        monkeypatch.delenv(key)


@pytest.fixture(scope="module")
def grid_render():
    hs = api.HostScene([fb.grid_scene_path(), "-w=40", "-s=64", "--seed=21"])
    ref, _ = pyoracle.render(hs.desc, hs.camera, hs.params)
    return hs, ref


@pytest.mark.parametrize("pipeline", ["mega", "wavefront"])
def test_scaled_grid_render(dev, grid_render, pipeline):
    """The f32 frame at the f32 bar of tests/test_gpu_parity.py.  Without the mesh in the indirect rays the image mean moves
    by far more than 1 %."""
    hs, ref = grid_render
    p = hs.params.copy()
    p.precision = F32
    p.pipeline = {"mega": api.RT_PIPELINE_MEGAKERNEL, "wavefront": api.RT_PIPELINE_WAVEFRONT}[pipeline]
    gpu = api.DeviceScene(hs.desc, 0).render(hs.camera, p)
    a, b = gpu[..., :3], ref[..., :3]
    assert np.isfinite(b).all() and b.std() > 0.01
    assert not np.isnan(a).any()
    close = np.abs(a - b) <= np.maximum(0.05 * np.abs(b), 0.02)
    print(f"scaled_grid {pipeline}: mean {a.mean():.6f} against {b.mean():.6f}, {close.mean():.3%} of values close")
    assert abs(a.mean() - b.mean()) <= 0.01 * b.mean()
    assert close.mean() >= 0.95, f"only {close.mean():.3%} of f32 values are close to the f64 oracle"


# ---- (d) the megakernel's search, vertex by vertex ----
@pytest.mark.parametrize("name", ["two_meshes", "nested_transform", "scaled_grid"])
def test_megakernel_vertices(dev, name):
    """Every recorded bounce of about 60 samples: the recorded ray taken as given, its t, position, material and normal held to
    pyoracle.world_hit for that ray.  Paths are not compared."""
    rs = fb.grid_set() if name == "scaled_grid" else fb.scene_set(name)
    scene = device_scene(rs)
    hs = rs.hs
    p = hs.params.copy()
    p.precision = F32
    rows = []
    w, h = hs.width, hs.height
    for k in range(60):
        x, y = (7 * k + 3) % w, (5 * k + h // 3) % h
        _, tr = scene.trace_sample(hs.camera, p, 0, x, y, 0, 0, max_bounces=16)
        rows.append(tr)
    tr = np.concatenate(rows)
    o, d = np.ascontiguousarray(tr[:, 11:14]), np.ascontiguousarray(tr[:, 14:17])
    want = oracle_hits(hs.desc, o, d)
    mesh_mats = {e["material"] for e in rs.geom.entries if e["type"] == api.RT_NODE_MESH}
    assert (want["klass"] == SURFACE).sum() >= 30
    assert ((want["klass"] == SURFACE) & np.isin(want["material"], list(mesh_mats))).sum() >= 15
    got = fb.vertex_records(rs.geom, tr[:, 0], tr[:, 1:4], tr[:, 4], tr[:, 8:11])
    fb.check_closest(rs.geom, o, d, got, want, rs.extent, name + " megakernel vertices", face=False, uv=False).check()
