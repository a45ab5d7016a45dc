"""Primitive-group search on the GPU (OP_GROUP, group_search, k_wf_prims<GROUPS>) at its limits and offsets, held to the oracle
(tests/group_cases.py has the scenes and the ray sets; tests/test_group_cases_host.py shows that every scene sits on its side of
each limit, that the trees are whole and that the ray sets reach every primitive).

Two groups and three (every base of try_emit_group and derive_groups non-zero), a group under a transform with a non-uniform
scale and one BVH instanced twice (make_cull_ray on an object-space ray), the LDS stack at its bound of 16 levels and the
scene one sphere past it, the node limit of 384 from both sides, the launch with 65 552 B of dynamic LDS, tables left in global
memory by the 44 KB rule, a radius-1000 sphere among radius-0.2 ones and a group 4096 units from the origin."""
import numpy as np
import pytest

from oracle import pyoracle
from rust_raytracer_amd import api
from ray_query_cases import SURFACE, T_MIN, assert_hits_equal_oracle
from test_gpu_parity import assert_f64_parity
import f32_ray_bounds as fb
import group_cases as gc

pytestmark = pytest.mark.gpu

F32 = api.RT_PRECISION_F32
# no group BVHs, the combined intersect kernel, no tables in LDS, a prefix of them only
SWITCHES = ("RT_WF_GROUPS=0", "RT_WF_SPLIT=0", "RT_LDS_TABLES=0", "RT_LDS_BUDGET=1024")
PIPELINES = {"mega": api.RT_PIPELINE_MEGAKERNEL, "wavefront": api.RT_PIPELINE_WAVEFRONT}
FEWER_TESTS = ("lattice900", "nodes_at_limit", "two_groups", "instanced")   # the group form must save primitive tests here
WIDE_SCALES = ("ground", "stack16")


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


_scenes = {}


def device_scene(name):
    """One DeviceScene per scene for the whole module (queries and renders leave a scene as it was)."""
    if name not in _scenes:
        _scenes[name] = api.DeviceScene(gc.host_scene(name).desc, 0)
    return _scenes[name]


def frame(scene, name, pipeline=api.RT_PIPELINE_WAVEFRONT, stats=0):
    hs = gc.frame_scene(name)
    p = hs.params.copy()
    p.pipeline, p.collect_stats = pipeline, stats
    out = scene.render(hs.camera, p)
    assert out.shape == (32, 32, 4) and p.spp == 4
    return out


# ---- 1. f64 closest hits and occlusion ----
@pytest.mark.parametrize("name", gc.NAMES)
def test_closest_hits_and_occlusion_equal_oracle(dev, name):
    c = gc.case(name)
    scene = device_scene(name)
    got = scene.trace_rays(c.o, c.d)
    assert_hits_equal_oracle(got, c.want, c.desc, c.extent)
    # the node reported is the primitive on whose surface the hit lies
    surf = c.want["klass"] == SURFACE
    dist = c.surface_distance(got["node"][surf], got["pos"][surf])
    assert (dist <= c.tol()).all(), f"{int((dist > c.tol()).sum())} hits do not lie on the node they name"
    np.testing.assert_array_equal(scene.occluded(c.seg_o, c.seg_d, T_MIN, c.seg_hi), c.seg_occluded)


# ---- 2. the same bytes under every plan and with the reference's own tree ----
@pytest.mark.parametrize("name", gc.NAMES)
def test_same_bytes_under_every_switch(dev, monkeypatch, name):
    c = gc.case(name)
    scene = device_scene(name)
    hits, img = scene.trace_rays(c.o, c.d), frame(scene, name)
    for switch in SWITCHES:
        key, value = switch.split("=")
        monkeypatch.setenv(key, value)
        other, other_img = scene.trace_rays(c.o, c.d), frame(scene, name)
        monkeypatch.delenv(key)
        assert other.tobytes() == hits.tobytes(), f"{switch}: hit records differ"
        assert other_img.tobytes() == img.tobytes(), f"{switch}: frames differ"
    monkeypatch.setenv("RT_PRIM_REBUILD", "0")
    plain = api.DeviceScene(c.desc, 0)
    try:
        other, other_img = plain.trace_rays(c.o, c.d), frame(plain, name)
    finally:
        plain.close()
    assert other.tobytes() == hits.tobytes(), "RT_PRIM_REBUILD=0: hit records differ"
    assert other_img.tobytes() == img.tobytes(), "RT_PRIM_REBUILD=0: frames differ"


# ---- 3. f64 frames ----
_oracle_frames = {}


def oracle_frame(name):
    if name not in _oracle_frames:
        hs = gc.frame_scene(name)
        _oracle_frames[name] = pyoracle.render(hs.desc, hs.camera, hs.params)[0]
    return _oracle_frames[name]


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
@pytest.mark.parametrize("name", gc.NAMES)
def test_f64_frame_matches_oracle(dev, name, pipeline):
    scene = device_scene(name)
    gpu = frame(scene, name, PIPELINES[pipeline])
    assert scene.stats().pipeline_used == PIPELINES[pipeline]
    ref = oracle_frame(name)
    assert np.isfinite(ref[..., :3]).all() and ref[..., :3].mean() > 0.01      # lit
    assert_f64_parity(gpu, ref)


# ---- 4. which path ran ----
@pytest.mark.parametrize("name", gc.NAMES)
def test_group_form_runs_where_the_plan_admits_it(dev, monkeypatch, name):
    """prim_tests counts sphere and quad tests, not box tests: the op form tests every primitive whose skip-pointer boxes the
    ray passes, the group form only those in the leaves it reaches nearest first.  A scene over a limit keeps the op form, so
    RT_WF_GROUPS=0 changes nothing at all there."""
    scene = device_scene(name)
    img = frame(scene, name, stats=1)
    with_groups = scene.stats().prim_tests
    monkeypatch.setenv("RT_WF_GROUPS", "0")
    img_ops = frame(scene, name, stats=1)
    without = scene.stats().prim_tests
    print(f"{name}: prim_tests {with_groups} at the default switches, {without} under RT_WF_GROUPS=0")
    assert img.tobytes() == img_ops.tobytes()
    if name in gc.OP_FORM:
        assert with_groups == without
    elif name in FEWER_TESTS:
        assert with_groups < without
    # the other scenes: printed only.  The group form need not save a test there: a chain's quantised f32 boxes are wider than
    # the op form's f64 ones, and stack16 pays one test more (12 901 against 12 900)


# ---- 5. f32 ----
@pytest.mark.parametrize("name", gc.NAMES)
def test_f32_rule(dev, name):
    rs = gc.f32_set(name)
    rs.assert_not_vacuous()
    scene = device_scene(name)
    got = scene.trace_rays(rs.o, rs.d, precision=F32)
    assert scene.ray_query_stats().precision == F32
    seg = scene.occluded(rs.seg_o, rs.seg_d, rs.seg_lo, rs.seg_hi, precision=F32)
    closest, segments = rs.closest(got), rs.occlusion(seg)
    print(closest.line())
    print(segments.line())
    if name in WIDE_SCALES:
        # what the rule could excuse on the oracle alone bounds what it may excuse of the kernels' answers
        fragile = gc.fragile_shares(name)
        print(f"{name}: excused {closest.share:.2%} / {segments.share:.2%}, fragile on the oracle alone {fragile[0]:.2%} / {fragile[1]:.2%}")
        assert closest.share <= fragile[0] and segments.share <= fragile[1]
    closest.check(show=False)
    segments.check(show=False)
