"""The traversal stack of k_wf_mesh (MeshStack in csrc/rt_wavefront.h): the first RT_WF_LDS_LEVELS levels in LDS, deeper ones in
the spill buffer.  A wave pushes and pops without a spill test while a ballot says that every lane taking part is clear of the
spill part (three free LDS levels for the pushes of a node step, the whole stack in LDS for the pop loop), and entry by entry with
the test otherwise.  Which form a wave takes must not matter: the entries, their order and the entries culled on pop are the
same, so every frame here equals the megakernel's bit for bit and every counting render counts what the default setting counts
(node visits, triangle tests, mesh rays and the entries culled on pop).

RT_WF_LDS_LEVELS = 0: every entry spills; 1-3: the wave sits on the edge where only some lanes have three free levels; 4: most
waves mix both forms; 12: the default.  Scenes and sizes are those of tests/test_gpu_handout.py; one generated mesh is deep
enough that the default setting spills too.  Everything here needs the GPU."""
import re

import numpy as np
import pytest

from rust_raytracer_amd import api
from ray_query_cases import assert_hits_equal_oracle, cases

pytestmark = pytest.mark.gpu

SCENES = {
    "light_test": ["scenes/light_test", "-w=45", "-r=1.2162", "-s=9", "--seed=51"],   # 45 x 37; one mesh op: k_wf_mesh<MULTI = false>
    "two_meshes": ["tests/scenes/two_meshes", "-w=40", "-r=1", "-s=16", "--seed=52"],  # 40 x 40; the MULTI form
}
PRECISIONS = {"f64": api.RT_PRECISION_F64, "f32": api.RT_PRECISION_F32}
LEVELS = [0, 1, 2, 3, 4, 12]
DEFAULT_LEVELS = 12
SWITCH = "RT_WF_LDS_LEVELS"


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


_loaded = {}


def loaded(name, make=None):
    """Host scene, device scene and the references of a scene, computed once: per precision the megakernel's frame and the
    counters of a counting wavefront render at the default setting."""
    if name not in _loaded:
        hs = make() if make else api.HostScene(SCENES[name])
        _loaded[name] = (hs, api.DeviceScene(hs.desc, 0), {}, {})
    return _loaded[name]


def params(hs, precision, pipeline, stats=False):
    p = hs.params.copy()
    p.pipeline = pipeline
    p.precision = PRECISIONS[precision]
    p.collect_stats = int(stats)
    return p


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def megakernel_frame(name, precision):
    hs, scene, mega, _ = loaded(name)
    if precision not in mega:
        mega[precision] = scene.render(hs.camera, params(hs, precision, api.RT_PIPELINE_MEGAKERNEL))
    return mega[precision]


def wavefront(name, precision, monkeypatch, levels, capfd=None):
    """A lean render, or with `capfd` a counting one -> frame, (node_visits, tri_tests, mesh_rays, pops_culled).  The entries
    culled on pop are not part of RtRenderStats: the library prints them with RT_WF_DEBUG=1."""
    hs, scene, _, _ = loaded(name)
    if levels is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, str(levels))
    if capfd is None:
        frame = scene.render(hs.camera, params(hs, precision, api.RT_PIPELINE_WAVEFRONT))
        assert scene.stats().pipeline_used == api.RT_PIPELINE_WAVEFRONT
        return frame, None
    monkeypatch.setenv("RT_WF_DEBUG", "1")
    capfd.readouterr()
    frame = scene.render(hs.camera, params(hs, precision, api.RT_PIPELINE_WAVEFRONT, True))
    err = capfd.readouterr().err
    monkeypatch.delenv("RT_WF_DEBUG")
    st = scene.stats()
    assert st.pipeline_used == api.RT_PIPELINE_WAVEFRONT
    culled = re.search(r"stack entries culled on pop (\d+)", err)
    assert culled, f"no k_wf_mesh counter line in the library's RT_WF_DEBUG output: {err!r}"
    return frame, (st.node_visits, st.tri_tests, st.mesh_rays, int(culled.group(1)))


def default_counts(name, precision, monkeypatch, capfd):
    counts = loaded(name)[3]
    if precision not in counts:
        _, counts[precision] = wavefront(name, precision, monkeypatch, None, capfd)
        assert min(counts[precision]) > 0
    return counts[precision]


def assert_unchanged(name, precision, monkeypatch, capfd, levels):
    want = megakernel_frame(name, precision)
    frame, _ = wavefront(name, precision, monkeypatch, levels)
    differ = int((frame != want).any(axis=2).sum())
    assert same_bits(frame, want), f"{SWITCH}={levels}: {differ} pixels differ from the megakernel"
    want_counts = default_counts(name, precision, monkeypatch, capfd)
    counted, counts = wavefront(name, precision, monkeypatch, levels, capfd)
    assert same_bits(counted, want), f"{SWITCH}={levels}: the counting render differs from the megakernel"
    assert counts == want_counts, f"{SWITCH}={levels}: (node_visits, tri_tests, mesh_rays, pops_culled) differ from the default setting's"


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("name", list(SCENES))
def test_lds_levels(dev, monkeypatch, capfd, name, levels, precision):
    assert_unchanged(name, precision, monkeypatch, capfd, levels)


# ---- a mesh whose stack is deeper than the default LDS part ----
STRIP_TRIANGLES = 3000


def strip_obj(path, n=STRIP_TRIANGLES):
    """n thin triangles that all start at the same short edge and reach further and further along x, each a little above the one
    before: every bounding box contains the boxes of the shorter triangles, so no split separates them and the BVH degenerates
    into a long comb whose every node leaves siblings on the stack."""
    lines = ["vt 0 0", "vn 0 1 0"]
    for i in range(n):
        reach = 0.05 + 1.95 * (i + 1) / n
        y = 0.2 * i / n
        lines += [f"v -1 {y!r} -0.4", f"v -1 {y!r} 0.4", f"v {-1 + reach!r} {y + 0.05!r} 0"]
    for i in range(n):
        a = 3 * i + 1
        lines.append(f"f {a}/1/1 {a + 1}/1/1 {a + 2}/1/1")
    path.write_text("\n".join(lines) + "\n")


def strip_scene(tmp_path_factory):
    d = tmp_path_factory.mktemp("strip")
    strip_obj(d / "strip.obj")
    scene = d / "scene"
    scene.write_text("@config output_width = 40\n@config aspect_ratio = 1\n@config focal_length = 40\n"
                     "@config camera_pos = 0,1.5,3\n@config camera_target = 0,0.1,0\n"
                     "strip: mesh strip.obj (glossy (constant 0.7,0.6,0.3) (constant 0.3))\n"
                     "lamp: plane -0.5,2,-0.5 1,0,0 0,0,1 (emissive (constant 8,8,8)) backface\n"
                     "sky: sky (constant 0.3,0.4,0.6)\nworld: list $strip $lamp $sky\nlights: list $lamp\n")
    return api.HostScene([str(scene), "-s=16", "--seed=53"])


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("levels", [None, 0, 4])
def test_deep_mesh_spills_at_the_default(dev, monkeypatch, capfd, tmp_path_factory, levels, precision):
    """mesh_levels = bvh4_stack + 1 of the compiled scene is above the twelve default LDS levels (checked on the CPU first), so
    the default setting has a spill part of its own here (the shallow scenes above have none at 12: their whole stack is in
    LDS).  The bound is the BVH's worst case: how deep the rays of this frame really get is not observed."""
    hs = loaded("strip", lambda: strip_scene(tmp_path_factory))[0]
    stack = api.scene_mesh_stats(hs.desc)["bvh4_stack"]
    assert stack + 1 > DEFAULT_LEVELS + 4, f"the strip's BVH4 needs only {stack + 1} stack levels: nothing spills at the default"
    assert_unchanged("strip", precision, monkeypatch, capfd, levels)


def test_ray_queries_on_the_edge(dev, monkeypatch):
    """rt_trace_rays goes through the same launches: the closest-hit batch of tests/ray_query_cases.py at one LDS level, against
    the oracle at the bar of tests/test_gpu_ray_query.py."""
    c = cases("two_meshes")
    monkeypatch.setenv(SWITCH, "1")
    scene = api.DeviceScene(c.hs.desc, 0)
    got = scene.trace_rays(c.ab_o, c.ab_d)
    assert_hits_equal_oracle(got, c.ab_hits, c.hs.desc, c.extent)
    monkeypatch.delenv(SWITCH)
    assert scene.trace_rays(c.ab_o, c.ab_d).tobytes() == got.tobytes()
    scene.close()
