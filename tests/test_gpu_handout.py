"""How the waves of the persistent search kernels share their queue (csrc/rt_handout.h): a static first
range per wave, ranges that shrink towards the end of the queue, and in k_wf_mesh the range's entries staged in LDS.  Which
wave traverses a ray must not matter: every render here is compared bit for bit with RT_WF_HANDOUT=0 (256 entries per atomic
from the first on, through the same code object) and with the megakernel, in both precisions.

RT_WF_MESH_GRID = 1, 2, 3 workgroups are 4, 8, 12 waves; with pools of 63 .. 4096 slots the queues then fit the static ranges
(no atomic), overrun them by less than one range, or run through full, shrinking and final partial ranges to exhaustion.
The policy itself is checked without a GPU in tests/test_handout_host.py.  Everything here needs the GPU."""
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
SWITCHES = ("RT_WF_HANDOUT", "RT_WF_MESH_GRID", "RT_WF_POOL", "RT_WF_SPLIT")


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


_loaded = {}


def loaded(name):
    """Host scene, device scene and the megakernel's frames (computed once per precision) of a scene."""
    if name not in _loaded:
        hs = api.HostScene(SCENES[name])
        assert (hs.width, hs.height) == ((45, 37) if name == "light_test" else (40, 40))
        _loaded[name] = (hs, api.DeviceScene(hs.desc, 0), {})
    return _loaded[name]


def params(hs, precision, pipeline, stats=False):
    p = hs.params.copy()
    p.pipeline = pipeline
    p.precision = PRECISIONS[precision]
    p.collect_stats = int(stats)
    return p


def megakernel_frame(name, precision):
    hs, scene, mega = loaded(name)
    if precision not in mega:
        mega[precision] = scene.render(hs.camera, params(hs, precision, api.RT_PIPELINE_MEGAKERNEL))
    return mega[precision]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def render(name, precision, monkeypatch, env, handout, stats=False):
    hs, scene, _ = loaded(name)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    if handout is not None:
        monkeypatch.setenv("RT_WF_HANDOUT", str(handout))
    frame = scene.render(hs.camera, params(hs, precision, api.RT_PIPELINE_WAVEFRONT, stats))
    st = scene.stats()
    assert st.pipeline_used == api.RT_PIPELINE_WAVEFRONT
    return frame, st


def assert_frames_unchanged(name, precision, monkeypatch, env):
    """The default (= 2: with staging in f64; f32 stages nothing) and RT_WF_HANDOUT=1 against RT_WF_HANDOUT=0 and the megakernel."""
    control, _ = render(name, precision, monkeypatch, env, 0)
    assert same_bits(control, megakernel_frame(name, precision)), "RT_WF_HANDOUT=0 differs from the megakernel"
    for handout in (None, 1):
        frame, _ = render(name, precision, monkeypatch, env, handout)
        differ = int((frame != control).any(axis=2).sum())
        assert same_bits(frame, control), f"RT_WF_HANDOUT={handout}: {differ} pixels differ from RT_WF_HANDOUT=0"


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("name", list(SCENES))
def test_small_grids(dev, monkeypatch, name, grid, precision):
    """The driver's own pool (every sample at once: 14 985 / 25 600 entries) on 4, 8 and 12 waves: static ranges of 256, then
    many full ranges, the shrinking ones, the partial last one."""
    assert_frames_unchanged(name, precision, monkeypatch, {"RT_WF_MESH_GRID": grid})


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("pool", [63, 64, 65, 257, 1000, 4096])
@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("name", list(SCENES))
def test_small_pools(dev, monkeypatch, name, grid, pool, precision):
    """Queues of at most `pool` entries on 4 and 12 waves: fewer entries than waves x 64 (waves without a range), exactly the
    static ranges, one entry more, and queues that need the cursor."""
    assert_frames_unchanged(name, precision, monkeypatch, {"RT_WF_MESH_GRID": grid, "RT_WF_POOL": pool})


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_far_more_waves_than_entries(dev, monkeypatch, precision):
    """The default grid (thousands of waves) on queues of at most 1000 entries: 16 waves have a range, the others none."""
    assert_frames_unchanged("light_test", precision, monkeypatch, {"RT_WF_POOL": 1000})


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_combined_intersect_kernel(dev, monkeypatch, precision):
    """RT_WF_SPLIT=0: k_wf_intersect has the static range and the shrinking ranges too (no staging)."""
    assert_frames_unchanged("two_meshes", precision, monkeypatch, {"RT_WF_SPLIT": 0, "RT_WF_MESH_GRID": 2, "RT_WF_POOL": 4096})


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("name", list(SCENES))
def test_no_entry_is_handed_out_twice(dev, monkeypatch, name, precision):
    """An entry handed out twice leaves the frame as it is (the second traversal finds the same hit) but is counted twice."""
    env = {"RT_WF_MESH_GRID": 3, "RT_WF_POOL": 4096}
    want_frame, want = render(name, precision, monkeypatch, env, 0, stats=True)
    assert want.mesh_rays > 0 and want.node_visits > 0 and want.tri_tests > 0
    for handout in (None, 1):
        frame, st = render(name, precision, monkeypatch, env, handout, stats=True)
        assert same_bits(frame, want_frame)
        assert (st.mesh_rays, st.node_visits, st.tri_tests) == (want.mesh_rays, want.node_visits, want.tri_tests), f"RT_WF_HANDOUT={handout}"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_ray_queries(dev, monkeypatch, n):
    """trace_rays shares the search setup and the launches: n rays of tests/ray_query_cases.py against the oracle, at the bar of
    tests/test_gpu_ray_query.py, and the same bytes as RT_WF_HANDOUT=0."""
    c = cases("two_meshes")
    o, d = np.concatenate([c.ab_o, c.ab_o[::-1]])[:n], np.concatenate([c.ab_d, c.ab_d[::-1]])[:n]
    want = np.concatenate([c.ab_hits, c.ab_hits[::-1]])[:n]
    assert len(o) == n
    if "queries" not in _loaded:
        _loaded["queries"] = api.DeviceScene(c.hs.desc, 0)
    scene = _loaded["queries"]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    got = scene.trace_rays(o, d)
    assert_hits_equal_oracle(got, want, c.hs.desc, c.extent)
    monkeypatch.setenv("RT_WF_HANDOUT", "0")
    assert scene.trace_rays(o, d).tobytes() == got.tobytes()
