"""The search setup that renders and ray queries share (rt_kernels.hip make_search_setup), on the three paths that only a
switch selects: a staged PREFIX of the small tables, a k_wf_mesh stack that spills to global memory after two levels, and the
counting kernels of re-built primitive groups.  Each must give the frames and the RtRayHit records of the default switches
bit for bit: these are equalities between runs of the library; the anchors to the oracle and the megakernel are
tests/test_gpu_parity.py, test_gpu_wavefront.py and test_gpu_ray_query.py.

Frames: 45 x 37 at 9 samples per pixel with a 4096-slot pool, as in tests/test_gpu_fused_prims.py (partial last chunk, every
slot restarts).  Rays: the camera rays of tests/ray_query_cases.py.  Everything here needs the GPU."""
import numpy as np
import pytest

from rust_raytracer_amd import api
from ray_query_cases import SCENES, camera_rays, host_scene

pytestmark = pytest.mark.gpu

SIZE = ["-w=45", "-r=1.2162", "-s=9", "--seed=52"]
F64, F32 = api.RT_PRECISION_F64, api.RT_PRECISION_F32
SWITCHES = ("RT_LDS_BUDGET", "RT_LDS_SHADE_PREFIX", "RT_LDS_TABLES", "RT_WF_LDS_LEVELS")


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


class Bench:
    """One device scene of `name`, rendered and queried under sets of switches."""

    def __init__(self, name, monkeypatch):
        self.hs = api.HostScene([SCENES[name]] + SIZE)
        assert (self.hs.width, self.hs.height) == (45, 37)
        self.scene = api.DeviceScene(self.hs.desc, 0)
        self.rays = camera_rays(host_scene(name))
        self.mp = monkeypatch
        monkeypatch.setenv("RT_WF_POOL", "4096")

    def switch(self, env):
        for k in SWITCHES:
            self.mp.delenv(k, raising=False)
        for k, v in env.items():
            self.mp.setenv(k, v)

    def render(self, env, precision=F64, collect_stats=0):
        self.switch(env)
        p = self.hs.params.copy()
        p.pipeline = api.RT_PIPELINE_WAVEFRONT
        p.precision = precision
        p.collect_stats = collect_stats
        frame = self.scene.render(self.hs.camera, p)
        st = self.scene.stats()
        assert st.pipeline_used == api.RT_PIPELINE_WAVEFRONT
        return frame, st

    def trace(self, env, precision=F64):
        self.switch(env)
        return self.scene.trace_rays(*self.rays, precision=precision)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_as_default(b, env):
    """f64 and f32 frames and hit records under `env` against the default switches, on one scene object (default first: the
    workspaces exist already and have to grow where `env` asks for more)."""
    for prec in (F64, F32):
        base, _ = b.render({}, prec)
        hits = b.trace({}, prec)
        assert (hits["flags"] & api.RT_RAY_HIT).any()
        got, st = b.render(env, prec)
        assert same_bits(got, base), f"precision {prec}: {int((got.view(np.uint64) != base.view(np.uint64)).any(axis=2).sum())} pixels differ"
        assert same_bits(b.trace(env, prec), hits), f"precision {prec}: hit records differ"
    return st


# RT_LDS_BUDGET per scene: see the docstring of test_prefix_staging
PREFIX_BUDGET = {"texture_mix": "1024", "light_test": "512"}


@pytest.mark.parametrize("name", ["texture_mix", "light_test"])
def test_prefix_staging(dev, monkeypatch, name):
    """RT_LDS_BUDGET small enough that only the first tables of the staging order fit: k_wf_prims<.., 2, ..> (lds_prims == 2) and, with
    RT_LDS_SHADE_PREFIX=1 where the scene has no texture interpreter, k_wf_shade<.., 2, ..>.  Staged / total bytes of the tables:

        scene         budget   prims f64    prims f32    shade f64    shade f32
        texture_mix   1024     976 / 3152   896 / 2176   (interpreter variant: tables from global memory)
        light_test    512      384 / 1536   464 / 1072   400 / 1536   496 / 1072

    k_wf_prims' dynamic LDS is the 8208 B of its lists plus the staged bytes, measured on the MI355X (f64 / f32): light_test
    8592 / 8672 B against 8208 B at RT_LDS_TABLES=0 and 9744 / 9280 B by default; texture_mix 9184 / 9104 B against 8208 B and
    11360 / 10384 B (profiles/search_setup/README.md)."""
    b = Bench(name, monkeypatch)
    st = assert_same_as_default(b, {"RT_LDS_BUDGET": PREFIX_BUDGET[name], "RT_LDS_SHADE_PREFIX": "1"})
    if name == "light_test":  # fused by default; a prefix of the prims tables keeps the stand-alone k_wf_prims in every iteration
        assert st.n_launches == st.n_iterations
        _, st0 = b.render({}, F32)
        assert st0.n_launches < st0.n_iterations


@pytest.mark.parametrize("name", ["light_test", "two_meshes"])
def test_stack_spill(dev, monkeypatch, name):
    """RT_WF_LDS_LEVELS=2: k_wf_mesh (single-mesh and MULTI form) keeps two stack levels in LDS and the rest in the spill buffer,
    whose size the shared setup gives to two workspaces: the render's (RtScene::Wavefront) and the queries' (RtScene::Query).  Both
    were allocated for the default twelve levels by the runs before and have to grow."""
    b = Bench(name, monkeypatch)
    assert api.scene_mesh_stats(b.hs.desc)["bvh4_stack"] + 1 > 2  # mesh_levels of the setup: something is left to spill
    assert_same_as_default(b, {"RT_WF_LDS_LEVELS": "2"})


@pytest.mark.parametrize("tables", ["0", "1"])
def test_groups_with_counters(dev, monkeypatch, tables):
    """tests/scenes/sphere_field (re-built primitive groups): the counting k_wf_prims<GROUPS> with the tables in global memory
    and staged renders the lean frame and counts primitive tests."""
    b = Bench("sphere_field", monkeypatch)
    lean, _ = b.render({})
    got, st = b.render({"RT_LDS_TABLES": tables}, collect_stats=1)
    assert same_bits(got, lean)
    assert st.prim_tests > 0
    assert st.prims_kernel_ms > 0  # the split plan (k_wf_prims), not the combined kernel
