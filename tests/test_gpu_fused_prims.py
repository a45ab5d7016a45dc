"""k_wf_prims as phase 4 of k_wf_shade (rt_wavefront.h): the fused pipeline `k_wf_mesh -> k_wf_shade(+search)`
must render the frame of the unfused one (RT_WF_FUSE=0: `k_wf_prims -> k_wf_mesh -> k_wf_shade`) bit for bit, with fewer launches
of the stand-alone search kernel.

The frames are 45 x 37 at 9 samples per pixel = 14985 samples: no multiple of a 256-lane trip or a 2048-entry chunk, so the last
chunk of a queue is partial; the pools (5000 / 4096 slots) are far smaller than the sample count, so every slot restarts several
times (chunks in slot order) before the tail thins the queue out (chunks walked through the list).  Everything here needs the GPU."""
import numpy as np
import pytest

from rust_raytracer_amd import api

pytestmark = pytest.mark.gpu

SIZE = ["-w=45", "-r=1.2162", "-s=9"]  # 45 / 1.2162 = 37.0005 -> 37 rows


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def render_pair(scene_args, monkeypatch, env, threads=None, precision=None, fused_mode=None):
    """The frame and the statistics of the default (fused where the plan allows it; fused_mode="2": wherever the fused kernel
    exists) and of the RT_WF_FUSE=0 render."""
    hs = api.HostScene(scene_args + SIZE + ([f"-t={threads}"] if threads else []))
    assert (hs.width, hs.height) == (45, 37)
    scene = api.DeviceScene(hs.desc, 0)
    p = hs.params.copy()
    p.pipeline = api.RT_PIPELINE_WAVEFRONT
    if precision is not None:
        p.precision = precision
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = {}
    for fuse in ("1", "0"):
        if fuse == "0":
            monkeypatch.setenv("RT_WF_FUSE", "0")
        elif fused_mode is not None:
            monkeypatch.setenv("RT_WF_FUSE", fused_mode)
        else:
            monkeypatch.delenv("RT_WF_FUSE", raising=False)
        frame = scene.render(hs.camera, p)
        st = scene.stats()
        out[fuse] = (frame, {k: getattr(st, k) for k in ("n_launches", "n_iterations", "prims_kernel_ms", "shade_kernel_ms",
                                                          "n_tail_compactions", "n_replica_groups", "pipeline_used")})
    monkeypatch.delenv("RT_WF_FUSE", raising=False)
    return hs, scene, p, out


def assert_fused_and_identical(out):
    (fused, sf), (plain, sp) = out["1"], out["0"]
    assert sf["pipeline_used"] == sp["pipeline_used"] == api.RT_PIPELINE_WAVEFRONT
    assert same_bits(fused, plain), f"{int((fused.view(np.uint64) != plain.view(np.uint64)).any(axis=2).sum())} pixels differ from RT_WF_FUSE=0"
    assert sf["n_iterations"] == sp["n_iterations"]
    assert sp["n_launches"] == sp["n_iterations"]            # unfused: one search launch per iteration
    assert sf["n_launches"] < sp["n_launches"], (sf, sp)     # fused: after k_wf_generate and after each compaction only
    assert sf["prims_kernel_ms"] < sp["prims_kernel_ms"], (sf, sp)
    return sf, sp


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_no_mesh_partial_last_chunk(dev, monkeypatch, precision):
    """scenes/cornell (no mesh op: the iteration is the fused kernel alone); 5000 slots = two whole chunks and one of 904."""
    prec = api.RT_PRECISION_F64 if precision == "f64" else api.RT_PRECISION_F32
    _, _, _, out = render_pair(["scenes/cornell", "--seed=41"], monkeypatch, {"RT_WF_POOL": "5000", "RT_WF_COMPACT": "0"}, precision=prec)
    sf, _ = assert_fused_and_identical(out)
    assert sf["n_launches"] == 1 and sf["n_tail_compactions"] == 0


def test_one_mesh_against_the_megakernel(dev, monkeypatch):
    """scenes/light_test: deferred mesh op, the mesh queue is built by phase 4.  Also the megakernel's frame, bit for bit."""
    hs, scene, p, out = render_pair(["scenes/light_test", "--seed=42"], monkeypatch, {"RT_WF_POOL": "4096", "RT_WF_COMPACT": "0"})
    assert_fused_and_identical(out)
    p.pipeline = api.RT_PIPELINE_MEGAKERNEL
    mega = scene.render(hs.camera, p)
    assert same_bits(out["1"][0], mega)


def test_two_meshes(dev, monkeypatch):
    """tests/scenes/two_meshes: the general (MULTI) form of k_wf_mesh fed by the fused queue.  The plan leaves programs with
    several mesh ops unfused (they were slower fused), so the fused side is forced with RT_WF_FUSE=2; by default nothing changes."""
    env = {"RT_WF_POOL": "4096", "RT_WF_COMPACT": "0"}
    _, _, _, out = render_pair(["tests/scenes/two_meshes", "--seed=43"], monkeypatch, env, fused_mode="2")
    assert_fused_and_identical(out)
    _, _, _, dflt = render_pair(["tests/scenes/two_meshes", "--seed=43"], monkeypatch, env)
    assert same_bits(dflt["1"][0], out["0"][0]) and dflt["1"][1]["n_launches"] == dflt["1"][1]["n_iterations"]


def test_multi_mesh_kernel_on_a_fused_plan(dev, monkeypatch):
    """scenes/light_test with the general form of k_wf_mesh (RT_WF_MESH_MULTI=1): fused by default."""
    _, _, _, out = render_pair(["scenes/light_test", "--seed=48"], monkeypatch, {"RT_WF_POOL": "4096", "RT_WF_COMPACT": "0", "RT_WF_MESH_MULTI": "1"})
    assert_fused_and_identical(out)


def test_compaction_is_followed_by_the_stand_alone_search(dev, monkeypatch):
    """A tail compaction moves the paths to new slots without their hit records: the stand-alone kernel recomputes them and
    rebuilds the mesh queue (the one phase 4 had built names the old slots)."""
    _, _, _, out = render_pair(["scenes/light_test", "--seed=44"], monkeypatch,
                               {"RT_WF_POOL": "4096", "RT_WF_COMPACT": "1", "RT_WF_COMPACT_MIN": "64"})
    sf, sp = assert_fused_and_identical(out)
    assert sf["n_tail_compactions"] > 0 and sp["n_tail_compactions"] > 0
    assert sf["n_tail_compactions"] == sp["n_tail_compactions"]
    assert sf["n_launches"] == 1 + sf["n_tail_compactions"]


def test_bvh_spheres_frame_unchanged(dev, monkeypatch):
    """tests/scenes/bvh_spheres (an object BVH in the scene file): the frame is unchanged and the stand-alone kernel still runs."""
    _, _, _, out = render_pair(["tests/scenes/bvh_spheres", "--seed=45"], monkeypatch, {"RT_WF_POOL": "4096"})
    (fused, sf), (plain, sp) = out["1"], out["0"]
    assert same_bits(fused, plain)
    assert sf["prims_kernel_ms"] > 0 and sp["prims_kernel_ms"] > 0


@pytest.mark.parametrize("scene", ["tests/scenes/sphere_field", "scenes/cornell_smoke", "tests/scenes/smoke"])
def test_plans_the_fused_form_does_not_cover_stay_unfused(dev, monkeypatch, scene):
    """Re-built primitive groups (k_wf_prims<GROUPS>), volumes inside k_wf_prims<VOL> and the combined intersect kernel: one
    search launch per iteration with and without RT_WF_FUSE, the same frame."""
    _, _, _, out = render_pair([scene, "--seed=47"], monkeypatch, {"RT_WF_POOL": "4096"})
    (fused, sf), (plain, sp) = out["1"], out["0"]
    assert same_bits(fused, plain)
    assert sf["n_launches"] == sf["n_iterations"] == sp["n_launches"] == sp["n_iterations"]
    if scene != "tests/scenes/smoke":  # the combined kernel's time is reported as traversal time
        assert sf["prims_kernel_ms"] > 0 and sp["prims_kernel_ms"] > 0


def test_second_replica_group_starts_with_the_stand_alone_search(dev, monkeypatch):
    """-t=2 with one replica per group: the second group's first iteration follows k_wf_generate, not a fused k_wf_shade."""
    _, _, _, out = render_pair(["scenes/light_test", "--seed=46"], monkeypatch,
                               {"RT_WF_POOL": "3000", "RT_WF_SAMPLE_GB": "0", "RT_WF_COMPACT": "0"}, threads=2)
    sf, sp = assert_fused_and_identical(out)
    assert sf["n_replica_groups"] == sp["n_replica_groups"] == 2
    assert sf["n_launches"] == 2
