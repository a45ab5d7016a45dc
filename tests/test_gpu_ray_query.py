"""Ray queries on the GPU (rt_trace_rays, rt_occluded) against the CPU oracle, ray by ray.

The ray sets and the yardstick are those of tests/ray_query_cases.py: camera rays (a), incoherent follow-up rays (b) and
segments between hit points (c), answered by pyoracle.world_hit.  f64 answers must agree exactly in class (miss / surface /
environment), material and front face and at the bar of tests/test_gpu_parity.py (1e-12 relative, floor 1e-15) in t, position,
normal, u and v; f32 answers at that file's statistical bar (95 % of the rays, t within 5 %)."""
import numpy as np
import pytest

from rust_raytracer_amd import api
from ray_query_cases import (ENVIRONMENT, SURFACE, T_MAX, T_MIN, Cases, assert_hits_equal_oracle, cases, host_scene, klass_of)
from scene_update_cases import MONKEY, displaced_obj, same_bits, two_meshes_variant

pytestmark = pytest.mark.gpu

F64, F32 = api.RT_PRECISION_F64, api.RT_PRECISION_F32
ORACLE_SCENES = ["cornell", "two_meshes", "nested_transform", "sun_sky", "sphere_field", "hollow_glass", "light_test", "texture_mix"]


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


_scenes = {}


def device_scene(name):
    """One DeviceScene per scene for the whole module (queries leave a scene as it was)."""
    if name not in _scenes:
        _scenes[name] = api.DeviceScene(cases(name).hs.desc, 0)
    return _scenes[name]


# ---- 1. f64 closest hit against the oracle ----
@pytest.mark.parametrize("name", ORACLE_SCENES)
def test_closest_hit_matches_oracle(dev, name):
    c = cases(name)
    c.assert_not_vacuous()
    got = device_scene(name).trace_rays(c.ab_o, c.ab_d)
    assert_hits_equal_oracle(got, c.ab_hits, c.hs.desc, c.extent)
    assert (c.fu_hits["klass"] == SURFACE).any() and (~c.fu_hits["front"][c.fu_hits["klass"] == SURFACE]).any(), "no back-face hit among the follow-ups"
    st = device_scene(name).ray_query_stats()
    assert st.rays == len(got) and st.n_chunks == 1 and st.precision == F64 and st.kernel_ms > 0.0
    if name == "two_meshes":   # the two instances of the one mesh are told apart
        d = c.hs.desc.contents
        mesh_nodes = {int(n) for n in got["node"][klass_of(got) == SURFACE] if d.nodes[n].type == api.RT_NODE_MESH}
        assert len(mesh_nodes) == 2
        assert (got["prim"][np.isin(got["node"], list(mesh_nodes))] >= 0).all()
    if name == "texture_mix":  # normal-mapped materials are hit, and the normal reported is the unmapped one (it matched the oracle's)
        d = c.hs.desc.contents
        mapped = {k for k in range(d.n_materials) if d.materials[k].type in (api.RT_MAT_GLOSSY, api.RT_MAT_NORMAL_DEBUG) and d.materials[k].tex_c >= 0}
        assert mapped and np.isin(got["material"], list(mapped)).any()
    if name == "sun_sky":
        assert (c.ab_hits["klass"] == ENVIRONMENT).any()


# ---- 2. same bytes under the other kernel plans ----
@pytest.mark.parametrize("switch", ["RT_WF_SPLIT=0", "RT_WF_GROUPS=0", "RT_WF_NODES=0", "RT_WF_MESH_MULTI=1"])
@pytest.mark.parametrize("name", ["two_meshes", "sphere_field"])
def test_same_bytes_under_other_plans(dev, monkeypatch, name, switch):
    c = cases(name)
    base = device_scene(name).trace_rays(c.ab_o, c.ab_d)
    key, value = switch.split("=")
    monkeypatch.setenv(key, value)
    other = device_scene(name).trace_rays(c.ab_o, c.ab_d)
    assert other.tobytes() == base.tobytes()


# ---- 3. f64 occlusion against the oracle ----
@pytest.mark.parametrize("name", ORACLE_SCENES)
def test_occlusion_matches_oracle(dev, name):
    c = cases(name)
    c.assert_not_vacuous()
    scene = device_scene(name)
    got = scene.occluded(c.seg_o, c.seg_d, T_MIN, T_MAX)
    assert got.dtype == bool
    np.testing.assert_array_equal(got, c.seg_occluded)
    # existence agrees with the closest hit on these segments (no closest t lies within 1e-6 of t_max)
    closest = scene.trace_rays(c.seg_o, c.seg_d)
    np.testing.assert_array_equal(got, closest["t"] < T_MAX)
    # just short of / just past the oracle's closest surface hit of the follow-up rays
    surf = c.fu_hits["klass"] == SURFACE
    o, d, t = c.fu_o[surf], c.fu_d[surf], c.fu_hits["t"][surf]
    assert not scene.occluded(o, d, None, 0.999 * t).any()
    assert scene.occluded(o, d, None, 1.001 * t).all()


# ---- 4. shapes, chunks, device pointers, broadcasting ----
def test_shapes_and_chunks(dev, monkeypatch):
    c = cases("two_meshes")
    scene = device_scene("two_meshes")
    o, d = np.concatenate([c.ab_o, c.ab_o[::-1]]), np.concatenate([c.ab_d, c.ab_d[::-1]])
    assert len(o) >= 1000
    whole = scene.trace_rays(o, d)
    seg_whole = scene.occluded(c.seg_o, c.seg_d, T_MIN, T_MAX)
    for n in (0, 1, 63, 65, 577):
        part = scene.trace_rays(o[:n], d[:n])
        assert part.shape == (n,) and part.tobytes() == whole[:n].tobytes()
        m = min(n, len(c.seg_o))
        np.testing.assert_array_equal(scene.occluded(c.seg_o[:m], c.seg_d[:m], T_MIN, T_MAX), seg_whole[:m])
    monkeypatch.setenv("RT_RQ_CHUNK", "256")
    chunked = scene.trace_rays(o, d)
    assert scene.ray_query_stats().n_chunks == (len(o) + 255) // 256
    assert chunked.tobytes() == whole.tobytes()
    np.testing.assert_array_equal(scene.occluded(c.seg_o, c.seg_d, T_MIN, T_MAX), seg_whole)
    assert scene.ray_query_stats().n_chunks == (len(c.seg_o) + 255) // 256


def test_device_pointer_variants(dev):
    import torch
    c = cases("two_meshes")
    scene = device_scene("two_meshes")
    n = len(c.seg_o)
    d_o, d_d = torch.from_numpy(c.seg_o).cuda(), torch.from_numpy(c.seg_d).cuda()
    d_lo = torch.full((n,), T_MIN, dtype=torch.float64, device="cuda")
    d_hi = torch.full((n,), T_MAX, dtype=torch.float64, device="cuda")
    d_hits = torch.zeros(n * api.RtRayHit.itemsize, dtype=torch.uint8, device="cuda")
    d_occ = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    scene.trace_rays_device(n, d_o.data_ptr(), d_d.data_ptr(), d_hits.data_ptr())
    scene.occluded_device(n, d_o.data_ptr(), d_d.data_ptr(), d_occ.data_ptr(), d_lo.data_ptr(), d_hi.data_ptr())
    assert d_hits.cpu().numpy().tobytes() == scene.trace_rays(c.seg_o, c.seg_d).tobytes()
    np.testing.assert_array_equal(d_occ.cpu().numpy().astype(bool), scene.occluded(c.seg_o, c.seg_d, T_MIN, T_MAX))
    scene.occluded_device(n, d_o.data_ptr(), d_d.data_ptr(), d_occ.data_ptr())   # default interval
    np.testing.assert_array_equal(d_occ.cpu().numpy().astype(bool), scene.occluded(c.seg_o, c.seg_d))


def test_scalars_broadcast(dev):
    c = cases("two_meshes")
    scene = device_scene("two_meshes")
    n = len(c.seg_o)
    np.testing.assert_array_equal(scene.occluded(c.seg_o, c.seg_d, T_MIN, T_MAX),
                                  scene.occluded(c.seg_o, c.seg_d, np.full(n, T_MIN), np.full(n, T_MAX)))
    origin = c.cam_o[0]
    assert (c.cam_o == origin).all(), "no lens in this scene: every camera ray starts at the camera"
    assert scene.trace_rays(origin, c.cam_d).tobytes() == scene.trace_rays(c.cam_o, c.cam_d).tobytes()
    one = scene.trace_rays(origin, c.cam_d[5])
    assert one.shape == (1,) and one.tobytes() == scene.trace_rays(c.cam_o, c.cam_d)[5:6].tobytes()


# ---- 5. f32 ----
@pytest.mark.parametrize("name", ["cornell", "two_meshes", "sphere_field", "light_test"])
def test_f32_statistical(dev, name):
    c = cases(name)
    scene = device_scene(name)
    got, want = scene.trace_rays(c.ab_o, c.ab_d, precision=F32), c.ab_hits
    assert scene.ray_query_stats().precision == F32
    same = (klass_of(got) == want["klass"]) & (got["material"] == want["material"])
    surf = want["klass"] == SURFACE
    t_err = np.where(surf & same, np.abs(got["t"] - want["t"]) / np.abs(want["t"]), 0.0)
    agree = same & (t_err <= 0.05)
    seg = scene.occluded(c.seg_o, c.seg_d, T_MIN, T_MAX, precision=F32) == c.seg_occluded
    print(f"{name} f32: {agree.mean():.4%} of {len(got)} rays agree (class, material, t within 5 %), largest t error "
          f"{t_err.max():.3e}; {seg.mean():.4%} of {len(seg)} segments agree")
    assert agree.mean() >= 0.95
    assert seg.mean() >= 0.95


# ---- 6. refusals ----
def test_refusals(dev):
    hs = host_scene("smoke")
    assert api.scene_info(hs.desc) & api.RT_SCENE_INFO_VOLUMES
    scene = api.DeviceScene(hs.desc, 0)
    o, d = np.zeros((2, 3)), np.ones((2, 3))
    for call in (lambda: scene.trace_rays(o, d), lambda: scene.occluded(o, d)):
        with pytest.raises(api.RtError) as e:
            call()
        assert e.value.status == api.RT_E_UNSUPPORTED and "volumes" in str(e.value)
    scene.close()
    scene = device_scene("two_meshes")
    lib, h = scene._lib, scene._h
    hits = np.zeros(2, dtype=api.RtRayHit)
    occ = np.zeros(2, dtype=np.uint8)
    assert lib.rt_trace_rays(h, 2, None, d.ctypes.data, F64, hits.ctypes.data) == api.RT_E_INVALID
    assert lib.rt_trace_rays(h, 2, o.ctypes.data, d.ctypes.data, F64, None) == api.RT_E_INVALID
    assert lib.rt_occluded(h, 2, o.ctypes.data, None, None, None, F64, occ.ctypes.data) == api.RT_E_INVALID
    assert lib.rt_occluded(h, 2, o.ctypes.data, d.ctypes.data, None, None, F64, None) == api.RT_E_INVALID
    assert lib.rt_trace_rays(h, 2, o.ctypes.data, d.ctypes.data, 7, hits.ctypes.data) == api.RT_E_INVALID
    assert b"precision" in lib.rt_last_error()
    assert lib.rt_trace_rays(h, 0, None, None, F64, None) == api.RT_OK   # n = 0: a no-op


# ---- 7. after rt_scene_update ----
def test_queries_after_update(dev, tmp_path):
    args = ("-w=24", "-s=1", "--seed=31")
    a = api.HostScene(["tests/scenes/two_meshes"] + list(args))
    displaced_obj(MONKEY, tmp_path / "moved.obj")
    b = two_meshes_variant(tmp_path, "moved", numeric=True, m1=tmp_path / "moved.obj", args=args)
    cb = Cases(b)
    cb.assert_not_vacuous()
    scene = api.DeviceScene(a.desc, 0)
    before = scene.trace_rays(cb.ab_o, cb.ab_d)   # the workspace and its tables exist before the update
    info = scene.update(b.desc)
    assert info["n_meshes_refit"] == 1
    after = scene.trace_rays(cb.ab_o, cb.ab_d)
    assert after.tobytes() != before.tobytes()
    assert_hits_equal_oracle(after, cb.ab_hits, b.desc, cb.extent)
    np.testing.assert_array_equal(scene.occluded(cb.seg_o, cb.seg_d, T_MIN, T_MAX), cb.seg_occluded)
    scene.close()


# ---- 8. renders unaffected ----
@pytest.mark.parametrize("prec", [F64, F32])
def test_render_unaffected_by_queries(dev, prec):
    c = cases("two_meshes")
    hs = api.HostScene(["tests/scenes/two_meshes", "-w=48", "-s=4", "--seed=31"])
    p = hs.params.copy()
    p.precision = prec
    scene = api.DeviceScene(hs.desc, 0)
    first = scene.render(hs.camera, p)
    stats = scene.stats().as_dict()
    scene.trace_rays(c.ab_o, c.ab_d, precision=prec)
    scene.occluded(c.seg_o, c.seg_d, T_MIN, T_MAX, precision=prec)
    assert scene.stats().as_dict() == stats, "queries leave rt_get_stats alone"
    second = scene.render(hs.camera, p)
    scene.close()
    assert same_bits(first, second)
