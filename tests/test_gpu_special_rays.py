"""Ray searches on the GPU held to the unculled oracle on rays in special position (tests/special_ray_cases.py has the scenes,
the families and the yardstick; tests/test_special_rays_host.py shows that the yardstick is exact and the sets not vacuous).

Zero and -0.0 direction components, rays at vertices and along shared edges, origins on box planes, tangents and rims: the
inputs that clamped_inv, the NaN conventions of the 4-wide node step, make_cull_ray's t_shift guard, quantise_dir's range
test, span_misses' slack and node2_step's near/far tie (csrc/rt_traverse.h) were written for.  A hit that the reference's
primitive test accepts inside the reference's list / transform / object-BVH boxes must be reported; the project's own trees
never drop one.

f64: class, material, front face, t and position of every ray equal the oracle's, with `==` on mesh hits of the dyadic rays;
normal, u, v where no two triangles tie, and a tie-aware rule where they do - under every kernel plan, with the cone and
slab culls on and off, with the tree built on the host and on the device, through the wavefront kernels and the megakernel's
search, for closest hits and for occlusion.  f32: the per-ray rule of tests/f32_ray_bounds.py, unchanged."""
import numpy as np
import pytest

from rust_raytracer_amd import api
from ray_query_cases import ENVIRONMENT, MISS, SURFACE, T_MIN, close
import f32_ray_bounds as fb
import special_ray_cases as sc

pytestmark = pytest.mark.gpu

F64, F32 = api.RT_PRECISION_F64, api.RT_PRECISION_F32
ALL = sc.MESH_SCENES + ("S",)
# every plan of the search kernels (rt_wavefront.h): BVH2 instead of 4-wide nodes, the multi-mesh kernel, no sphere / quad
# split, no primitive groups, the cone cull off, the slab cull off / on every child / on leaf children
SWITCHES = ("RT_WF_NODES=0", "RT_WF_MESH_MULTI=1", "RT_WF_SPLIT=0", "RT_WF_GROUPS=0", "RT_WF_CONES=0", "RT_WF_SLABS=0",
            "RT_WF_SLABS=1", "RT_WF_SLABS=2")


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


_scenes = {}


def device_scene(name):
    """One DeviceScene per scene for the whole module (queries leave a scene as it was)."""
    if name not in _scenes:
        _scenes[name] = api.DeviceScene(sc.case(name).desc, 0)
    return _scenes[name]


def check_subset(got, c, rays, sel):
    o, d, want, near, _, dyadic = rays
    sc.assert_equal_unculled(got[sel], c, o[sel], d[sel], want[sel], near[sel], dyadic[sel])


# ---- 1. f64 closest hit ----
@pytest.mark.parametrize("name", ALL)
def test_closest_hit_equals_unculled_oracle(dev, name):
    c = sc.case(name)
    rays = c.all_rays()
    got = device_scene(name).trace_rays(rays[0], rays[1])
    check_subset(got, c, rays, np.arange(len(got)))


# ---- 2. the same answers under every plan ----
@pytest.mark.parametrize("name", ALL)
def test_same_answers_under_every_plan(dev, monkeypatch, name):
    c = sc.case(name)
    rays = c.all_rays()
    o, d, want, near = rays[:4]
    scene = device_scene(name)
    base = scene.trace_rays(o, d)
    so, sd, hi, occ = c.segments()
    for switch in SWITCHES:
        key, value = switch.split("=")
        monkeypatch.setenv(key, value)
        other = scene.trace_rays(o, d)
        seg = scene.occluded(so, sd, T_MIN, hi)
        monkeypatch.delenv(key)
        differ = np.flatnonzero((other.view(np.uint8).reshape(len(other), -1) != base.view(np.uint8).reshape(len(base), -1)).any(axis=1))
        assert (near[differ] > 1).all(), f"{switch}: {int((near[differ] <= 1).sum())} rays without a tie change their bytes"
        check_subset(other, c, rays, differ)          # which of the tied triangles wins may change, nothing else
        np.testing.assert_array_equal(seg, occ, err_msg=switch)


# ---- 3. the tree built on the device ----
@pytest.mark.parametrize("name", ["G", "C", "D", "G_twice", "C_moved", "D_twice"])
def test_device_built_tree(dev, name):
    """A different tree (LBVH over Morton codes; D's three copies have identical centroids), so no same bytes: the tie-aware
    comparison against the oracle, and occlusion."""
    c = sc.case(name)
    desc = c.desc.contents
    desc.flags |= api.RT_SCENE_BVH_ON_DEVICE
    try:
        scene = api.DeviceScene(c.desc, 0)
    finally:
        desc.flags &= ~api.RT_SCENE_BVH_ON_DEVICE
    rays = c.all_rays()
    got = scene.trace_rays(rays[0], rays[1])
    so, sd, hi, occ = c.segments()
    seg = scene.occluded(so, sd, T_MIN, hi)
    scene.close()
    check_subset(got, c, rays, np.arange(len(got)))
    np.testing.assert_array_equal(seg, occ)


# ---- 4. the megakernel's search ----
@pytest.mark.parametrize("name", sc.MESH_SCENES)
def test_megakernel_search(dev, name):
    """world_test and resolve_hit of the megakernel (mesh_traverse over the BVH2) on the mesh families, through
    rt_debug_shade_rays: the entry that takes caller-supplied rays (rt_debug_trace_sample draws its rays from a camera with
    pixel jitter and cannot send one in special position)."""
    c = sc.case(name)
    o, d, want, near, _, dyadic = c.all_rays()
    p = c.hs.params.copy()
    p.precision = F64
    out, _ = device_scene(name).shade_rays(p, o, d, np.arange(len(o), dtype=np.uint64))
    hit = want["klass"] != MISS
    surf = want["klass"] == SURFACE
    np.testing.assert_array_equal(out[:, 10].astype(np.int32), want["material"])
    np.testing.assert_array_equal(out[hit, 9] != 0, want["front"][hit])
    assert (out[surf & dyadic, 0] == want["t"][surf & dyadic]).all() and (out[surf & dyadic, 1:4] == want["pos"][surf & dyadic]).all()
    assert close(out[hit, 0], want["t"][hit]).all() and close(out[hit, 1:4], want["pos"][hit]).all()
    one = hit & (near <= 1)
    assert close(out[one, 4:7], want["normal"][one]).all()
    # a tie: the normal is a face normal of the mesh with the sign the front-face rule gives it (every face is axis-aligned)
    tied = out[surf & (near > 1), 4:7]
    assert ((np.abs(tied) == 1).sum(axis=1) == 1).all() and ((tied == 0).sum(axis=1) == 2).all()


# ---- 5. occlusion ----
@pytest.mark.parametrize("name", ALL)
def test_occlusion_equals_unculled_oracle(dev, name):
    c = sc.case(name)
    scene = device_scene(name)
    so, sd, hi, occ = c.segments()
    assert occ.mean() >= 0.3 and (~occ).mean() >= 0.3
    got = scene.occluded(so, sd, T_MIN, hi)
    np.testing.assert_array_equal(got, occ)
    # the rays that lie in a face, run along a border or pass one ulp outside a box / the rays on the guard planes, over an
    # interval that keeps the environment out
    r = c.families["d" if c.is_mesh else "f"]
    want = sc.unculled_hits(c.desc, r.o, r.d, T_MIN, sc.T_FINITE)["klass"] != MISS
    np.testing.assert_array_equal(scene.occluded(r.o, r.d, T_MIN, sc.T_FINITE), want)
    assert (~want).any()


# ---- 6. f32 ----
@pytest.mark.parametrize("name", ALL)
def test_f32_rule_with_the_unculled_yardstick(dev, name):
    c = sc.case(name)
    geom, o, d, want, so, sd, hi, occ = sc.f32_set(name)
    scene = device_scene(name)
    got = scene.trace_rays(o, d, precision=F32)
    assert scene.ray_query_stats().precision == F32
    seg = scene.occluded(so, sd, T_MIN, hi, precision=F32)
    closest = fb.check_closest(geom, o, d, got, want, c.extent(), name + " closest", oracle=lambda oo, dd: sc.unculled_hits(c.desc, oo, dd))
    segments = fb.check_occlusion(geom, so, sd, seg, occ, name + " segments", T_MIN, hi, hi, oracle=sc.unculled_hits)
    print(closest.line())
    print(segments.line())
    closest.check(show=False)
    segments.check(show=False)
    # no leak through a crack: a ray through an interior vertex or edge of the mesh is a surface hit of the right material in
    # f32 - none of its copies sees the sky, so `fit` above has already failed it otherwise; here it is said outright
    if c.is_mesh:
        interior = (want["klass"] == SURFACE) & ~np.isin(np.arange(len(o)), closest.excused)
        assert (got["material"][interior] == want["material"][interior]).all()
