"""Point queries on the GPU (rt_closest_points) against the brute-force f64 reference of
tests/closest_points_ref.py, point by point.

Point set per scene, rng = default_rng(31), extent = the largest |world coordinate| of the primitives (closest_points_ref.point_sets):
256 points uniform in the primitives' box inflated 1.5x, 256 points on random primitives displaced by rng.normal(3) * 1e-3 * extent,
16 points at 1e4 * extent from the centre, 16 exact mesh vertices in world space (where there is a mesh), every sphere centre.

The f64 bar is tol = 1e-12 * (|q|inf + extent): the parity bar of tests/test_gpu_parity.py applied to the magnitude the roundings
act on.  The f32 bar is that of tests/f32_point_bounds.py.  The reference answers are computed once per scene and shared.

The two max_distance statements (nothing found below 0.5 d_ref, the unlimited answer below 2 d_ref) are made for the points with
d_ref >= 2 tol: for a point ON the surface (the exact mesh vertices: d_ref = 0) no limit of the form c * d_ref separates "strictly
below" from "not below", and such points may go either way."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import closest_points_ref as cr
import f32_point_bounds as pb
from rust_raytracer_amd import api
from ray_query_cases import SCENES, host_scene
from scene_update_cases import displaced_obj

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTRACE = os.path.join(REPO, "rust_raytracer_amd", "rtrace")
F64, F32 = api.RT_PRECISION_F64, api.RT_PRECISION_F32
FOUND, BACK = api.RT_POINT_FOUND, api.RT_POINT_BACK_SIDE
POINT_SCENES = ["cornell", "two_meshes", "light_test", "sphere_field", "hollow_glass", "polished", "sun_sky"]
PATHS = dict(SCENES, polished="tests/scenes/polished")


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


class Case:
    """A scene's reference, its point sets and the reference answer of every point (computed once)."""

    def __init__(self, hs):
        self.hs = hs
        self.ref = cr.Reference(hs.desc)
        self.sets = cr.point_sets(self.ref, np.random.default_rng(31))
        self.points = np.ascontiguousarray(np.concatenate(list(self.sets.values())))
        self.tol = 1e-12 * (np.abs(self.points).max(axis=1) + self.ref.extent)
        answers = [self.ref.query(q, 2 * t) for q, t in zip(self.points, self.tol)]
        self.d_ref = np.array([a[0] for a in answers])
        self.near = [a[1] for a in answers]

    def slice_of(self, name):
        at = 0
        for k, v in self.sets.items():
            if k == name:
                return slice(at, at + len(v))
            at += len(v)
        raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(api.HostScene([PATHS[name], "-w=24", "-s=1", "--seed=31"]))


_scenes = {}


def device_scene(name):
    """One DeviceScene per scene for the whole module (queries leave a scene as it was)."""
    if name not in _scenes:
        _scenes[name] = api.DeviceScene(case(name).hs.desc, 0)
    return _scenes[name]


NOT_FOUND = np.zeros(1, dtype=api.RtPointHit)
NOT_FOUND["distance"] = np.inf
NOT_FOUND["material"] = NOT_FOUND["node"] = NOT_FOUND["prim"] = -1


def assert_matches_reference(c, got, points=None, tol=None, d_ref=None, near=None):
    """Test 1, every point."""
    ref, desc = c.ref, c.hs.desc.contents
    points = c.points if points is None else points
    tol, d_ref, near = (c.tol if tol is None else tol), (c.d_ref if d_ref is None else d_ref), (c.near if near is None else near)
    assert len(got) == len(points)
    worst = 0.0
    for i, (q, g) in enumerate(zip(points, got)):
        t = tol[i]
        assert g["flags"] & FOUND and not g["flags"] & ~np.uint32(FOUND | BACK), (i, g)
        d, pos, nrm, node, prim = float(g["distance"]), g["pos"], g["normal"], int(g["node"]), int(g["prim"])
        worst = max(worst, abs(d - d_ref[i]) / t)
        assert abs(d - d_ref[i]) <= t, (i, q, d, d_ref[i], t)
        assert (node, prim) in near[i], (i, q, node, prim, near[i])
        if prim >= 0:
            assert ref.geom.on_primitive(node, prim, pos, t), (i, q, pos)
        else:
            assert ref.distance_to(pos, node, prim) <= t, (i, q, pos)
        assert abs(np.linalg.norm(q - pos) - d) <= t, (i, q, pos, d)
        want = [n for n in ref.normal(node, prim, pos)]
        if all(np.isfinite(n).all() for n in want):
            assert abs(np.linalg.norm(nrm) - 1.0) <= 1e-9, (i, nrm)
            assert min(np.abs(nrm - n).max() for n in want) <= 1e-9, (i, q, nrm, want)
        else:   # a zero-area triangle
            assert not nrm.any()
        side = float(np.dot(q - pos, nrm))
        if abs(side) > t:
            assert bool(g["flags"] & BACK) == (side < 0), (i, q, side)
        assert g["material"] == desc.nodes[node].material
        assert g["_reserved"] == 0
    return worst


# ---- 1. f64 against the reference ----
@pytest.mark.parametrize("name", POINT_SCENES)
def test_f64_matches_reference(dev, name):
    c = case(name)
    for s, n in (("box", 256), ("near", 256), ("far", 16)):
        assert len(c.sets[s]) == n
    assert ("vertices" in c.sets) == any(e["type"] == api.RT_NODE_MESH for e in c.ref.geom.entries)
    assert np.isfinite(c.d_ref).all()
    got = device_scene(name).closest_points(c.points)
    worst = assert_matches_reference(c, got)
    st = device_scene(name).point_query_stats()
    assert st.rays == len(c.points) and st.precision == F64 and st.n_chunks == 1 and st.kernel_ms > 0
    if "vertices" in c.sets:
        assert len({len(s) for s in c.near[c.slice_of("vertices")]} - {1}) >= 1   # the vertices are many-way ties
    print(f"[closest points f64] {name}: n={len(c.points)} largest |d - d_ref| / tol {worst:.3g}, kernel {st.kernel_ms:.3f} ms")


# ---- f32 at the bound of tests/f32_point_bounds.py ----
@pytest.mark.parametrize("name", POINT_SCENES)
def test_f32_within_bounds(dev, name):
    c = case(name)
    got = device_scene(name).closest_points(c.points, precision=F32)
    pb.check(c.ref, c.points, got, c.d_ref, name)
    assert (got["_reserved"] == 0).all()


# ---- 2. max_distance ----
@pytest.mark.parametrize("prec", [F64, F32])
def test_max_distance(dev, prec):
    c = case("two_meshes")
    scene = device_scene("two_meshes")
    free = scene.closest_points(c.points, precision=prec)
    clear = c.d_ref >= 2 * c.tol if prec == F64 else c.d_ref >= 4 * pb.K_DIST * pb.U * np.maximum(np.abs(c.points).max(axis=1), c.ref.extent)
    assert clear.sum() >= 512 and (~clear).sum() >= 16
    half = scene.closest_points(c.points, 0.5 * c.d_ref, precision=prec)
    assert half[clear].tobytes() == np.repeat(NOT_FOUND, clear.sum()).tobytes()
    twice = scene.closest_points(c.points, 2.0 * c.d_ref, precision=prec)
    assert twice[clear].tobytes() == free[clear].tobytes()
    for k in np.nonzero(~clear)[0]:   # on the surface: found as without a limit, or not found
        assert twice[k].tobytes() in (free[k].tobytes(), NOT_FOUND.tobytes())
    mixed_limit = np.where(np.arange(len(c.points)) % 3 == 0, 0.5 * c.d_ref, np.where(np.arange(len(c.points)) % 3 == 1, 2.0 * c.d_ref, np.inf))
    mixed = scene.closest_points(c.points, mixed_limit, precision=prec)
    k = np.arange(len(c.points)) % 3
    assert mixed[clear & (k == 0)].tobytes() == half[clear & (k == 0)].tobytes()
    assert mixed[clear & (k == 1)].tobytes() == free[clear & (k == 1)].tobytes()
    assert mixed[k == 2].tobytes() == free[k == 2].tobytes()
    assert scene.closest_points(c.points[:5], 1e-30, precision=prec).tobytes() == np.repeat(NOT_FOUND, 5).tobytes()   # a scalar broadcasts


# ---- 3. independence, bit for bit ----
def test_chunks_give_the_same_bytes(dev, monkeypatch):
    c = case("light_test")
    scene = device_scene("light_test")
    pts = c.points[:377]
    for prec in (F64, F32):
        one = scene.closest_points(pts, precision=prec)
        monkeypatch.setenv("RT_RQ_CHUNK", "64")
        many = scene.closest_points(pts, precision=prec)
        assert scene.point_query_stats().n_chunks == 6
        monkeypatch.delenv("RT_RQ_CHUNK")
        assert many.tobytes() == one.tobytes()
        lim = np.linspace(0.0, 2.0, 377) * c.d_ref[:377]
        one = scene.closest_points(pts, lim, precision=prec)
        monkeypatch.setenv("RT_RQ_CHUNK", "64")
        many = scene.closest_points(pts, lim, precision=prec)
        monkeypatch.delenv("RT_RQ_CHUNK")
        assert many.tobytes() == one.tobytes()


def test_device_pointer_variant(dev):
    import torch
    c = case("two_meshes")
    scene = device_scene("two_meshes")
    n = len(c.points)
    lim = np.where(np.arange(n) % 2 == 0, np.inf, 1.5 * c.d_ref)
    d_p, d_lim = torch.from_numpy(c.points).cuda(), torch.from_numpy(lim).cuda()
    d_out = torch.full((n * api.RtPointHit.itemsize,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for prec in (F64, F32):
        scene.closest_points_device(n, d_p.data_ptr(), d_out.data_ptr(), precision=prec)
        assert d_out.cpu().numpy().tobytes() == scene.closest_points(c.points, precision=prec).tobytes()
        scene.closest_points_device(n, d_p.data_ptr(), d_out.data_ptr(), d_lim.data_ptr(), precision=prec)
        assert d_out.cpu().numpy().tobytes() == scene.closest_points(c.points, lim, precision=prec).tobytes()


def test_tree_built_on_the_device_gives_the_same_distances(dev):
    c = case("light_test")
    host_tree = device_scene("light_test").closest_points(c.points)
    desc = c.hs.desc.contents
    desc.flags |= api.RT_SCENE_BVH_ON_DEVICE
    try:
        scene = api.DeviceScene(c.hs.desc, 0)
    finally:
        desc.flags &= ~api.RT_SCENE_BVH_ON_DEVICE
    device_tree = scene.closest_points(c.points)
    scene.close()
    assert device_tree["distance"].tobytes() == host_tree["distance"].tobytes()   # conservative culling: the tree cannot change the minimum
    same = (device_tree["node"] == host_tree["node"]) & (device_tree["prim"] == host_tree["prim"])
    assert same.mean() >= 0.9
    assert device_tree["pos"][same].tobytes() == host_tree["pos"][same].tobytes()


# ---- 4. after rt_scene_update ----
def test_after_scene_update(dev, tmp_path):
    displaced_obj(os.path.join(REPO, "scenes", "resource", "monkey.obj"), tmp_path / "moved.obj")
    text = open(os.path.join(REPO, "scenes", "light_test")).read()
    assert "resource/monkey.obj" in text
    (tmp_path / "light_test_moved").write_text(text.replace("resource/monkey.obj", "moved.obj"))
    args = ["-w=24", "-s=1", "--seed=31"]
    moved = Case(api.HostScene([str(tmp_path / "light_test_moved")] + args))
    # the new geometry at the points of the old scene near its surface, and at the new one's own
    pts = np.ascontiguousarray(np.concatenate([case("light_test").sets["near"][:128], moved.sets["near"][:128], moved.sets["vertices"], moved.sets["far"]]))
    tol = 1e-12 * (np.abs(pts).max(axis=1) + moved.ref.extent)
    answers = [moved.ref.query(q, 2 * t) for q, t in zip(pts, tol)]
    scene = api.DeviceScene(case("light_test").hs.desc, 0)
    before = scene.closest_points(pts)   # the workspace and its tables exist before the update
    info = scene.update(moved.hs.desc)
    assert info["n_meshes_refit"] == 1
    after = scene.closest_points(pts)
    assert after.tobytes() != before.tobytes()
    assert_matches_reference(moved, after, pts, tol, np.array([a[0] for a in answers]), [a[1] for a in answers])
    fresh = api.DeviceScene(moved.hs.desc, 0)
    assert fresh.closest_points(pts).tobytes() == after.tobytes()
    assert fresh.closest_points(pts, precision=F32).tobytes() == scene.closest_points(pts, precision=F32).tobytes()
    fresh.close()
    scene.close()


# ---- 5. refusals ----
@pytest.mark.parametrize("name, word", [("nested_transform", "similarity"), ("smoke", "volumes")])
def test_refusals_allocate_nothing(dev, name, word):
    hs = host_scene(name)
    scene = api.DeviceScene(hs.desc, 0)
    pts = np.zeros((4, 3))
    live = api.live_resources()
    for call in (lambda: scene.closest_points(pts), lambda: scene.closest_points(pts, 1.0, F32), lambda: scene.closest_points_counts(pts)):
        with pytest.raises(api.RtError) as e:
            call()
        assert e.value.status == api.RT_E_UNSUPPORTED and word in str(e.value)
        assert api.live_resources() == live
    scene.close()


def test_argument_errors_and_empty_scene(dev):
    scene = device_scene("two_meshes")
    lib, h = scene._lib, scene._h
    p, out = np.zeros((2, 3)), np.zeros(2, dtype=api.RtPointHit)
    assert lib.rt_closest_points(h, 2, None, None, F64, out.ctypes.data) == api.RT_E_INVALID
    assert lib.rt_closest_points(h, 2, p.ctypes.data, None, F64, None) == api.RT_E_INVALID
    assert lib.rt_closest_points(h, 2, p.ctypes.data, None, 7, out.ctypes.data) == api.RT_E_INVALID
    assert b"precision" in lib.rt_last_error()
    assert lib.rt_closest_points(h, 0, None, None, F64, None) == api.RT_OK   # n = 0: a no-op
    # non-finite inputs are not an error
    weird = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 1], [1e308, 1e308, 1e308]])
    for prec in (F64, F32):
        assert len(scene.closest_points(weird, precision=prec)) == 4
        assert len(scene.closest_points(p, np.array([np.nan, -1.0]), precision=prec)) == 2
    sky_host = api.HostScene(["tests/scenes/sky_only", "-w=8"])
    sky = api.DeviceScene(sky_host.desc, 0)
    pts = np.random.default_rng(31).normal(size=(70, 3))
    for prec in (F64, F32):
        assert sky.closest_points(pts, precision=prec).tobytes() == np.repeat(NOT_FOUND, 70).tobytes()
    sky.close()


# ---- 6. resources ----
def test_resources_return_to_the_baseline(dev):
    c = case("two_meshes")
    base = api.live_resources()
    scene = api.DeviceScene(c.hs.desc, 0)
    scene.closest_points(c.points[:100])
    scene.closest_points(c.points[:300], precision=F32)
    scene.closest_points_counts(c.points[:50])
    scene.closest_points(c.points[:100], 1.0)
    assert api.live_resources() != base
    scene.close()
    assert api.live_resources() == base


# ---- 7. the traversal culls ----
def test_traversal_culls(dev):
    c = case("light_test")
    ref, scene = c.ref, device_scene("light_test")
    near = c.sets["near"]
    mesh_rows = np.nonzero(ref.tri_ids[:, 2] >= 0)[0]
    n_triangles = len(mesh_rows)
    assert n_triangles == 15744
    d_mesh = np.array([cr.closest_on_triangles(ref.tri[mesh_rows], q)[0].min() for q in near])
    pts = np.ascontiguousarray(near[d_mesh <= 1e-3 * ref.extent])
    assert len(pts) >= 16
    for prec in (F64, F32):
        counts = scene.closest_points_counts(pts, precision=prec)
        assert counts.shape == (len(pts), 2) and counts.dtype == np.uint32
        print(f"[closest points counts] light_test, {len(pts)} points within 1e-3 extent of the mesh, precision {prec}: "
              f"mean nodes {counts[:, 0].mean():.1f}, mean triangle tests {counts[:, 1].mean():.1f}")
        assert (counts[:, 0] >= 1).all() and (counts[:, 1] >= 1).all()
        assert counts[:, 1].mean() <= n_triangles / 16


# ---- 8. rtrace --nearest ----
def test_rtrace_nearest_prints_what_closest_points_returns(dev, tmp_path):
    pts = np.array([[278.0, 273.0, -100.0], [10.5, 20.25, 30.125], [555.0, 548.8, 0.0], [-1000.0, 2000.0, 1e5]])
    arg = "--nearest=" + ":".join(",".join(repr(float(x)) for x in p) for p in pts)
    r = subprocess.run([RTRACE, os.path.join(REPO, "scenes/cornell"), "-w=16", arg], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert not (tmp_path / "out.png").exists()
    hs = api.HostScene(["scenes/cornell", "-w=16", arg])
    assert hs.nearest.tolist() == pts.tolist()
    scene = api.DeviceScene(hs.desc, 0)
    want = scene.closest_points(pts, precision=hs.params.precision)
    scene.close()
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Nearest ")]
    assert len(lines) == len(pts)
    for i, (ln, w) in enumerate(zip(lines, want)):
        nums = ["%.17g" % x for x in [w["distance"], *w["pos"], *w["normal"]]]
        assert ln == (f"Nearest {i}: distance {nums[0]} position {nums[1]} {nums[2]} {nums[3]} normal {nums[4]} {nums[5]} {nums[6]} "
                      f"node {w['node']} triangle {w['prim']} material {w['material']} flags {w['flags']}"), (ln, w)
        m = re.search(r"distance (\S+) ", ln)
        assert float(m.group(1)) == w["distance"]   # %.17g round-trips: every bit
