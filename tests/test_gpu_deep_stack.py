"""The per-lane LDS traversal stacks at their limits (DESIGN.md sections 14, 15 and 20): k_rq_occluded, k_bake_visibility and
k_pq_closest on the chains of tests/deep_stack_cases.py, whose trees need 32, 33, 64 and 65 stack levels, against brute force.

  levels  occlusion / bake (4 B x 256 lanes)   point query (8 B)
  32      32 KB                                256 lanes, 64 KB
  33      33 KB                                the first 128-lane launch, 33 KB
  64      64 KB                                128 lanes, 64 KB
  65      refused                              refused

The segments hold levels - 2 entries (every box is entered) and, one per stack index, depend on the entry at that index
alone: a keyed segment's only occluder sits in the leaf popped from index k, its near miss passes that triangle by 2e-6 of
its size.  A dropped entry is a lost occluder.  The yardsticks are the oracle's primitive tests without its octree, the
brute-force point reference and bake_ref's recipe; the restated walks of deep_stack_cases only chose the inputs
(tests/test_deep_stack_host.py checks them).  f32 runs at 32 and 33 levels only: the coordinates of the deeper chains span
1e+-30 and their squares leave the f32 range.  Everything here needs the GPU."""
import ctypes as C

import numpy as np
import pytest

import closest_points_ref as cr
import deep_stack_cases as dc
import f32_point_bounds as pb
import f32_ray_bounds as fb
from oracle import pyoracle
from ray_query_cases import SURFACE, assert_hits_equal_oracle, close
from rust_raytracer_amd import api
from special_ray_cases import unculled_hits
from test_gpu_closest_points import assert_matches_reference

pytestmark = pytest.mark.gpu

F64, F32 = api.RT_PRECISION_F64, api.RT_PRECISION_F32
F32_MARGIN = 2.0 ** -10
SWITCH = "RT_WF_LDS_LEVELS"


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


_scenes = {}


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for scene in _scenes.values():
        scene.close()
    _scenes.clear()


def device_scene(name):
    """One DeviceScene per case for the whole module (queries and bakes leave a scene as it was)."""
    if name not in _scenes:
        _scenes[name] = api.DeviceScene(dc.host_scene(name).desc, 0)
    return _scenes[name]


# ---- 1. occlusion ----
@pytest.mark.parametrize("name", ["L32", "L33", "L64", "L33_back"])
def test_occluded_f64_equals_brute_force(dev, name):
    sg = dc.segments(name)
    got = device_scene(name).occluded(sg.o, sg.d, sg.t_lo, sg.t_hi)
    wrong = np.flatnonzero(got != sg.occluded)
    print(f"{name}: {len(sg)} segments, {int(sg.occluded.sum())} occluded; wrong: {[(str(sg.kind[i]), int(sg.key[i])) for i in wrong]}")
    np.testing.assert_array_equal(got, sg.occluded)
    assert sg.occluded.any() and (~sg.occluded).any()


@pytest.mark.parametrize("name", dc.F32_CASES)
def test_occluded_f32_within_the_ray_bounds(dev, name):
    sg = dc.segments(name, F32_MARGIN)
    assert (sg.t_lo == 0.0).all()
    scene = device_scene(name)
    got = scene.occluded(sg.o, sg.d, sg.t_lo, sg.t_hi, precision=F32)
    assert scene.ray_query_stats().precision == F32
    rep = fb.check_occlusion(fb.Geometry(dc.host_scene(name).desc), sg.o, sg.d, got, sg.occluded, name + " deep-stack segments", 0.0, sg.t_hi,
                             sg.t_hi, oracle=unculled_hits)
    print(rep.line())
    print(f"{name} f32: excused share {rep.share:.2%} (cap {fb.CAP:.0%}), differing from the reference "
          f"{[(str(sg.kind[i]), int(sg.key[i])) for i in np.flatnonzero(got != sg.occluded)]}")
    rep.check(show=False)


# ---- 2. the bake ----
def baked(scene, g, samples, precision=F64):
    return scene.bake_visibility(g.pos, g.nrm, samples=samples, seed=dc.BAKE_SEED, bias=g.bias, max_distance=g.max_distance, precision=precision)


@pytest.mark.parametrize("name", ["L32", "L64"])
def test_bake_f64_matches_the_reference(dev, name):
    scene = device_scene(name)
    for g in dc.bake_groups(name):
        for samples, count, vis, bent in g.shapes:
            got = baked(scene, g, samples)
            got_count = np.rint(got["visibility"] * samples).astype(np.int64)
            print(f"{name} s = {g.s:.3g}, {len(g.pos)} x {samples}: counts {got_count.tolist()} reference {count.tolist()}, "
                  f"largest bent difference {np.abs(got['bent'] - bent).max():.3e}")
            np.testing.assert_array_equal(got_count, count)
            assert (got["visibility"] == count / float(samples)).all()
            assert np.abs(got["bent"] - bent).max() <= 1e-12
            assert scene.bake_stats().rays == len(g.pos) * samples and scene.bake_stats().precision == F64


# The rule of tests/test_gpu_bake.py's test_f32_against_the_f64_reference: the yardstick is the reference's f64 counts, the bound
# twice the mean of |count32 - count_ref| / S measured on the MI355X, which is 0 of 1 312 samples on L32: the f32 counts must
# equal the reference's.
F32_BAKE_MEASURED = 0.0


def test_bake_f32_against_the_f64_reference(dev):
    scene = device_scene("L32")
    diff, rays = 0.0, 0
    for g in dc.bake_groups("L32"):
        for samples, count, vis, bent in g.shapes:
            got = baked(scene, g, samples, F32)
            assert scene.bake_stats().precision == F32
            assert ((got["visibility"] >= 0.0) & (got["visibility"] <= 1.0)).all()
            c32 = np.rint(got["visibility"] * samples).astype(np.int64)
            assert (got["visibility"] == c32 / float(samples)).all()
            assert (np.linalg.norm(got["bent"], axis=1) <= 1.0 + 1e-5).all()
            diff += float(np.abs(c32 - count).sum())
            rays += len(g.pos) * samples
    share = diff / rays
    print(f"L32 f32: mean |count32 - count_ref| / S = {share:.6f} ({int(diff)} of {rays} samples)")
    assert share <= 2.0 * F32_BAKE_MEASURED


# ---- 3. point queries ----
class PointCase:
    """What test_gpu_closest_points.assert_matches_reference wants of a case.  tol = 1e-12 * (|q|inf + the largest coordinate of
    the nearest triangle): the parity bar applied to the numbers the roundings act on.  The extent of the whole chain, which
    the other point tests use, is up to 1e39 times the size of the triangle asked about."""

    def __init__(self, name):
        self.hs = dc.host_scene(name)
        self.ref = cr.Reference(self.hs.desc)
        self.points = dc.points(name).q
        dist = [self.ref.distances(q)[0] for q in self.points]
        size = np.array([np.abs(self.ref.tri[int(np.argmin(d))]).max() for d in dist])
        self.tol = 1e-12 * (np.abs(self.points).max(axis=1) + size)
        answers = [self.ref.query(q, 2 * t) for q, t in zip(self.points, self.tol)]
        self.d_ref = np.array([a[0] for a in answers])
        self.near = [a[1] for a in answers]


_point_cases = {}


def point_case(name):
    if name not in _point_cases:
        _point_cases[name] = PointCase(name)
    return _point_cases[name]


@pytest.mark.parametrize("name", ["L32", "L33", "L64"])
def test_closest_points_f64_equal_brute_force(dev, name):
    c = point_case(name)
    scene = device_scene(name)
    got = scene.closest_points(c.points)
    worst = assert_matches_reference(c, got)
    st = scene.point_query_stats()
    assert st.rays == len(c.points) == dc.N_POINTS and st.precision == F64 and st.n_chunks == 1
    print(f"{name}: {len(c.points)} points, largest |d - d_ref| / tol {worst:.3g}")
    # the counting form of the kernel runs with the same stack: it must not disturb the records, and it visits what it says
    counts = scene.closest_points_counts(c.points)
    assert counts.shape == (len(c.points), 2) and (counts[:, 0] >= 1).all() and (counts[:, 1] >= 1).all()
    assert (counts == scene.closest_points_counts(c.points)).all()
    assert scene.closest_points(c.points).tobytes() == got.tobytes()
    print(f"{name}: mean nodes visited {counts[:, 0].mean():.1f}, mean triangles tested {counts[:, 1].mean():.1f}")


@pytest.mark.parametrize("name", dc.F32_CASES)
def test_closest_points_f32_within_the_point_bounds(dev, name):
    c = point_case(name)
    got = device_scene(name).closest_points(c.points, precision=F32)
    pb.check(c.ref, c.points, got, c.d_ref, name + " deep-stack points")
    assert (got["_reserved"] == 0).all()


# ---- 4. 65 levels: the three kernels refuse, k_wf_mesh spills ----
def test_refusals_at_65_levels_leave_the_outputs_alone(dev):
    sg, scene = dc.segments("L65"), device_scene("L65")
    n = 40
    o, d = np.ascontiguousarray(sg.o[:n]), np.ascontiguousarray(sg.d[:n])
    normals = np.ascontiguousarray(np.broadcast_to([0.0, 1.0, 0.0], (n, 3)))
    for call, word in ((lambda: scene.occluded(o, d, 0.0, sg.t_hi[:n]), "mesh BVH too deep for the occlusion kernel's LDS traversal stack"),
                       (lambda: scene.occluded(o, d, 0.0, sg.t_hi[:n], precision=F32), "mesh BVH too deep for the occlusion kernel's LDS traversal stack"),
                       (lambda: scene.bake_visibility(o, normals, samples=8), "mesh BVH too deep for the bake kernel's LDS traversal stack"),
                       (lambda: scene.closest_points(o), "mesh BVH too deep for the point-query kernel's LDS traversal stack"),
                       (lambda: scene.closest_points_counts(o), "mesh BVH too deep for the point-query kernel's LDS traversal stack")):
        with pytest.raises(api.RtError) as e:
            call()
        assert e.value.status == api.RT_E_UNSUPPORTED and word in str(e.value), str(e.value)
    lib, h = scene._lib, scene._h
    occ = np.full(n, 0xA5, dtype=np.uint8)
    assert lib.rt_occluded(h, n, o.ctypes.data, d.ctypes.data, None, None, F64, occ.ctypes.data) == api.RT_E_UNSUPPORTED
    assert (occ == 0xA5).all()
    vis = np.full(n * api.RtBakeResult.itemsize, 0xA5, dtype=np.uint8)
    bp = api.RtBakeParams.defaults(samples=8)
    assert lib.rt_bake_visibility(h, n, o.ctypes.data, normals.ctypes.data, C.byref(bp), vis.ctypes.data) == api.RT_E_UNSUPPORTED
    assert (vis == 0xA5).all()
    pts = np.full(n * api.RtPointHit.itemsize, 0xA5, dtype=np.uint8)
    assert lib.rt_closest_points(h, n, o.ctypes.data, None, F64, pts.ctypes.data) == api.RT_E_UNSUPPORTED
    assert (pts == 0xA5).all()


@pytest.mark.parametrize("lds_levels", [None, 0])
def test_trace_rays_at_65_levels_equal_the_oracle(dev, monkeypatch, lds_levels):
    """rt_trace_rays goes through k_wf_mesh, whose stack spills beyond its LDS part: the through lines and the keyed lines as
    rays over (0.001, inf), at the default LDS part and with every entry spilled.  A keyed line of a small triangle is a miss
    here as in the oracle (its crossing lies below t = 0.001); those of the larger triangles hit the triangle they are keyed to."""
    sg = dc.segments("L65")
    sel = (sg.kind == "through") | (sg.kind == "keyed")
    o, d = np.ascontiguousarray(sg.o[sel]), np.ascontiguousarray(sg.d[sel])
    want = unculled_hits(dc.host_scene("L65").desc, o, d)
    surf = want["klass"] == SURFACE
    assert surf.sum() >= 16 and (~surf).sum() >= 16
    if lds_levels is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, str(lds_levels))
    got = device_scene("L65").trace_rays(o, d)
    assert_hits_equal_oracle(got, want)
    np.testing.assert_array_equal(got["prim"][surf], sg.target[sel][surf])


@pytest.mark.parametrize("name", ["L65", "L65_lit"])
def test_frame_at_65_levels(dev, name):
    """24 x 24, megakernel and wavefront: bit-identical, and at the parity bar (1e-12 relative, non-finite values of the same
    kind) against the oracle's frame.  L65 has the empty light list of the query scenes: the reference's light sampling makes a
    NaN of every path that meets the chain, so that frame only says WHICH pixels meet it.  L65_lit has the sky for a light
    and finite values everywhere: there the scattered rays, which start on the chain and run along it, are held too."""
    hs = dc.host_scene(name)
    scene = device_scene(name)
    frames = {}
    for pipeline in (api.RT_PIPELINE_MEGAKERNEL, api.RT_PIPELINE_WAVEFRONT):
        p = hs.params.copy()
        p.pipeline, p.precision = pipeline, F64
        frames[pipeline] = scene.render(hs.camera, p)
        assert scene.stats().pipeline_used == pipeline
    mega, wave = frames[api.RT_PIPELINE_MEGAKERNEL], frames[api.RT_PIPELINE_WAVEFRONT]
    assert mega.shape == (24, 24, 4) and mega.tobytes() == wave.tobytes()
    want = pyoracle.render(hs.desc, hs.camera, hs.params)[0]
    ok = close(mega[..., :3], want[..., :3])
    nan = np.isnan(want[..., :3]).any(axis=2)
    print(f"{name}: {int(nan.sum())} of 576 pixels are NaN in the oracle's frame, {int((~ok).sum())} values beyond the bar")
    assert ok.all(), f"{int((~ok).sum())} values beyond 1e-12 relative"
    if name == "L65":
        assert 64 <= nan.sum() <= 512
    else:
        assert not nan.any() and len(np.unique(want[..., :3].reshape(-1, 3), axis=0)) >= 64, "the chain is not in the frame"


# ---- 5. after rt_scene_update ----
def test_after_update_at_64_levels(dev):
    """Every vertex of L64 times 1 + 2^-10: the refit keeps the tree and with it the 64 levels; occlusion and point queries give
    the bytes of a fresh scene of the scaled chain (and occlusion, by similarity, the flags of the unscaled one)."""
    k = 1.0 + 2.0 ** -10
    moved = dc.new_host_scene("L64", positions_scale=k)
    assert api.scene_mesh_stats(moved.desc)["bvh4_stack"] + 1 == 64
    sg, pts = dc.segments("L64"), dc.points("L64").q * k
    o, d = sg.o * k, sg.d * k
    scene = api.DeviceScene(dc.host_scene("L64").desc, 0)
    before = scene.closest_points(pts)   # the workspaces exist before the update
    assert scene.update(moved.desc)["n_meshes_refit"] == 1
    fresh = api.DeviceScene(moved.desc, 0)
    occ = scene.occluded(o, d, sg.t_lo, sg.t_hi)
    np.testing.assert_array_equal(occ, fresh.occluded(o, d, sg.t_lo, sg.t_hi))
    np.testing.assert_array_equal(occ, sg.occluded)
    after = scene.closest_points(pts)
    assert after.tobytes() == fresh.closest_points(pts).tobytes()
    assert after.tobytes() != before.tobytes()
    fresh.close()
    scene.close()
