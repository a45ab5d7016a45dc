"""The point queries without a GPU: the C ABI is declared and exported, api.RtPointHit has the header's
layout, argument errors need no device, `rtrace --nearest` is checked while the command line is read, the brute-force reference
the GPU tests hold the kernel to (tests/closest_points_ref.py) gives hand-derived answers, and a numpy-float32 restatement of the
kernel's triangle and sphere routines stays inside the f32 bound of tests/f32_point_bounds.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import closest_points_ref as cr
import f32_point_bounds as pb
from rust_raytracer_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rt_mi355.h")
RTRACE = os.path.join(REPO, "rust_raytracer_amd", "rtrace")
ENTRY_POINTS = ("rt_closest_points", "rt_closest_points_device", "rt_point_query_stats", "rt_debug_closest_points_counts")
NEAREST_MESSAGE = "Nearest must be a list of points"


def test_header_declares_and_library_exports_the_entry_points():
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert "RT_MI355_ABI_VERSION 2 " in text   # additions only: the version stands
    lib = C.CDLL(api.DEVICE_LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert hasattr(C.CDLL(api.HOST_LIB_PATH), "rth_nearest_points")
    assert re.search(r"\brth_nearest_points\s*\(", open(os.path.join(REPO, "include", "rt_host.h")).read())
    for method in ("closest_points", "closest_points_device", "point_query_stats", "closest_points_counts"):
        assert callable(getattr(api.DeviceScene, method))
    assert (api.RT_POINT_FOUND, api.RT_POINT_BACK_SIDE) == (1, 2)


def test_layout_matches_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler to check the header with")
    fields = ("distance", "pos", "normal", "material", "node", "prim", "flags", "_reserved")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_mi355.h"\n'
                   'int main(void) { printf("%zu %u %u", sizeof(RtPointHit), RT_POINT_FOUND, RT_POINT_BACK_SIDE);\n'
                   + "".join(f'printf(" %zu", offsetof(RtPointHit, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    h = api.RtPointHit
    assert out[0] == 80 == h.itemsize
    assert out[1:3] == [api.RT_POINT_FOUND, api.RT_POINT_BACK_SIDE]
    assert out[3:] == [h.fields[f][1] for f in fields] == [0, 8, 32, 56, 60, 64, 68, 72]


def test_argument_errors_need_no_device():
    lib = api.load_device_lib()
    buf = (C.c_double * 16)()
    assert lib.rt_closest_points(None, 1, buf, None, api.RT_PRECISION_F64, buf) == api.RT_E_INVALID
    assert b"NULL scene" in lib.rt_last_error()
    assert lib.rt_closest_points_device(None, 1, buf, None, api.RT_PRECISION_F64, buf, None) == api.RT_E_INVALID
    assert lib.rt_debug_closest_points_counts(None, 1, buf, None, api.RT_PRECISION_F64, buf) == api.RT_E_INVALID
    assert lib.rt_point_query_stats(None, None) == api.RT_E_INVALID


# ---- rtrace --nearest ----
def test_nearest_flag():
    assert api.HostScene(["scenes/cornell", "-w=8"]).nearest.shape == (0, 3)
    hs = api.HostScene(["scenes/cornell", "-w=8", "--nearest=278,273,-100"])
    assert hs.nearest.tolist() == [[278.0, 273.0, -100.0]]
    hs = api.HostScene(["scenes/cornell", "-w=8", "--nearest=1,2,3:-0.5,1e2,7:0,0,0", "--precision=f32"])
    assert hs.nearest.tolist() == [[1.0, 2.0, 3.0], [-0.5, 100.0, 7.0], [0.0, 0.0, 0.0]]


# the malformed forms of test_ray_query_host.test_pick_flag_malformed, with three components
@pytest.mark.parametrize("value", ["3", "3,4", "3,4,", ",4,5", "3,4,5:", ":3,4,5", "3,4,5,6", "a,b,c", "3;4;5", "3,4,5:6", "3,4,5:6,7",
                                   "1,2,inf", "nan,2,3", "1,-inf,3"])
def test_nearest_flag_malformed(value):
    with pytest.raises(api.RtError) as e:
        api.HostScene(["scenes/cornell", "-w=8", f"--nearest={value}"])
    assert e.value.status == api.RT_E_INVALID and NEAREST_MESSAGE in str(e.value)


@pytest.mark.parametrize("other", ["--gpus=2", "--progressive=1", "--noise-threshold=0.1", "--pick=0,0", "--ao=4", "--probe=1,2,3",
                                   "--irradiance", "--pipeline=mega", "--sh-probe=1,2,3"])
def test_nearest_flag_refused_combinations(other):
    with pytest.raises(api.RtError, match="--nearest queries points|--sh-probe bakes probes"):
        api.HostScene(["scenes/cornell", "-w=8", "--nearest=1,2,3", other])


def test_rtrace_rejects_nearest_with_a_sequence_before_touching_a_device(tmp_path):
    r = subprocess.run([RTRACE, os.path.join(REPO, "scenes/cornell"), "-w=16", "-s=4", "--nearest=278,273,-100", "--sequence=scenes/cornell"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "--nearest" in r.stderr and "--sequence" in r.stderr
    assert "Nearest 0" not in r.stdout and "no HIP device" not in r.stderr


# ---- known answers of the reference ----
UNIT = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])   # the unit right triangle in z = 0
S2 = np.sqrt(2.0)
# one query point in each of the seven Voronoi regions: (q, closest point, distance), derived by hand
VORONOI = [
    ((0.25, 0.25, 2.0), (0.25, 0.25, 0.0), 2.0),                 # face: straight down
    ((-1.0, -2.0, 0.0), (0.0, 0.0, 0.0), np.sqrt(5.0)),          # vertex (0, 0)
    ((2.0, -1.0, 0.0), (1.0, 0.0, 0.0), S2),                     # vertex (1, 0)
    ((-1.0, 3.0, 0.0), (0.0, 1.0, 0.0), np.sqrt(5.0)),           # vertex (0, 1)
    ((0.5, -1.0, 1.0), (0.5, 0.0, 0.0), S2),                     # edge y = 0
    ((-2.0, 0.25, 0.0), (0.0, 0.25, 0.0), 2.0),                  # edge x = 0
    ((1.5, 1.5, 0.0), (0.5, 0.5, 0.0), S2),                      # hypotenuse: foot of (1.5, 1.5) on x + y = 1
]


@pytest.mark.parametrize("q, c, d", VORONOI)
def test_reference_unit_triangle_voronoi_regions(q, c, d):
    dist, pt = cr.closest_on_triangles(UNIT, np.array(q))
    assert abs(dist[0] - d) <= 4e-16 * max(1.0, d)
    np.testing.assert_allclose(pt[0], c, rtol=0, atol=4e-16)


def test_reference_zero_area_triangle():
    # three collinear corners (0,0,0), (2,0,0), (1,0,0): the segment [0, 2] on the x axis
    tri = np.array([[[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 0.0, 0.0]]])
    for q, c, d in (((1.5, 3.0, 4.0), (1.5, 0.0, 0.0), 5.0), ((5.0, 0.0, 4.0), (2.0, 0.0, 0.0), 5.0), ((-3.0, 4.0, 0.0), (0.0, 0.0, 0.0), 5.0)):
        dist, pt = cr.closest_on_triangles(tri, np.array(q))
        assert np.isfinite(dist[0]) and abs(dist[0] - d) <= 1e-15
        np.testing.assert_allclose(pt[0], c, rtol=0, atol=1e-15)
    # all three corners the same point
    dist, pt = cr.closest_on_triangles(np.full((1, 3, 3), 1.0), np.array([1.0, 1.0, 4.0]))
    assert dist[0] == 3.0 and pt[0].tolist() == [1.0, 1.0, 1.0]


def test_reference_sheared_parallelogram():
    # centre 0, u = (1, 0, 0), v = (1, 1, 0): corners (-2,-1), (0,-1), (2,1), (0,1).  q = (2, 0, 0) has skewed coordinates
    # (a, b) = (2, 0); clamping a to 1 gives (1, 0, 0) at distance 1, but the nearest point lies on the edge from (0,-1) to
    # (2, 1), the line x - y = 1: the foot of q is (1.5, 0.5, 0) at distance sqrt(0.5).
    tri = cr.parallelogram_triangles([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0])
    dist, pt = cr.closest_on_triangles(tri, np.array([2.0, 0.0, 0.0]))
    k = int(np.argmin(dist))
    assert abs(dist[k] - np.sqrt(0.5)) <= 4e-16
    np.testing.assert_allclose(pt[k], [1.5, 0.5, 0.0], rtol=0, atol=4e-16)
    # a point above the interior: the plane distance
    dist, pt = cr.closest_on_triangles(tri, np.array([0.5, 0.25, -3.0]))
    assert dist.min() == 3.0


def test_reference_sphere_inside_outside_centre():
    c = np.array([1.0, 2.0, 3.0])
    d, p, n = cr.closest_on_sphere(c, 2.0, np.array([1.0, 2.0, 8.0]))       # outside, 5 from the centre
    assert d == 3.0 and p.tolist() == [1.0, 2.0, 5.0] and n.tolist() == [0.0, 0.0, 1.0]
    d, p, n = cr.closest_on_sphere(c, 2.0, np.array([1.0, 1.5, 3.0]))       # inside, 0.5 from the centre
    assert d == 1.5 and p.tolist() == [1.0, 0.0, 3.0] and n.tolist() == [0.0, -1.0, 0.0]
    d, p, n = cr.closest_on_sphere(c, -2.0, np.array([1.0, 2.0, 3.0]))      # the centre of a hollow sphere: towards +x
    assert d == 2.0 and p.tolist() == [3.0, 2.0, 3.0] and n.tolist() == [1.0, 0.0, 0.0]


def test_reference_on_a_scene():
    hs = api.HostScene(["tests/scenes/polished", "-w=8"])
    ref = cr.Reference(hs.desc)
    assert len(ref.spheres) == 4 and len(ref.tri) == 2 * 4
    radii = sorted(r for _, _, r in ref.spheres)
    assert abs(radii[2] - 0.7) <= 1e-15     # the sphere of radius 0.5 under s=1.4
    # the point 0.3 above the scaled sphere's top: that sphere, at 0.3
    d_ref, near, _ = ref.query(np.array([2.1, 0.7 + 0.7 + 0.3, -1.0]), 1e-12)
    assert abs(d_ref - 0.3) <= 1e-15 and len(near) == 1


# ---- the kernel's routines in numpy float32 against the f64 reference, at the f32 bound ----
def test_f32_constants():
    assert pb.K_DIST >= pb.K_FLOOR == 8.0 and np.log2(pb.K_DIST) == int(np.log2(pb.K_DIST))


def _hold(d32, c32, d64, on_prim, q, extent):
    L = max(float(np.abs(q).max()), extent)
    assert abs(d32 - d64) <= pb.K_DIST * pb.U * L, (d32, d64)
    assert on_prim(c32) <= pb.K_DIST * pb.U * L, on_prim(c32)


def test_f32_restatement_on_known_answers():
    for q, _, _ in VORONOI:
        q = np.array(q)
        d32, c32 = pb.triangles_f32(UNIT, q)
        d64, _ = cr.closest_on_triangles(UNIT, q)
        _hold(d32[0], c32[0], d64[0], lambda p: cr.closest_on_triangles(UNIT, p)[0][0], q, 1.0)
    c = np.array([1.0, 2.0, 3.0])
    for q in ([1.0, 2.0, 8.0], [1.0, 1.5, 3.0], [1.1, 2.2, 3.3], [100.0, -50.0, 7.0]):
        q = np.array(q)
        d32, p32, _ = pb.sphere_f32(c, 2.0, q)
        d64, _, _ = cr.closest_on_sphere(c, 2.0, q)
        _hold(d32, p32, d64, lambda p: cr.closest_on_sphere(c, 2.0, p)[0], q, 5.0)


def test_f32_restatement_on_two_meshes_near_surface_points():
    hs = api.HostScene(["tests/scenes/two_meshes", "-w=8"])
    ref = cr.Reference(hs.desc)
    pts = cr.point_sets(ref, np.random.default_rng(31))["near"]
    worst = 0.0
    for q in pts:
        d64, _ = cr.closest_on_triangles(ref.tri, q)
        d32, c32 = pb.triangles_f32(ref.tri, q)
        k = int(np.argmin(d32))
        L = max(float(np.abs(q).max()), ref.extent)
        on = cr.closest_on_triangles(ref.tri[k:k + 1], c32[k])[0][0]
        worst = max(worst, abs(d32[k] - d64.min()) / (pb.U * L), max(0.0, d64[k] - d64.min()) / (2 * pb.U * L), on / (pb.U * L))
    print(f"[f32 restatement] two_meshes near-surface points: largest ratio {worst:.2f} (K_DIST {pb.K_DIST:g})")
    assert worst <= pb.K_DIST
