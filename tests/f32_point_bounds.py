"""Bounds on the f32 answers of the point queries (rt_closest_points with RT_PRECISION_F32), DESIGN.md section 20.

With u = 2^-24 and, per point q, L = max(|q|inf, extent), extent = the largest |world coordinate| of the scene's primitives:
  (1) |d32 - d_ref| <= K_DIST u L                                  the distance against the f64 brute-force minimum;
  (2) ref distance(q, reported primitive) <= d_ref + 2 K_DIST u L   the primitive reported is (nearly) a nearest one;
  (3) ref distance(pos, reported primitive) <= K_DIST u L           the reported point lies on that primitive.
All three hold for every point of a set.

K_DIST is set the way tests/f32_ray_bounds.py sets K_POS: the smallest power of two at least 4x the largest ratio measured on
the MI355X against tests/closest_points_ref.py over the scenes and point sets of tests/test_gpu_closest_points.py (the table is in
DESIGN.md section 20), and never below the derived floor of 8 (rounding of q to f32: 1; of the primitive's table numbers: 1; one
f32 transform level, four roundings of numbers up to L each way: 4; the test itself: 2)."""
import numpy as np

from closest_points_ref import closest_on_sphere, closest_on_triangles

U = 2.0 ** -24
K_FLOOR = 8.0
K_DIST = 2.0 ** 3   # largest measured ratio 1.85 (sun_sky, the distance): 4 x 1.85 = 7.4; the table is in DESIGN.md section 20


def ratios(ref, q, d32, pos32, node, prim, d_ref):
    """The three ratios (left-hand side / (u L)) for one found point."""
    L = max(float(np.abs(q).max()), ref.extent)
    r1 = abs(d32 - d_ref) / (U * L)
    r2 = max(0.0, ref.distance_to(q, node, prim) - d_ref) / (U * L)
    r3 = ref.distance_to(pos32, node, prim) / (U * L)
    return r1, r2, r3


def check(ref, points, got, d_refs, label, k_dist=K_DIST, show=True):
    """Asserts (1)-(3) for every point; returns the largest ratio of each."""
    worst = np.zeros(3)
    for q, g, d_ref in zip(points, got, d_refs):
        assert np.isfinite(d_ref) and g["flags"] & 1, f"{label}: point {q} not found"
        r = ratios(ref, q, float(g["distance"]), g["pos"], int(g["node"]), int(g["prim"]), d_ref)
        worst = np.maximum(worst, r)
    if show:
        print(f"[f32 point bounds] {label}: n={len(points)} largest ratios distance {worst[0]:.2f} primitive {worst[1]:.2f} "
              f"position {worst[2]:.2f} (K_DIST {k_dist:g}, primitive bar 2 K_DIST)")
    assert worst[0] <= k_dist and worst[1] <= 2 * k_dist and worst[2] <= k_dist, (label, worst.tolist())
    return worst


# ---- the kernel's arithmetic restated in numpy float32 (CPU test) ----
def triangles_f32(tri, q):
    """closest_on_triangle in float32 on the f32-rounded corners: (distance, point) per triangle, as float64."""
    d, c = closest_on_triangles(np.asarray(tri, dtype=np.float32), np.asarray(q, dtype=np.float32))
    assert d.dtype == np.float32 and c.dtype == np.float32
    return d.astype(np.float64), c.astype(np.float64)


def sphere_f32(centre, radius, q):
    d, c, n = closest_on_sphere(np.asarray(centre, dtype=np.float32), np.float32(radius), np.asarray(q, dtype=np.float32))
    assert np.asarray(d).dtype == np.float32
    return float(d), c.astype(np.float64), n.astype(np.float64)
