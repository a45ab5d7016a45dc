"""Normal slabs of the mesh BVH (rt_bvh.cpp build_mesh_slabs, read by k_wf_mesh through node4q_cull_slabs), without a GPU.

Per child with a cone the node carries [lo, hi], two signed 16-bit integers that bound P(x) = q . (x - org) / s over every
vertex x below the child (q: the three axis bytes of the child's cone word, org: the node's grid origin, s = 4 x its largest
cell), widened by the builder's margin |q|_1 (2 m / s + 2^-12) with m the pad of the mesh's boxes.  k_wf_mesh drops an
entered child when the culling ray's span [tn, tf] inside the child's box evaluates wholly below lo or wholly above hi.

The words come from the diagnostic export rt_scene_mesh_slabs, the tree and the triangle records from rt_scene_mesh_cones
and the decoded child boxes from rt_scene_refit_mesh: all three read the tables that rt_tables.cpp derives for the device
itself, not a second computation of them (tests/test_gpu_scene_tables.py holds the upload to those tables).  Checked here:
 1. every vertex below a child lies inside the decoded slab by at least the stated margin;
 2. the device step, restated in numpy float32 (fmaf as the correctly rounded float64 product plus addend, rounded once more to
    float32: the product of two float32 is exact in float64), never drops a child for a ray aimed at a point of a triangle
    below it - centroids, vertices and edge midpoints, origins along a lattice of directions far from the mesh and close to
    the point, with the exact ray in float64 and in float32.  tn and tf are the slab distances of the decoded child box
    (fma(plane, iv, -o iv) per plane, the form of the unquantised nodes; the kernel's differs from it by one rounding);
 3. children without a cone, empty children included, carry the word of a child without a slab."""
import os
import subprocess

import numpy as np
import pytest

from rust_raytracer_amd import api
from test_mesh_cones import EMPTY, NEUTRAL, degenerate_obj, mesh_scene, triangles_below

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEUTRAL_SLAB = 0x7FFF8000
DTYPE = {"f64": np.float64, "f32": np.float32}
F = np.float32


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def lattice(n=3):
    """Integer vectors on the surface of the cube [-n, n]^3 (218 for n = 3), at a length that is no power of two."""
    r = np.arange(-n, n + 1)
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    return g[np.abs(g).max(axis=1) == n].astype(np.float64) * 0.37


def tables(desc, prec):
    f32 = prec == "f32"
    children, cones, tris64 = api.scene_mesh_cones(desc, 0, f32)
    sl = api.scene_mesh_slabs(desc, 0, f32)
    boxes = api.scene_refit_mesh(desc, desc, 0, f32)["boxes"]
    assert sl["words"].shape == children.shape and boxes.shape[:2] == children.shape
    return children, cones, tris64, sl, boxes


def corners_of(tris64):
    v0 = tris64[:, 0, :]
    return np.stack([v0, v0 + tris64[:, 1, :], v0 + tris64[:, 2, :]], axis=1)   # (t, 3, 3), as the builder forms them


def cull_step(R, o, d, mesh_lo, mesh_hi, box_lo, box_hi, org, inv_s, q, lo, hi):
    """enter_mesh's culling ray and node4q_cull_slabs for N rays (o, d in R) against one child each.  Returns (entered, dropped)."""
    big = R(1e150) if R is np.float64 else R(1e18)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = R(1) / d
        inv = np.where(np.abs(inv) > big, np.copysign(big, inv), inv)
        e0, e1 = (mesh_lo - o) * inv, (mesh_hi - o) * inv
        t_enter = np.maximum(np.minimum(e0, e1).max(axis=1), R(0))
        t_shift = np.where(np.abs(t_enter) < np.inf, t_enter, R(0)).astype(R)
        oc = o + d * t_shift[:, None]                                      # make_cull_ray: the culling ray's origin
        iv = F(1) / d.astype(F)
        iv = np.where(np.abs(iv) > F(1e18), np.copysign(F(1e18), iv), iv).astype(F)
        oi = oc.astype(F) * iv
        neg = iv < 0
        near, far = np.where(neg, box_hi, box_lo), np.where(neg, box_lo, box_hi)
        tn = np.maximum(fma32(near, iv, -oi).max(axis=1), F(0))
        tf = fma32(far, iv, -oi).min(axis=1)                              # tmax32 = +inf: no bound from another hit
        entered = tn <= tf
        # node4q_cull_slabs
        start = (d * t_shift[:, None] + o) if R is np.float64 else fma32(d, t_shift[:, None], o)
        r = ((start.astype(F) - org) * inv_s[:, None]).astype(F)
        e = (d.astype(F) * inv_s[:, None]).astype(F)
        em = np.abs(e).max(axis=1)
        gm = np.maximum(np.abs(org).max(axis=1) * inv_s, np.abs(r).max(axis=1))
        ok = (em > F(1e-20)) & (em < F(1e30)) & (gm < F(65536))
        e[:, 0] = np.where(ok, e[:, 0], F(np.nan))
        qf = q.astype(F)
        A = fma32(qf[:, 0], r[:, 0], fma32(qf[:, 1], r[:, 1], (qf[:, 2] * r[:, 2]).astype(F)))
        B = fma32(qf[:, 0], e[:, 0], fma32(qf[:, 1], e[:, 1], (qf[:, 2] * e[:, 2]).astype(F)))
        pn, pf = fma32(tn, B, A), fma32(tf, B, A)
        dropped = (np.fmax(pn, pf) < lo) | (np.fmin(pn, pf) > hi)     # fmaxf / fminf: a NaN operand is dropped
    return entered, dropped, ok


def check_mesh(desc, prec, expect_full_coverage):
    R = DTYPE[prec]
    children, cones, tris64, sl, boxes = tables(desc, prec)
    words, bounds, org, inv_s, pad = sl["words"], sl["bounds"], sl["org"], sl["inv_s"], sl["pad"]
    real = children != EMPTY
    no_cone = (cones == NEUTRAL).all(axis=-1)
    no_slab = words == NEUTRAL_SLAB
    # 3. no cone, no slab
    assert no_cone[~real].all() and no_slab[no_cone].all(), "a child without a cone carries a slab"
    np.testing.assert_array_equal(bounds[..., 0], (words & 0xFFFF).astype(np.uint16).view(np.int16).astype(F))
    np.testing.assert_array_equal(bounds[..., 1], (words >> 16).astype(np.uint16).view(np.int16).astype(F))
    assert pad > 0 and np.isfinite(pad)

    corners = corners_of(tris64)
    below = triangles_below(children)
    mesh_lo, mesh_hi = corners.reshape(-1, 3).min(axis=0), corners.reshape(-1, 3).max(axis=0)
    assert abs(pad - max(np.abs(mesh_lo).max(), np.abs(mesh_hi).max()) / 524288.0) <= 1e-12 * pad   # m = 2^-19 S
    if R is np.float32:   # the record's box, rounded outward
        mesh_lo, mesh_hi = np.nextafter(mesh_lo.astype(F), F(-np.inf)), np.nextafter(mesh_hi.astype(F), F(np.inf))
    with_slab = [(i, k) for i in range(len(children)) for k in range(4) if not no_slab[i, k]]

    # 1. the vertices inside the slab by the margin
    thickness = []
    for i, k in with_slab:
        q = cones[i, k, :3].astype(np.float64)
        x = corners[below[i][k]].reshape(-1, 3)
        p = ((x - org[i].astype(np.float64)) * float(inv_s[i])) @ q
        margin = np.abs(q).sum() * (2.0 * pad * float(inv_s[i]) + 2.0 ** -12)
        lo, hi = float(bounds[i, k, 0]), float(bounds[i, k, 1])
        slack = margin * (1 - 1e-9) - 1e-9
        assert (lo == -32768.0 or p.min() - slack >= lo) and (hi == 32767.0 or p.max() + slack <= hi), \
            f"child {k} of node {i}: a vertex lies closer than the margin to the slab's bound ({lo}, {p.min()}, {p.max()}, {hi}, margin {margin})"
        # how thin the slab is against what its box spans along the same axis
        blo, bhi = boxes[i, k, 0].astype(np.float64), boxes[i, k, 1].astype(np.float64)
        span = (np.abs(q) * (bhi - blo)).sum() * float(inv_s[i])
        thickness.append((hi - lo) / span if span > 0 else 1.0)

    # 2. the device step on rays aimed at points of the triangles below each child
    dirs = lattice()
    pts, who = [], []
    for n_child, (i, k) in enumerate(with_slab):
        idx = below[i][k]
        idx = idx[np.unique(np.linspace(0, len(idx) - 1, 4).astype(np.int64))]   # first, last and two between
        c = corners[idx]                                                        # (t, 3, 3)
        p = np.concatenate([c.mean(axis=1), c[:, 0], c[:, 1], c[:, 2], 0.5 * (c[:, 0] + c[:, 1]), 0.5 * (c[:, 1] + c[:, 2]),
                            0.5 * (c[:, 2] + c[:, 0])])
        pts.append(p)
        who.append(np.full(len(p), n_child))
    pts, who = np.concatenate(pts), np.concatenate(who)
    ik = np.array(with_slab)
    ni, nk = ik[who, 0], ik[who, 1]
    extent = float((mesh_hi.astype(np.float64) - mesh_lo.astype(np.float64)).max())
    args = (mesh_lo.astype(R), mesh_hi.astype(R), boxes[ni, nk, 0], boxes[ni, nk, 1], org[ni], inv_s[ni], cones[ni, nk, :3].astype(np.int32),
            bounds[ni, nk, 0], bounds[ni, nk, 1])
    n_rays = n_entered = n_in_range = 0
    for j in range(26):
        dsel = dirs[(who * 7 + j * 9) % len(dirs)]          # every child walks its own 26 of the 218 directions
        for dist in (10.0 * extent, 0.05 * extent):         # far from the mesh / close to the point, inside the mesh's box for most
            o = (pts - dsel * (dist / 0.37 / 3.0)).astype(R)
            d = dsel.astype(R)
            entered, dropped, ok = cull_step(R, o, d, *args)
            bad = entered & dropped
            assert not bad.any(), f"{int(bad.sum())} rays aimed at a triangle below a child lose that child to its slab, first: child " \
                                  f"{nk[bad][0]} of node {ni[bad][0]}, direction {dsel[bad][0]}, distance {dist}"
            n_rays += len(o)
            n_entered += int(entered.sum())
            n_in_range += int(ok.sum())
    stats = {"slabs": len(with_slab), "with_cone": int((~no_cone).sum()), "rays": n_rays, "entered": n_entered / max(n_rays, 1),
             "in_range": n_in_range / max(n_rays, 1), "median_thickness": float(np.median(thickness)) if thickness else 1.0}
    print(prec, stats)
    if expect_full_coverage:
        # not vacuous: every child with a cone has a slab, the rays do enter the boxes they are aimed into, the step's range
        # gate lets them through, and a slab is much thinner than its box along the same axis
        assert stats["slabs"] == stats["with_cone"] > 0
        assert stats["entered"] >= 0.99 and stats["in_range"] == 1.0
        assert stats["median_thickness"] < 0.5
    return stats


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_slabs_hold_their_triangles_suzanne(tmp_path, prec):
    hs = mesh_scene(tmp_path, os.path.join(REPO, "scenes", "resource", "monkey.obj"))
    check_mesh(hs.desc, prec, expect_full_coverage=True)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_slabs_hold_their_triangles_knot_surface(tmp_path, prec):
    obj = tmp_path / "knot.obj"
    subprocess.run([os.path.join(REPO, "tools", "gen_dragon"), str(obj), "40", "40"], check=True)
    hs = mesh_scene(tmp_path, str(obj))
    check_mesh(hs.desc, prec, expect_full_coverage=True)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_slabs_on_degenerate_triangles(tmp_path, prec):
    """A zero-area triangle, a sliver and a coincident pair of opposite winding (tests/test_mesh_cones.py): the children above
    the first two have no cone and so no slab; the pair's leaf has none either (no cone holds both normals)."""
    degenerate_obj(tmp_path / "deg.obj")
    hs = mesh_scene(tmp_path, str(tmp_path / "deg.obj"))
    st = check_mesh(hs.desc, prec, expect_full_coverage=False)
    assert 0 < st["slabs"] == st["with_cone"]
    children, cones, _, sl, _ = tables(hs.desc, prec)
    assert ((children != EMPTY) & (sl["words"] == NEUTRAL_SLAB)).sum() >= 3
