"""Back-face cones of the mesh BVH (rt_bvh.cpp build_mesh_cones, read by k_wf_mesh), without a GPU.

k_wf_mesh skips a child of a 4-wide node when the integer product of the ray's packed direction (round(127 d / |d|), -127)
and the child's cone word (ax, ay, az, w) is positive.  That is only allowed if the triangle test would have rejected every
triangle below the child: det = e1 . (d x e2) < EPSILON (mesh.rs:77).  Here the words come from the diagnostic export
rt_scene_mesh_cones, the kernel's packing and its determinant are restated in numpy in the kernel's arithmetic type
(elementwise IEEE operations in the same order, no contraction), and the claim is checked for every child with a cone over
a lattice of 10 586 directions plus, per child, directions on the edge of its cone whose product is exactly 1 (the weakest
cull there is).  The test asks for det < 0, which is stronger than det < EPSILON."""
import os
import subprocess

import numpy as np
import pytest

from rust_raytracer_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = -2 ** 31
NEUTRAL = np.array([0, 0, 0, 127], dtype=np.int8)
# rt_bvh.cpp cone_limits(): a triangle with |e1 x e2| < sigma |e1| |e2| is ill-conditioned
SIGMA = {"f64": 2.0 ** -20, "f32": 2.0 ** -5}
DTYPE = {"f64": np.float64, "f32": np.float32}


def lattice_directions():
    """Every integer vector on the surface of the cube [-21, 21]^3 (10 586 directions, 2.7 degrees apart at most), at a
    length that is no power of two so that normalising them rounds."""
    r = np.arange(-21, 22)
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    g = g[np.abs(g).max(axis=1) == 21]
    assert len(g) == 10586
    return g.astype(np.float64) * 0.37


def pack_direction(d):
    """enter_mesh of k_wf_mesh, in d's dtype: the three direction bytes (the fourth is -127)."""
    R = d.dtype.type
    len2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    sc = R(127) / np.sqrt(len2)
    return np.rint(d * sc[..., None]).astype(np.int32)


def det_kernel(d, e1, e2):
    """dot(edge1, cross(d, edge2)) as rt_device.h evaluates it; d (..., 3) against e1, e2 (..., 3), broadcast."""
    cx = d[..., 1] * e2[..., 2] - d[..., 2] * e2[..., 1]
    cy = d[..., 2] * e2[..., 0] - d[..., 0] * e2[..., 2]
    cz = d[..., 0] * e2[..., 1] - d[..., 1] * e2[..., 0]
    return e1[..., 0] * cx + e1[..., 1] * cy + e1[..., 2] * cz


def triangles_below(children):
    """Per (node, child): sorted triangle indices below it, bottom-up (children stand behind their parent)."""
    n = len(children)
    below = [[None] * 4 for _ in range(n)]
    for i in range(n - 1, -1, -1):
        for k in range(4):
            c = int(children[i, k])
            if c == EMPTY:
                below[i][k] = np.zeros(0, dtype=np.int64)
            elif c < 0:
                code = ~c
                below[i][k] = np.arange(code >> 3, (code >> 3) + (code & 7) + 1, dtype=np.int64)
            else:
                assert c > i
                below[i][k] = np.sort(np.concatenate(below[c]))
    return below


def edge_directions(q, w, rng, per_child=512):
    """Directions on the edge of the cone (q, w): unit vectors whose cosine to the axis puts 127 d^ . q at 127 w + 1, all
    round the axis.  Rounding to bytes moves the integer product by up to +-|q| sqrt(3) / 2 around that, so some of
    them land on exactly 1."""
    qf = q.astype(np.float64)
    al = np.sqrt((qf * qf).sum())
    a = qf / al
    cos_t = min((127.0 * w + 1.0) / (127.0 * al), 1.0)
    sin_t = np.sqrt(max(0.0, 1.0 - cos_t * cos_t))
    h = np.array([1.0, 0.0, 0.0]) if abs(a[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    u = np.cross(a, h)
    u /= np.sqrt((u * u).sum())
    v = np.cross(a, u)
    phi = rng.uniform(0.0, 2.0 * np.pi, per_child)
    d = cos_t * a[None, :] + sin_t * (np.cos(phi)[:, None] * u[None, :] + np.sin(phi)[:, None] * v[None, :])
    return d * rng.uniform(0.5, 2.0, per_child)[:, None]


def check_mesh(desc, prec, expect_full_coverage):
    R = DTYPE[prec]
    children, cones, tris64 = api.scene_mesh_cones(desc, 0, prec == "f32")
    tris = tris64.astype(R)  # the records the kernel reads: the f64 records rounded to its type
    e1, e2 = tris[:, 1, :], tris[:, 2, :]
    below = triangles_below(children)
    real = children != EMPTY
    neutral = (cones == NEUTRAL).all(axis=-1)
    assert neutral[~real].all(), "an empty child carries a cone"
    assert ((cones[..., 3] >= 1) | neutral).all() and (cones[..., :3] > -128).all()

    # (b) ill-conditioned triangles (judged on the f64 records, like the builder): neutral word on every child above one
    c64 = np.cross(tris64[:, 1, :], tris64[:, 2, :])
    l1, l2, lc = (np.sqrt((x * x).sum(axis=1)) for x in (tris64[:, 1, :], tris64[:, 2, :], c64))
    bad = ~(lc >= SIGMA[prec] * l1 * l2) | ~(lc > 0) | ~np.isfinite(tris64).all(axis=(1, 2))
    n_above_bad = 0
    for i in range(len(children)):
        for k in range(4):
            if real[i, k] and bad[below[i][k]].any():
                n_above_bad += 1
                assert neutral[i, k], f"child {k} of node {i} has a cone above an ill-conditioned triangle"

    # (a) the lattice: det of every (triangle, direction), then per child "culled => every triangle below has det < 0"
    dirs = lattice_directions().astype(R)
    dq_all = pack_direction(dirs)                                   # (D, 3)
    assert (np.abs(dq_all) <= 127).all()
    with_cone = [(i, k) for i in range(len(children)) for k in range(4) if not neutral[i, k]]
    leaf_pairs = leaf_culled = 0
    for d0 in range(0, len(dirs), 2048):
        dch, dq = dirs[d0:d0 + 2048], dq_all[d0:d0 + 2048]
        not_neg = np.zeros((len(tris) + 1, len(dch)), dtype=np.int32)  # prefix sums over the triangles of !(det < 0)
        for t0 in range(0, len(tris), 256):
            det = det_kernel(dch[None, :, :], e1[t0:t0 + 256, None, :], e2[t0:t0 + 256, None, :])
            not_neg[t0 + 1:t0 + 1 + det.shape[0]] = ~(det < 0)
        np.cumsum(not_neg, axis=0, out=not_neg)
        for i, k in with_cone:
            idx = below[i][k]
            q, w = cones[i, k, :3].astype(np.int32), int(cones[i, k, 3])
            culled = dq @ q - 127 * w > 0
            if idx[-1] - idx[0] + 1 == len(idx):
                wrong = not_neg[idx[-1] + 1] - not_neg[idx[0]]
            else:
                wrong = (not_neg[idx + 1] - not_neg[idx]).sum(axis=0)
            assert not (culled & (wrong != 0)).any(), \
                f"child {k} of node {i}: culled for a lattice direction although a triangle below it has det >= 0"
            if children[i, k] < 0:
                leaf_pairs += len(dch)
                leaf_culled += int(culled.sum())
    # the weakest culls of every child: product exactly 1 (and the next weakest edge directions that cull)
    rng = np.random.default_rng(7)
    n_exact_one, n_with_cone = 0, len(with_cone)
    for i, k in with_cone:
        idx = below[i][k]
        q, w = cones[i, k, :3].astype(np.int32), int(cones[i, k, 3])
        ed = edge_directions(q, w, rng).astype(R)
        prod = pack_direction(ed) @ q - 127 * w
        sel = np.flatnonzero(prod > 0)
        sel = sel[np.argsort(prod[sel], kind="stable")][:8]
        n_exact_one += int((prod == 1).any())
        if len(sel):
            det = det_kernel(ed[sel][:, None, :], e1[idx][None, :, :], e2[idx][None, :, :])
            assert (det < 0).all(), f"child {k} of node {i}: culled on the edge of its cone although det >= 0"
    leaf = real & (children < 0)
    inner = children >= 0
    stats = {"leaf_cones": float((~neutral[leaf]).mean()), "inner_cones": float((~neutral[inner]).mean()) if inner.any() else 1.0,
             "leaf_culled": leaf_culled / max(leaf_pairs, 1), "exact_one": n_exact_one / max(n_with_cone, 1),
             "above_bad": n_above_bad, "bad": int(bad.sum())}
    print(prec, stats)
    # the edge directions do reach the weakest cull: 512 products spread over about +-110 around 1 hit it for most children
    assert stats["exact_one"] >= 0.5
    if expect_full_coverage:
        # (c) not vacuous
        assert stats["leaf_cones"] == 1.0
        assert stats["inner_cones"] >= 0.75
        assert stats["leaf_culled"] >= 0.25
    return stats


def mesh_scene(tmp_path, obj):
    """A scene with the one mesh `obj` (assets are named relative to the scene file)."""
    scene = tmp_path / "scene"
    obj = os.path.relpath(obj, str(tmp_path))
    scene.write_text(f"m: mesh {obj} (lambertian (constant 0.7,0.7,0.7))\nsky: sky (constant 1,1,1)\nworld: list $m $sky\nlights: list $sky\n")
    return api.HostScene([str(scene), "-w=16", "-s=1"])


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_cones_cull_only_back_facing_triangles_suzanne(tmp_path, prec):
    hs = mesh_scene(tmp_path, os.path.join(REPO, "scenes", "resource", "monkey.obj"))
    check_mesh(hs.desc, prec, expect_full_coverage=True)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_cones_cull_only_back_facing_triangles_knot_surface(tmp_path, prec):
    obj = tmp_path / "knot.obj"
    subprocess.run([os.path.join(REPO, "tools", "gen_dragon"), str(obj), "40", "40"], check=True)
    hs = mesh_scene(tmp_path, str(obj))
    check_mesh(hs.desc, prec, expect_full_coverage=True)


def degenerate_obj(path):
    """A bumpy 12 x 12 grid (288 well-shaped triangles) and, spread over it just above the surface: a zero-area triangle, a sliver with
    |e1 x e2| = 1e-9 |e1| |e2|, and two coincident triangles of opposite winding."""
    n = 12
    lines = ["vt 0 0", "vn 0 1 0"]
    for j in range(n + 1):
        for i in range(n + 1):
            x, z = -1 + 2 * i / n, -1 + 2 * j / n
            lines.append(f"v {x!r} {float(0.3 * np.sin(2.1 * x) * np.cos(1.7 * z))!r} {z!r}")
    idx = lambda i, j: j * (n + 1) + i + 1
    for j in range(n):
        for i in range(n):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            lines += [f"f {a}/1/1 {c}/1/1 {b}/1/1", f"f {a}/1/1 {d}/1/1 {c}/1/1"]
    base = (n + 1) * (n + 1)
    extra = [(-0.9, 0.1, -0.8), (-0.8, 0.1, -0.8), (-0.7, 0.1, -0.8),      # collinear: zero area
             (0.7, 0.1, 0.8), (0.9, 0.1, 0.8), (0.9, 0.1 + 2e-10, 0.8),      # e1 = (0.2, 0, 0), e2 = (0.2, 2e-10, 0)
             (-0.1, 0.35, 0.0), (0.1, 0.35, 0.0), (0.0, 0.35, 0.15)]         # used twice, once in each winding
    for p in extra:
        lines.append(f"v {p[0]!r} {p[1]!r} {p[2]!r}")
    v = lambda k: base + k
    lines += [f"f {v(1)}/1/1 {v(2)}/1/1 {v(3)}/1/1", f"f {v(4)}/1/1 {v(5)}/1/1 {v(6)}/1/1",
              f"f {v(7)}/1/1 {v(8)}/1/1 {v(9)}/1/1", f"f {v(7)}/1/1 {v(9)}/1/1 {v(8)}/1/1"]
    path.write_text("\n".join(lines) + "\n")


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_cones_on_degenerate_triangles(tmp_path, prec):
    degenerate_obj(tmp_path / "deg.obj")
    hs = mesh_scene(tmp_path, str(tmp_path / "deg.obj"))
    st = check_mesh(hs.desc, prec, expect_full_coverage=False)
    assert st["bad"] == 2 and st["above_bad"] >= 2   # the zero-area triangle and the sliver: their leaf and the inner children above it
    # the coincident pair of opposite winding: no direction may cull a child that holds both (checked by (a): one of the two
    # always has det >= 0 unless the ray lies in their plane); the well-shaped part of the mesh still has cones
    assert st["leaf_cones"] > 0.5
