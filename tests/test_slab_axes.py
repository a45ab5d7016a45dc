"""Slab-only axes of the mesh BVH (rt_bvh.cpp build_mesh_slab_axes, rule in rt_refit.h), without a GPU.

An inner child of a 4-wide mesh node that has no back-face cone gets the cone word (qx, qy, qz, 127) with q from a fixed table
of 46 integer directions, |q|_2 <= 126: the cone test can never cull with it, and the slab step reads its axis.  Checked here on
five meshes and with both conditioning limits (f64, f32):
 1. every slab-only word has w = 127, 0 < |q|_2 <= 126, sits on an inner child and is a table entry;
 2. no slab-only word culls for any packed direction of the 10 586-direction lattice of tests/test_mesh_cones.py, nor for the
    packed direction nearest its own axis (both signs), in the kernel's integer arithmetic;
 3. children above an ill-conditioned triangle and empty children are neutral in both words, and so is every leaf without a cone;
 4. the slab of every slab-only child holds every corner below it by the builder's margin;
 5. the chosen word equals a numpy restatement of the rule over the same table (same operation order in float64);
 6. RT_SLAB_AXES=0 gives words without any slab-only axis that otherwise equal the default's, and on monkey.obj the words
    recorded from the parent commit (tests/golden/slab_axes_parent_monkey.npz);
 7. on the knot and on Suzanne at least one child that had no cone gets an axis."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from rust_raytracer_amd import api
from scene_update_cases import mesh_arrays
from test_mesh_cones import EMPTY, NEUTRAL, SIGMA, degenerate_obj, lattice_directions, mesh_scene, pack_direction, triangles_below

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "slab_axes_parent_monkey.npz")
NEUTRAL_SLAB = 0x7FFF8000
MAX_RATIO = 0.9
MESHES = ("suzanne", "knot", "degenerate", "tube", "crumpled")


def axis_table():
    """rt_refit.h rf_slab_axis, restated: integer directions with components in -2..2, at least two non-zero, the first non-zero
    one positive, reduced; times the largest integer that keeps |q|_2 <= 126; ordered by (largest / smallest non-zero |component|,
    number of non-zero components), ties in lexicographic order."""
    out = []
    for v in itertools.product(range(-2, 3), repeat=3):
        nz = [c for c in v if c]
        if len(nz) < 2 or nz[0] < 0 or math.gcd(math.gcd(abs(v[0]), abs(v[1])), abs(v[2])) != 1:
            continue
        s = int(126 / math.sqrt(sum(c * c for c in v)))
        out.append(tuple(c * s for c in v))
    out.sort(key=lambda q: (max(abs(c) for c in q) // min(abs(c) for c in q if c), sum(1 for c in q if c)))
    t = np.array(out, dtype=np.int64)
    assert t.shape == (46, 3) and ((t * t).sum(axis=1) <= 126 * 126).all() and np.abs(t).sum(axis=1).max() == 216
    return t


TABLE = axis_table()


def tube_obj(path, n_u=64, n_v=16):
    """A closed torus-like tube, 2 n_u n_v = 2048 triangles, whose cross-section is flattened: thin along directions that turn."""
    lines = ["vt 0 0", "vn 0 1 0"]
    for i in range(n_u):
        for j in range(n_v):
            u, v = 2 * np.pi * i / n_u, 2 * np.pi * j / n_v
            r = 1.0 + 0.25 * np.cos(v)
            lines.append(f"v {float(r * np.cos(u))!r} {float(0.08 * np.sin(v) + 0.3 * np.sin(2 * u))!r} {float(r * np.sin(u))!r}")
    idx = lambda i, j: (i % n_u) * n_v + (j % n_v) + 1
    for i in range(n_u):
        for j in range(n_v):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            lines += [f"f {a}/1/1 {c}/1/1 {b}/1/1", f"f {a}/1/1 {d}/1/1 {c}/1/1"]
    path.write_text("\n".join(lines) + "\n")


def crumpled_obj(path, n=16):
    """A 16 x 16 patch (512 triangles) in the plane x + y + z = 0, crumpled by a checkerboard of steep spikes (slopes of about
    80 degrees): the normals of neighbouring triangles differ by more than a cone holds, so most inner children have none."""
    e1, e2, nn = np.array([1.0, -1.0, 0.0]) / np.sqrt(2), np.array([1.0, 1.0, -2.0]) / np.sqrt(6), np.array([1.0, 1.0, 1.0]) / np.sqrt(3)
    rng = np.random.default_rng(11)
    lines = ["vt 0 0", "vn 0 1 0"]
    for j in range(n + 1):
        for i in range(n + 1):
            x, z = -1 + 2 * i / n, -1 + 2 * j / n
            h = 0.8 * (1 if (i + j) % 2 else -1) * rng.uniform(0.7, 1.0)
            p = x * e1 + z * e2 + h * nn
            lines.append(f"v {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}")
    idx = lambda i, j: j * (n + 1) + i + 1
    for j in range(n):
        for i in range(n):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            lines += [f"f {a}/1/1 {c}/1/1 {b}/1/1", f"f {a}/1/1 {d}/1/1 {c}/1/1"]
    path.write_text("\n".join(lines) + "\n")


def make_mesh(name, d):
    if name == "suzanne":
        return os.path.join(REPO, "scenes", "resource", "monkey.obj")
    obj = d / f"{name}.obj"
    if name == "knot":
        subprocess.run([os.path.join(REPO, "tools", "gen_dragon"), str(obj), "40", "40"], check=True)
    elif name == "degenerate":
        degenerate_obj(obj)
    elif name == "tube":
        tube_obj(obj)
    else:
        crumpled_obj(obj)
    return str(obj)


def words_of(desc, prec, axes, monkeypatch):
    """Everything the checks read, derived with RT_SLAB_AXES unset (axes = True) or 0."""
    if axes:
        monkeypatch.delenv("RT_SLAB_AXES", raising=False)
    else:
        monkeypatch.setenv("RT_SLAB_AXES", "0")
    try:
        f32 = prec == "f32"
        children, cones, tris64 = api.scene_mesh_cones(desc, 0, f32)
        sl = api.scene_mesh_slabs(desc, 0, f32)
        order = api.scene_refit_mesh(desc, desc, 0, f32)["order"]
    finally:
        monkeypatch.delenv("RT_SLAB_AXES", raising=False)
    return children, cones, tris64, sl, order


@pytest.fixture(scope="module")
def meshes(tmp_path_factory):
    d = tmp_path_factory.mktemp("slab_axes")
    out = {}
    for name in MESHES:
        sub = d / name
        sub.mkdir()
        out[name] = mesh_scene(sub, make_mesh(name, sub))
    return out


def slab_only_mask(cones):
    q = cones[..., :3].astype(np.int64)
    l2 = (q * q).sum(axis=-1)
    return (cones[..., 3] == 127) & (l2 > 0) & (l2 <= 126 * 126)


def restated_pick(blo, bhi, corners):
    """rf_slab_axis_pick over the corners (m, 3) below a child with the exact box (blo, bhi): the table index, or -1."""
    ext = bhi - blo
    if not ((ext > 0) & np.isfinite(ext)).all():
        return -1
    q = TABLE.astype(np.float64)
    p = (q[:, None, 0] * corners[None, :, 0] + q[:, None, 1] * corners[None, :, 1]) + q[:, None, 2] * corners[None, :, 2]   # (46, m)
    num = p.max(axis=1) - p.min(axis=1)
    a = np.abs(q)
    den = (a[:, 0] * ext[0] + a[:, 1] * ext[1]) + a[:, 2] * ext[2]
    ratio = num / den
    best = int(np.argmin(ratio))   # the first of equals
    return best if ratio[best] < MAX_RATIO else -1


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", MESHES)
def test_slab_only_words(meshes, monkeypatch, name, prec):
    hs = meshes[name]
    children, cones, tris64, sl, order = words_of(hs.desc, prec, True, monkeypatch)
    children0, cones0, _, sl0, _ = words_of(hs.desc, prec, False, monkeypatch)
    words, bounds, org, inv_s, pad = sl["words"], sl["bounds"], sl["org"], sl["inv_s"], sl["pad"]
    real = children != EMPTY
    inner = children >= 0
    neutral = (cones == NEUTRAL).all(axis=-1)
    only = slab_only_mask(cones)
    below = triangles_below(children)
    v0 = tris64[:, 0, :]
    corners = np.stack([v0, v0 + tris64[:, 1, :], v0 + tris64[:, 2, :]], axis=1)   # (t, 3, 3), as the builder forms them
    pos, tri = mesh_arrays(hs.desc)
    exact = pos[tri[order]]                                                        # (slot, 3, 3): the vertices the exact boxes are built from

    # 6. the switch: no slab-only word, every other word unchanged
    assert np.array_equal(children0, children)
    assert not slab_only_mask(cones0).any()
    assert np.array_equal(cones0[~only], cones[~only]) and np.array_equal(sl0["words"][~only], words[~only])
    assert (cones0[only] == NEUTRAL).all() and (sl0["words"][only] == NEUTRAL_SLAB).all()

    # 1. shape of the words
    assert (only <= inner).all(), "a slab-only word on a leaf or an empty child"
    table = {tuple(q) for q in TABLE}
    for i, k in zip(*np.nonzero(only)):
        assert tuple(int(x) for x in cones[i, k, :3]) in table
    assert (words[only] != NEUTRAL_SLAB).all(), "a slab-only word without a slab"
    assert (words[neutral] == NEUTRAL_SLAB).all()

    # 2. never culls: dq . q - 127 x 127 > 0 for no packed direction
    if only.any():
        q = cones[only][:, :3].astype(np.int64)
        for R in (np.float64, np.float32):
            dq = pack_direction(lattice_directions().astype(R)).astype(np.int64)
            assert (dq @ q.T - 127 * 127 <= 0).all()
            for sign in (1.0, -1.0):
                own = pack_direction((sign * q.astype(np.float64) * 0.37).astype(R)).astype(np.int64)
                assert ((own * q).sum(axis=1) - 127 * 127 <= 0).all()
        assert (np.array([0, 0, 0, -127]) @ np.array([1, 1, 1, 127]) <= 0)   # kNoCullDir has no direction bytes at all

    # 3. neutral where the rule says so
    c64 = np.cross(tris64[:, 1, :], tris64[:, 2, :])
    l1, l2, lc = (np.sqrt((x * x).sum(axis=1)) for x in (tris64[:, 1, :], tris64[:, 2, :], c64))
    bad = ~(lc >= SIGMA[prec] * l1 * l2) | ~(lc > 0) | ~np.isfinite(tris64).all(axis=(1, 2))
    assert neutral[~real].all() and (words[~real] == NEUTRAL_SLAB).all()
    for i in range(len(children)):
        for k in range(4):
            if real[i, k] and bad[below[i][k]].any():
                assert neutral[i, k] and words[i, k] == NEUTRAL_SLAB, f"child {k} of node {i} stands above an ill-conditioned triangle"

    # 4. the slab holds the corners by the margin; 5. the restated rule, on every inner child that the cones left neutral
    neutral0 = (cones0 == NEUTRAL).all(axis=-1)
    n_fit = 0
    for i, k in zip(*np.nonzero(inner & neutral0)):
        idx = below[i][k]
        contiguous = len(idx) > 0 and idx[-1] - idx[0] + 1 == len(idx)
        want = -1
        if contiguous and not bad[idx].any():
            ex = exact[idx].reshape(-1, 3)
            want = restated_pick(ex.min(axis=0), ex.max(axis=0), corners[idx].reshape(-1, 3))
        if want < 0:
            assert neutral[i, k], f"child {k} of node {i}: an axis where the rule gives none"
            continue
        assert only[i, k] and tuple(cones[i, k, :3]) == tuple(TABLE[want]), \
            f"child {k} of node {i}: word {cones[i, k]} but the rule picks {TABLE[want]}"
        n_fit += 1
        q = cones[i, k, :3].astype(np.float64)
        p = ((corners[idx].reshape(-1, 3) - org[i].astype(np.float64)) * float(inv_s[i])) @ q
        margin = np.abs(q).sum() * (2.0 * pad * float(inv_s[i]) + 2.0 ** -12)
        lo, hi = float(bounds[i, k, 0]), float(bounds[i, k, 1])
        slack = margin * (1 - 1e-9) - 1e-9
        assert (lo == -32768.0 or p.min() - slack >= lo) and (hi == 32767.0 or p.max() + slack <= hi), \
            f"child {k} of node {i}: a corner lies closer than the margin to the slab's bound"
    assert n_fit == int(only.sum())
    print(name, prec, {"inner": int(inner.sum()), "without_cone": int((inner & neutral0).sum()), "slab_only": n_fit})
    # 7. not vacuous
    if name in ("suzanne", "knot", "tube"):
        assert n_fit >= 1
    if name == "crumpled":
        assert (inner & neutral0).sum() > 0.5 * inner.sum(), "the crumpled patch is meant to leave most inner children without a cone"


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_switch_reproduces_the_parent_words(meshes, monkeypatch, prec):
    """tests/golden/slab_axes_parent_monkey.npz: children, cone words and slab words of scenes/resource/monkey.obj as the commit
    before the slab axes derived them."""
    children, cones, _, sl, _ = words_of(meshes["suzanne"].desc, prec, False, monkeypatch)
    g = np.load(GOLDEN)
    assert np.array_equal(children, g["children"])
    assert np.array_equal(cones.view(np.uint32).reshape(-1, 4), g[f"cones_{prec}"])
    assert np.array_equal(sl["words"], g[f"slabs_{prec}"])
