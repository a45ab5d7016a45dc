"""The mesh trees at 131 072 triangles (tests/test_tree_scale_host.py, tests/test_gpu_tree_scale.py): scenes/cornell_dragon
with the 256 x 256 stand-in surface of tools/gen_dragon for its mesh, three deformations of it, a checker of the exported
4-wide tree, and ray sets with the oracle's answers.

Why this size: it is kSlabsMinTriangles, so the f64 search kernels pick the headline's plan when no RT_WF_* variable is set;
the host-built BVH2 has 40 603 nodes (159 workgroups of k_refit_up<2>), the 4-wide tree 19 792 (78 workgroups of
k_refit_up<4>), k_refit_tris and k_fit_boxes get 512 workgroups, and the worst-case 4-wide stack is 28, beyond the 12 LDS
levels of k_wf_mesh.  The smaller meshes of the other refit tests fit one or two workgroups, where the arrival counters never
hand a node from one compute unit to another.

Deformations (a second HostScene of the same file, meshes[0].positions rewritten in place; rt_scene_update compares arrays):
  smooth   the formula of scene_update_cases.displaced_obj, amplitude 0.06: every vertex moves
  weld     pos[i] = pos[i + 1] for i = 0, 64, 128, ...: 1 024 vertices welded, 2 048 zero-area triangles (the NaN cone markers)
  stretch  x * 50, y * 0.02: three orders of magnitude between the axes; tables only, no frames, no oracle
Ray sets (RaySets): the recipe of tests/ray_query_cases.py at -w=48 - (a) 2 304 camera rays, (b) one follow-up per surface hit,
(c) segments between hit positions - with every oracle answer from one batched pyoracle.shade_rays call per set.  The scene's
camera sees the whole box: 2 093 of its rays hit a surface, 302 of them the mesh.  So that the mesh's tree carries most of
the answers, set (d) adds 2 304 rays aimed at triangle centroids from a sphere around the mesh; all of them hit the mesh.
Nothing generated is committed; the mesh is written once per session into a temporary directory."""
import atexit
import functools
import os
import pathlib
import shutil
import subprocess
import sys
import tempfile

import numpy as np

from oracle import pyoracle
from rust_raytracer_amd import api
from ray_query_cases import leaf_nodes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TRIS, N_POS = 131072, 65536
FRAME_ARGS = ("-w=48", "-s=4", "--seed=3")
RAY_ARGS = ("-w=48", "-s=1", "--seed=31")
DEFORMATIONS = ("smooth", "weld", "stretch")
EMPTY = np.int32(np.iinfo(np.int32).min)   # kEmptyChild
T_MIN, T_MAX = 1e-3, 0.999
DBL_MAX = sys.float_info.max
MISS, SURFACE, ENVIRONMENT = 0, 1, 2
DIGESTS = ("BvhNode", "BvhNode4f", "MeshNode4qc", "TriRec", "TriAttr", "mesh_bounds", "MeshOpRec")
# slots of a pyoracle.shade_rays record (include/rt_mi355.h, rt_debug_shade_rays)
R_T, R_POS, R_FRONT, R_MATERIAL = 0, slice(1, 4), 9, 10


@functools.lru_cache(maxsize=None)
def scene_file():
    """The scene file beside its generated mesh, written once."""
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="tree_scale_"))
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    subprocess.run([os.path.join(REPO, "tools", "gen_dragon"), str(tmp / "knot.obj"), "256", "256"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(REPO, "scenes", "cornell_dragon")).read()
    assert "resource/dragon_high.obj" in text
    (tmp / "cornell_dragon").write_text(text.replace("resource/dragon_high.obj", "knot.obj"))
    return str(tmp / "cornell_dragon")


def positions(hs):
    """meshes[0].positions of a HostScene as a writable (n, 3) view."""
    m = hs.desc.contents.meshes[0]
    return np.ctypeslib.as_array(m.positions, shape=(m.n_positions, 3))


def deform(pos, case):
    """Rewrites the (n, 3) array `pos` in place."""
    if case == "smooth":
        x, y, z = pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy()
        pos[:, 0] = x + 0.06 * np.sin(5 * y + 1)
        pos[:, 1] = y + 0.06 * np.sin(4 * z + 2)
        pos[:, 2] = z + 0.06 * np.sin(6 * x + 3)
    elif case == "weld":
        i = np.arange(0, len(pos) - 1, 64)
        pos[i] = pos[i + 1]
    elif case == "stretch":
        pos[:, 0] *= 50.0
        pos[:, 1] *= 0.02
    else:
        assert case == "base", case


@functools.lru_cache(maxsize=None)
def host_scene(case="base", args=FRAME_ARGS):
    """The HostScene of `case` ("base" or one of DEFORMATIONS), shared: nobody writes into it afterwards."""
    hs = api.HostScene([scene_file()] + list(args))
    deform(positions(hs), case)
    return hs


def flagged_scene(hs):
    """DeviceScene(hs.desc) with RT_SCENE_BVH_ON_DEVICE; the shared description gets its flags back."""
    d = hs.desc.contents
    d.flags |= api.RT_SCENE_BVH_ON_DEVICE
    try:
        return api.DeviceScene(hs.desc, 0)
    finally:
        d.flags &= ~api.RT_SCENE_BVH_ON_DEVICE


def zero_area_triangles(hs):
    m = hs.desc.contents.meshes[0]
    pos = positions(hs)
    tri = np.ctypeslib.as_array(m.tri_pos, shape=(m.n_triangles, 3))
    p0, p1, p2 = pos[tri[:, 0]], pos[tri[:, 1]], pos[tri[:, 2]]
    return int((np.cross(p1 - p0, p2 - p0) == 0).all(axis=1).sum())


# ---- the exported tree ----
def tree_extents(children, tris, n_tris):
    """Bottom-up over the exported 4-wide tree, asserting (a) and (b) of check_tree on the way.  Per (node, child):
    lo, hi (n, 4, 3) float64, the exact hull of v0, v0 + e1, v0 + e2 of every slot below it (empty: +inf, -inf), and
    first, end, count (n, 4): the slots below it."""
    children = np.asarray(children)
    n = len(children)
    assert children.shape == (n, 4) and children.dtype == np.int32 and n >= 1
    assert tris.shape == (n_tris, 3, 3) and np.isfinite(tris).all()
    empty = children == EMPTY
    inner = children >= 0
    leaf = ~empty & ~inner
    own = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], (n, 4))
    # (a) an inner child lies behind its parent; so every node but the root has exactly one parent and there is no cycle
    bad = inner & ((children <= own) | (children >= n))
    assert not bad.any(), f"(a) node {np.argwhere(bad)[0][0]}: inner child {children[bad][0]} is not above its parent's index (of {n} nodes)"
    refs = np.bincount(children[inner], minlength=n)
    odd = np.flatnonzero(refs != (np.arange(n) > 0))
    assert odd.size == 0, f"(a) node {odd[:1]} has {refs[odd[:1]]} parents"
    # (b) the leaf ranges cover every slot exactly once
    code = ~children[leaf].astype(np.int64)
    first_l, count_l = code >> 3, (code & 7) + 1
    assert (first_l + count_l <= n_tris).all(), f"(b) a leaf range ends at {int((first_l + count_l).max())}, beyond the {n_tris} slots"
    cover = np.zeros(n_tris + 1, dtype=np.int64)
    np.add.at(cover, first_l, 1)
    np.add.at(cover, first_l + count_l, -1)
    cover = np.cumsum(cover)[:n_tris]
    assert (cover == 1).all(), (f"(b) slot {int(np.flatnonzero(cover != 1)[0])} is covered {int(cover[cover != 1][0])} times "
                                f"({int((cover == 0).sum())} slots uncovered, {int((cover > 1).sum())} covered more than once)")
    # the corners of every slot, from the exported records themselves
    corners = np.stack([tris[:, 0], tris[:, 0] + tris[:, 1], tris[:, 0] + tris[:, 2]], axis=1)
    slot_lo, slot_hi = corners.min(axis=1), corners.max(axis=1)
    lo = np.full((n, 4, 3), np.inf)
    hi = np.full((n, 4, 3), -np.inf)
    first = np.zeros((n, 4), dtype=np.int64)
    end = np.zeros((n, 4), dtype=np.int64)
    count = np.zeros((n, 4), dtype=np.int64)
    k = np.arange(8)
    slots = np.minimum(first_l[:, None] + k, n_tris - 1)
    live = (k < count_l[:, None])[..., None]
    lo[leaf] = np.where(live, slot_lo[slots], np.inf).min(axis=1)
    hi[leaf] = np.where(live, slot_hi[slots], -np.inf).max(axis=1)
    first[leaf], end[leaf], count[leaf] = first_l, first_l + count_l, count_l
    first[empty] = n_tris   # neutral for the minimum below
    for i in range(n - 1, -1, -1):   # children before parents
        for j in np.flatnonzero(inner[i]):
            c = children[i, j]
            lo[i, j], hi[i, j] = lo[c].min(axis=0), hi[c].max(axis=0)
            first[i, j], end[i, j], count[i, j] = first[c].min(), end[c].max(), count[c].sum()
    gap = inner & (end - first != count)
    assert not gap.any(), f"(b) node {np.argwhere(gap)[0][0]} child {np.argwhere(gap)[0][1]}: {count[gap][0]} slots below it in [{first[gap][0]}, {end[gap][0]}): not one run"
    assert count[0].sum() == n_tris
    first[empty] = 0
    return lo, hi, first, end, count


def check_tree(children, boxes, tris, order, n_tris):
    """The export of rt_debug_scene_mesh / rt_scene_refit_mesh is a tree that loses nothing:
      (a) every inner child index is larger than its parent's;
      (b) the leaf ranges (~c: first = code >> 3, count = (code & 7) + 1; INT32_MIN marks an empty child) cover every slot
          0 .. n_tris - 1 exactly once, the slots below every inner child form one contiguous run, `order` is a permutation;
      (c) every decoded child box, widened to f64, contains v0, v0 + e1 and v0 + e2 of every slot below that child;
      (d) every empty child has lo > hi on some axis.
    Returns the largest slack: the most a box face lies outside the exact hull of what is below it."""
    children, boxes = np.asarray(children), np.asarray(boxes)
    n = len(children)
    assert boxes.shape == (n, 4, 2, 3) and boxes.dtype == np.float32
    order = np.asarray(order)
    assert order.shape == (n_tris,) and (np.sort(order) == np.arange(n_tris)).all(), "(b) order is no permutation of the triangles"
    lo, hi, _, _, _ = tree_extents(children, tris, n_tris)
    empty = children == EMPTY
    blo, bhi = boxes[:, :, 0, :].astype(np.float64), boxes[:, :, 1, :].astype(np.float64)
    with np.errstate(invalid="ignore"):
        below, above = lo - blo, bhi - hi   # >= 0 where the box contains its contents
    full = ~empty
    assert np.isfinite(blo[full]).all() and np.isfinite(bhi[full]).all(), "(c) a child box is not finite"
    bad = full[..., None] & ~((below >= 0) & (above >= 0))
    if bad.any():
        i, j, a = np.argwhere(bad)[0]
        raise AssertionError(f"(c) node {i} child {j} axis {a}: box [{blo[i, j, a]!r}, {bhi[i, j, a]!r}] does not contain [{lo[i, j, a]!r}, {hi[i, j, a]!r}] "
                             f"({int(bad.any(axis=2).sum())} children in all)")
    inverted = (boxes[:, :, 0, :] > boxes[:, :, 1, :]).any(axis=2)
    assert inverted[empty].all(), f"(d) node {np.argwhere(empty & ~inverted)[0][0]}: an empty child whose box is not inverted"
    return float(max(below[full].max(), above[full].max()))


def worst_stack(children):
    """CompiledScene::max_bvh4_stack of an exported tree (Collapser::build): the sum of (children - 1) over a path from the
    root, plus one, at its largest."""
    children = np.asarray(children)
    width = (children != EMPTY).sum(axis=1)
    above = np.zeros(len(children), dtype=np.int64)
    for i in range(len(children)):   # parents before children
        here = above[i] + max(int(width[i]) - 1, 0)
        above[i] = here
        for c in children[i][children[i] >= 0]:
            above[c] = here
    return int(above.max()) + 1


def cell_of(boxes, node, axis):
    """The quantisation cell of `node` on `axis`, from its decoded child boxes: they are org + q cell with q = 0 .. 255 and the
    cell the smallest power of two that fits (rf_quantise4), so the largest q lies in [128, 255]."""
    b = boxes[node].astype(np.float64)
    full = b[:, 0, axis] <= b[:, 1, axis]
    hull = b[full, 1, axis].max() - b[full, 0, axis].min()
    assert hull > 0
    return 2.0 ** (np.floor(np.log2(hull)) - 7)


# ---- rays ----
Expected = np.dtype([("klass", "i4"), ("t", "f8"), ("pos", "f8", (3,)), ("front", "?"), ("material", "i4")])


def oracle_answers(hs, o, d):
    """One batched oracle call (generator state 0, the search of Interval(0.001, inf)) -> Expected per ray."""
    rec, _ = pyoracle.shade_rays(hs.desc, hs.params, o, d, np.zeros(len(o), dtype=np.uint64))
    out = np.zeros(len(o), dtype=Expected)
    mat = rec[:, R_MATERIAL].astype(np.int32)
    hit = mat >= 0
    env = hit & ((rec[:, R_T] == np.inf) | (rec[:, R_T] == DBL_MAX))
    out["klass"] = np.where(hit, np.where(env, ENVIRONMENT, SURFACE), MISS)
    out["material"] = np.where(hit, mat, -1)
    out["t"] = np.where(hit, rec[:, R_T], np.inf)
    out["pos"] = np.where(hit[:, None], rec[:, R_POS], 0.0)
    out["front"] = hit & (rec[:, R_FRONT] != 0)
    return out


class RaySets:
    """The recipe of tests/ray_query_cases.py (camera rays, one follow-up per surface hit, segments between hit positions,
    numpy.random.default_rng(31)) on one description, every oracle answer from a batched call."""

    def __init__(self, hs):
        self.hs = hs
        cam, prm = hs.camera, hs.params
        rays = np.array([pyoracle.get_ray(cam, prm, 0, x, y, 0, 0) for y in range(cam.image_height) for x in range(cam.image_width)])
        self.cam_o, self.cam_d = np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:])
        self.cam_hits = oracle_answers(hs, self.cam_o, self.cam_d)
        rng = np.random.default_rng(31)
        P = self.cam_hits["pos"][self.cam_hits["klass"] == SURFACE]
        fd = []
        for _ in range(len(P)):
            v = rng.normal(size=3)
            fd.append(v / np.linalg.norm(v) * rng.uniform(0.5, 2))
        self.fu_o, self.fu_d = np.ascontiguousarray(P), np.array(fd).reshape(-1, 3)
        self.fu_hits = oracle_answers(hs, self.fu_o, self.fu_d)
        perm = rng.permutation(len(P))
        d = P[perm] - P
        keep = (perm != np.arange(len(P))) & (np.linalg.norm(d, axis=1) > 1e-6)
        self.seg_o, self.seg_d = np.ascontiguousarray(P[keep]), np.ascontiguousarray(d[keep])
        # the closest hit over (0.001, inf) lies inside (0.001, 0.999) iff something does
        seg = oracle_answers(hs, self.seg_o, self.seg_d)
        self.seg_occluded = (seg["klass"] == SURFACE) & (seg["t"] < T_MAX)
        # (d) aimed rays.  The scene's camera sees the whole box and the mesh fills an eighth of its frame, so a set of the
        # camera's size goes from a sphere around the mesh to the centroids of triangles drawn by numpy.random.default_rng(33)
        # (not unit length; what the ray meets first is the oracle's business).
        d = hs.desc.contents
        node = next(i for i in range(d.n_nodes) if d.nodes[i].type == api.RT_NODE_MESH)
        (m,) = leaf_nodes(hs.desc)[node]
        mesh = d.meshes[d.nodes[node].mesh]
        pos = np.ctypeslib.as_array(mesh.positions, shape=(mesh.n_positions, 3))
        tri = np.ctypeslib.as_array(mesh.tri_pos, shape=(mesh.n_triangles, 3))
        rng = np.random.default_rng(33)
        pick = rng.choice(mesh.n_triangles, size=len(self.cam_o), replace=False)
        target = np.concatenate([pos[tri[pick]].mean(axis=1), np.ones((len(pick), 1))], axis=1) @ m.T
        centre = np.concatenate([pos.mean(axis=0), [1.0]]) @ m.T
        v = rng.normal(size=(len(pick), 3))
        v[:, 1] = np.abs(v[:, 1])   # above the floor
        self.aim_o = np.ascontiguousarray(centre[:3] + 200.0 * v / np.linalg.norm(v, axis=1)[:, None])
        self.aim_d = np.ascontiguousarray((target[:, :3] - self.aim_o) * rng.uniform(0.5, 2, size=(len(pick), 1)))
        self.aim_hits = oracle_answers(hs, self.aim_o, self.aim_d)
        self.mesh_materials = [d.nodes[node].material]

    @property
    def o(self):
        return np.concatenate([self.cam_o, self.fu_o, self.aim_o])

    @property
    def d(self):
        return np.concatenate([self.cam_d, self.fu_d, self.aim_d])

    @property
    def hits(self):
        return np.concatenate([self.cam_hits, self.fu_hits, self.aim_hits])

    def mesh_share(self, hits):
        """The share of the oracle's answers `hits` that carry the mesh's material."""
        return float(np.isin(hits["material"], self.mesh_materials).mean())

    def assert_not_vacuous(self):
        """Conditions on the oracle's answers alone."""
        assert (self.cam_hits["klass"] == SURFACE).mean() >= 0.5
        assert self.mesh_share(self.aim_hits) >= 0.5, f"{self.mesh_share(self.aim_hits):.1%} of the aimed rays hit the mesh"
        assert self.mesh_share(self.hits) >= 0.3
        assert self.seg_occluded.mean() >= 0.1 and (~self.seg_occluded).mean() >= 0.1, f"{self.seg_occluded.mean():.1%} of the segments are occluded"


@functools.lru_cache(maxsize=None)
def ray_sets(case="base"):
    return RaySets(host_scene(case, RAY_ARGS))


@functools.lru_cache(maxsize=None)
def oracle_frame(case="base"):
    hs = host_scene(case, FRAME_ARGS)
    return pyoracle.render(hs.desc, hs.camera, hs.params)[0]


def close(a, b, rel=1e-12, floor=1e-15):
    """The bar of tests/test_gpu_parity.py."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) <= np.maximum(rel * np.abs(b), floor)


def klass_of(hits):
    hit = (hits["flags"] & api.RT_RAY_HIT) != 0
    env = (hits["flags"] & api.RT_RAY_ENVIRONMENT) != 0
    return np.where(hit, np.where(env, ENVIRONMENT, SURFACE), MISS)


def assert_answers_equal_oracle(got, want):
    """f64 api.RtRayHit records against Expected: class, material and front face exactly, t and pos at 1e-12 relative."""
    assert got.dtype == api.RtRayHit and len(got) == len(want)
    np.testing.assert_array_equal(klass_of(got), want["klass"])
    np.testing.assert_array_equal(got["material"], want["material"])
    hit = want["klass"] != MISS
    np.testing.assert_array_equal(((got["flags"] & api.RT_RAY_FRONT_FACE) != 0)[hit], want["front"][hit])
    surf = want["klass"] == SURFACE
    for f in ("t", "pos"):
        ok = close(got[f][surf], want[f][surf])
        assert ok.all(), f"{f}: {int((~ok).sum())} values beyond 1e-12 relative, first at ray {int(np.flatnonzero(surf)[np.argwhere(~ok)[0][0]])}"
    assert (got["t"][want["klass"] == MISS] == np.inf).all()
