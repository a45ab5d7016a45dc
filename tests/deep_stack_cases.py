"""Meshes whose 4-wide tree is as deep as the per-lane LDS traversal stacks allow, and the inputs that fill those stacks
(tests/test_deep_stack_host.py, tests/test_gpu_deep_stack.py; DESIGN.md sections 14, 15 and 20).

k_rq_occluded and k_bake_visibility (mesh_any_hit, 4 B an entry, 256 lanes) and k_pq_closest (mesh_closest, 8 B an entry, 256
lanes up to 32 levels and 128 from 33) size a stack per lane from levels = CompiledScene::max_bvh4_stack + 1 and refuse a scene
above 64 levels.  Both walks push under `sp < levels`: were the bound, the LDS size or the stride wrong, an entry would be
dropped without a fault.  The chains below put the trees at 32, 33, 64 and 65 levels, the segments and points make the walks
use every stack index they can reach, and the answers come from brute force.

The chain: triangle i of n is (-s, 0, 0.25 s), (-s, 0, -0.25 s), (-1.5 s, 0.1 s, 0) with s = r^(i - n/2), self-similar along -x;
in this winding a line along D0 meets the fronts.  The host builder turns it into a comb: every node holds the largest
triangles left in two or three leaves (near the root two leaves and a small node of two more) and last the spine with
everything smaller.  mesh_any_hit descends into the LAST entered child and pushes the earlier
ones, so a line that enters every box (origin 0, direction D0 = (-1, 0.09, 0.2): by self-similarity it enters every box and
hits nothing) holds levels - 2 entries at the bottom of the spine; levels - 2 = the sum of (children - 1) down the spine is the
tree's true worst case, max_bvh4_stack adds one and `levels` one more.

  case  r    n    levels      f32
  L32   1.5  102  32          yes: 1.5^+-53 ~ 1e+-9
  L33   1.5  106  33          yes
  L64   3    124  64          no: 3^+-63 ~ 1e+-30, squares overflow f32
  L65   3    126  65          no; refused by the three kernels
  L33_back = L33 with RT_MESH_HIT_BACK_FACES set on the description (the scene language has no word for it), which turns
  the cone culling of quantise_dir / node4q_cull_cones off.

Segments, per case, all from x = 0 over the explicit interval (0, 4 s_max / c) for a direction c (-1, ., .): they run along -x
past every triangle.  c = 1 but for the keyed lines of small triangles (direction_scale):
  (a) `through`  lines through the origin with directions near D0 that enter every box and hit nothing: restated peak levels - 2;
  (b) `keyed`    lines along D0 through a point inside triangle j: j is the only triangle they cross, and the restated walk
                 pops j's leaf from stack index k.  A line through one of the largest triangles passes under every smaller
                 box and the walk turns round at j's node; further down every box carries the tree's absolute pad (2^-19
                 of the extent), the line enters them all and j's leaf waits under a full stack.  One segment is kept for
                 every k the search reaches;
  (c) `missed`   every keyed line moved along the triangle's first edge until it crosses the plane outside the triangle by
                 2 * margin (barycentric): it hits nothing.
`margin` (1e-6 for f64; tests pass a wider one for f32) bounds every decision: the barycentrics of a hit are inside by at
least margin, those of every miss outside by at least margin (barycentrics are relative to the triangle's own size), t inside
(0, T_HI) by that relative margin.  The back-face variant adds every keyed and missed segment reversed (from beyond triangle j
back towards the origin), which only a mesh that hits back faces answers with "occluded".

The two walks are restated here over api.scene_refit_mesh's export (children, decoded boxes, triangle records) to CHOOSE the
inputs and to say which stack index an answer depends on.  They are never the yardstick: occlusion is judged by the oracle's
primitive tests without its octree (pyoracle.world_hits(unculled=True), the way tests/special_ray_cases.py gets them), points
by closest_points_ref.Reference, the bake by bake_ref's recipe on that occlusion reference."""
import atexit
import functools
import pathlib
import shutil
import tempfile

import numpy as np

import bake_ref
import closest_points_ref as cr
from rust_raytracer_amd import api
from ray_query_cases import SURFACE
from special_ray_cases import unculled_hits
from tree_scale_cases import EMPTY

CHAINS = {"L32": (1.5, 102, 32), "L33": (1.5, 106, 33), "L64": (3.0, 124, 64), "L65": (3.0, 126, 65)}   # r, n, levels
F32_CASES = ("L32", "L33")
D0 = np.array([-1.0, 0.09, 0.2])
MARGIN = 1e-6
N_POINTS = 300          # a partial last workgroup at 256 lanes and at 128
BAKE_SHAPES = [(8, 64), (8, 100)]   # (points, samples): one full pass of a wave, and a second, partial one
BAKE_SEED = 2024
DET_EPS = 2.0 ** -52    # tri_test's absolute threshold on d . (e1 x e2), in both precisions (Lim<R>::det_eps)
DET_CLEAR = 2.0 ** -17  # what a keyed line's determinant is held above: 2^-10 <= |d|^2-free c s^2 < 2^-9 times 0.0275


# ---- the chain ----
def scales(r, n):
    return np.array([float(r) ** (i - n / 2) for i in range(n)])


def chain_triangles(r, n):
    """(n, 3, 3) corners."""
    s = scales(r, n)[:, None]
    return np.stack([s * [-1.0, 0.0, 0.25], s * [-1.0, 0.0, -0.25], s * [-1.5, 0.1, 0.0]], axis=1)


@functools.lru_cache(maxsize=None)
def _tmp():
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="deep_stack_"))
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    return tmp


def chain_obj(path, tri):
    lines = ["vt 0 0", "vn 0 1 0"]
    for t in tri:
        lines += ["v " + " ".join(repr(float(x)) for x in v) for v in t]   # float(): repr of a numpy scalar is no number
    for i in range(len(tri)):
        a = 3 * i + 1
        lines.append(f"f {a}/1/1 {a + 1}/1/1 {a + 2}/1/1")
    path.write_text("\n".join(lines) + "\n")


def new_host_scene(name, width=24, positions_scale=None):
    """A HostScene of its own (nobody else holds it): the chain of case `name`, a sky and an empty light list.  `_back` sets
    RT_MESH_HIT_BACK_FACES, `_lit` puts the sky into the light list (with an empty list the reference's light sampling turns
    every path that meets the chain into a NaN: good for queries, which shade nothing, useless for a frame);
    positions_scale multiplies every vertex after loading (the tree a DeviceScene builds first stays)."""
    chain, _, variant = name.partition("_")
    assert variant in ("", "back", "lit")
    back, lights = variant == "back", "$sky" if variant == "lit" else ""
    r, n, _ = CHAINS[chain]
    tmp = _tmp()
    scene = f"scene_{chain}_lit" if lights else f"scene_{chain}"
    if not (tmp / f"{chain}.obj").exists():
        chain_obj(tmp / f"{chain}.obj", chain_triangles(r, n))
    if not (tmp / scene).exists():
        (tmp / scene).write_text(
            f"@config output_width = 24\n@config aspect_ratio = 1\n@config focal_length = 40\n"
            f"@config camera_pos = -3,6,2\n@config camera_target = -3,0,0\n"   # from above: the triangles of size 0.5 .. 5
            f"chain: mesh {chain}.obj (lambertian (constant 0.7,0.6,0.5))\nsky: sky (constant 0.6,0.7,1)\n"
            f"world: list $chain $sky\nlights: list {lights}\n")
    hs = api.HostScene([str(tmp / scene), f"-w={width}", "-s=4", "--seed=53"])
    m = hs.desc.contents.meshes[0]
    assert hs.desc.contents.n_meshes == 1 and m.n_triangles == n
    if back:
        m.flags |= api.RT_MESH_HIT_BACK_FACES
    if positions_scale is not None:
        np.ctypeslib.as_array(m.positions, shape=(m.n_positions, 3))[:] *= positions_scale
    return hs


@functools.lru_cache(maxsize=None)
def host_scene(name):
    """Shared: nobody writes into it."""
    return new_host_scene(name)


# ---- brute force over the triangles (margins and the choice of inputs; the yardstick is the oracle) ----
def crossings(tri, o, d):
    """Moeller-Trumbore of the line o + t d against every triangle (T, 3, 3) in f64 -> (det, u, v, t); det > 0: the front."""
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    b = o - v0
    u = (b * p).sum(-1) / det
    q = np.cross(b, e1)
    return det, u, (q * d).sum(-1) / det, (e2 * q).sum(-1) / det


def decided(tri, o, d, t_lo, t_hi, margin, back=False):
    """-> (the triangles the segment hits, True iff every decision is clear of `margin`): a hit has u, v, 1 - u - v >= margin,
    t inside the interval by margin * t and a determinant of at least DET_CLEAR; a miss has one of the barycentrics <= -margin,
    or t outside by as much, or a determinant below half the threshold (its back, if the mesh does not hit backs)."""
    det, u, v, t = crossings(tri, o, d)
    dd = np.abs(det) if back else det
    inside = np.minimum(np.minimum(u, v), 1.0 - u - v)
    within = np.minimum(t - t_lo, t_hi - t) / np.abs(t)
    hit = (dd >= DET_CLEAR) & (inside >= margin) & (within >= margin)
    miss = (dd <= 0.5 * DET_EPS) | (inside <= -margin) | (within <= -margin)
    return np.flatnonzero(hit), bool((hit | miss).all())


# ---- the exported tree ----
class Tree:
    def __init__(self, desc):
        t = api.scene_refit_mesh(desc, desc, 0, False)
        self.children, self.order = t["children"], t["order"]
        self.lo, self.hi = t["boxes"][:, :, 0].astype(np.float64), t["boxes"][:, :, 1].astype(np.float64)
        rec = t["tris"]
        self.tri = np.stack([rec[:, 0], rec[:, 0] + rec[:, 1], rec[:, 0] + rec[:, 2]], axis=1)   # corners, in leaf-slot order

    def slots(self, leaf):
        code = ~int(leaf)
        return range(code >> 3, (code >> 3) + (code & 7) + 1)


@functools.lru_cache(maxsize=None)
def tree(name):
    return Tree(host_scene(name).desc)


def any_hit_walk(tr, o, d, t_lo, t_hi, back=False):
    """mesh_any_hit restated: an f64 slab test of the decoded child boxes over (t_lo, t_hi), the last entered child is
    descended into and the earlier ones are pushed in child order, the walk ends at the first triangle hit.  Cones are left
    out: they only skip children whose triangles all show their backs.
    -> (occluded, peak stack size, [(leaf, stack index it was popped from or -1 for a descent)], the leaf slot hit or -1)."""
    inv = 1.0 / d
    stack, peak, visits, node = [], 0, [], 0
    while True:
        at = -1
        if node >= 0:
            t0, t1 = (tr.lo[node] - o) * inv, (tr.hi[node] - o) * inv
            near, far = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
            entered = (tr.children[node] != EMPTY) & (np.maximum(near, t_lo) <= np.minimum(far, t_hi))
            nxt = None
            for k in np.flatnonzero(entered):
                if nxt is not None:
                    stack.append(nxt)
                nxt = int(tr.children[node, k])
            peak = max(peak, len(stack))
            if nxt is not None:
                node = nxt
                if node < 0:
                    visits.append((node, -1))
                continue
        else:
            slots = np.array(tr.slots(node))
            det, u, v, t = crossings(tr.tri[slots], o, d)
            hit = ((np.abs(det) if back else det) >= DET_EPS) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > t_lo) & (t < t_hi)
            if hit.any():
                return True, peak, visits, int(slots[np.flatnonzero(hit)[0]])
        if not stack:
            return False, peak, visits, -1
        node = stack.pop()
        if node < 0:
            visits.append((node, len(stack)))


_EPS = 2.0 ** -52


def _f32_at_most(x):
    """f32_at_most of rt_traverse.h: an f32 that is certainly no larger (2^-20 relative; 0 below 1e-30)."""
    f = np.minimum(np.float32(min(x, 3.0e38)), np.float32(3.402823466e+38))
    return np.float32(0.0) if f < np.float32(1e-30) else np.float32(f - f * np.float32(9.5367431640625e-7))


def _radius2(best):
    return np.inf if best == np.inf else best * best * (1.0 + 8.0 * _EPS) + 1e-300


def nearest_first_walk(tr, q):
    """mesh_closest restated in f64 (no distance limit, chain scale 1): box_dist2_below on the decoded boxes, the bounds below
    the squared search radius rounded down to f32 (f32_at_most), the sorting network RT_SORT4_NEAREST_FIRST with its ties, the
    nearest child continued with and the others pushed farthest first, a popped entry dropped if the radius has overtaken
    its bound, the radius shrunk at every nearer triangle.
    -> (distance, leaf slot of the winner, peak stack size, stack index the winner's leaf was popped from or -1)."""
    best, best_slot, best_at = np.inf, -1, -1
    stack, peak, node, at = [], 0, 0, -1
    while True:
        if node >= 0:
            lo, hi = tr.lo[node], tr.hi[node]
            gap = np.maximum(np.maximum(lo - q, q - hi), 0.0) - 2.0 * _EPS * (np.abs(q) + np.maximum(np.abs(lo), np.abs(hi)))
            gap = np.maximum(gap, 0.0)
            lb = (gap * gap).sum(axis=1) * (1.0 - 4.0 * _EPS)
            r2 = _radius2(best)
            ch = [int(c) for c in tr.children[node]]
            key = [_f32_at_most(lb[k]) if (ch[k] != EMPTY and lb[k] < r2) else np.float32(np.inf) for k in range(4)]
            for i, j in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
                if key[i] > key[j]:
                    key[i], key[j], ch[i], ch[j] = key[j], key[i], ch[j], ch[i]
            for k in (3, 2, 1):
                if key[k] < np.inf:
                    stack.append((ch[k], float(key[k])))
            peak = max(peak, len(stack))
            if key[0] < np.inf:
                node = ch[0]
                at = -1 if node < 0 else at
                continue
        else:
            slots = np.array(tr.slots(node))
            dist, _ = cr.closest_on_triangles(tr.tri[slots], q)
            k = int(np.argmin(dist))
            if dist[k] < best:
                best, best_slot, best_at = float(dist[k]), int(slots[k]), at
        r2 = _radius2(best)
        while True:
            if not stack:
                return best, best_slot, peak, best_at
            node, bound = stack.pop()
            if bound < r2:
                at = len(stack)
                break


# ---- segments ----
class Segments:
    """o, d (n, 3), t_lo, t_hi (n,), kind (n,) of 'through' / 'keyed' / 'missed', key (n,): the stack index the answer depends
    on (keyed and missed; -1 otherwise), target (n,): the triangle (the mesh's own index) crossed or just missed, occluded (n,):
    the oracle's answer, peak (n,): the restated walk's."""

    def __init__(self, name, rows):
        self.name = name
        self.o = np.ascontiguousarray([r[0] for r in rows], dtype=np.float64)
        self.d = np.ascontiguousarray([r[1] for r in rows], dtype=np.float64)
        self.t_lo = np.array([r[2] for r in rows])
        self.t_hi = np.array([r[3] for r in rows])
        self.kind = np.array([r[4] for r in rows])
        self.key = np.array([r[5] for r in rows])
        self.target = np.array([r[6] for r in rows])
        self.peak = np.array([r[7] for r in rows])
        self.restated = np.array([r[8] for r in rows])
        self.occluded = unculled_hits(host_scene(name).desc, self.o, self.d, self.t_lo, self.t_hi)["klass"] == SURFACE

    def __len__(self):
        return len(self.o)


def reach(name):
    """How far along -x a segment must run to pass every triangle: 4 s_max."""
    r, n, _ = CHAINS[name.partition("_")[0]]
    return 4.0 * float(scales(r, n)[-1])


def _through_directions():
    return [np.array([-1.0, 0.09 + a, 0.2 + b]) for a in (0.0, 0.004, 0.008, -0.004, 0.012) for b in (0.0, 0.01, -0.01, 0.02, -0.02)]


# where in triangle j a keyed line crosses: a = how far from the base edge towards the apex, w = how far from the axis towards
# the side, as a share of the half width there
_TARGETS = [(a, w) for a in (0.3, 0.1, 0.5, 0.7, 0.8, 0.9, 0.95) for w in (0.0, 0.5, -0.5, 0.8, -0.8)]


def direction_scale(s):
    """The power of two c >= 1 with c s^2 >= 2^-10: tri_test's determinant rule is absolute, d . (e1 x e2) = 0.0275 c s^2 for a
    direction c D0, so a triangle below s ~ 1e-7 is invisible to a direction of unit size whatever the line."""
    return max(1.0, 2.0 ** np.ceil(np.log2(2.0 ** -10 / (s * s))))


@functools.lru_cache(maxsize=None)
def segments(name, margin=MARGIN):
    chain, _, variant = name.partition("_")
    back = variant == "back"
    r, n, levels = CHAINS[chain]
    tr = tree(name)
    tri = chain_triangles(r, n)
    s = scales(r, n)
    far = reach(name)
    rows = []
    for d in _through_directions():
        o = np.zeros(3)
        hits, clear = decided(tri, o, d, 0.0, far, max(margin, 1e-3), back)
        flag, peak, _, _ = any_hit_walk(tr, o, d, 0.0, far, back)
        if clear and len(hits) == 0 and peak == levels - 2:
            rows.append((o, d, 0.0, far, "through", -1, -1, peak, flag))
    slot_of = np.argsort(tr.order)   # the mesh's own triangle -> leaf slot
    found = {}
    for a, w in _TARGETS:
        if len(found) == levels - 2:
            break
        for j in range(n):
            v0, v1, v2 = tri[j]
            mid = 0.5 * (v0 + v1)
            p = mid + a * (v2 - mid) + w * (1.0 - a) * 0.5 * (v1 - v0)
            o = p + D0 * p[0]    # back along D0 to x = 0
            c = direction_scale(s[j])
            d, t_hi = D0 * c, far / c
            hits, clear = decided(tri, o, d, 0.0, t_hi, margin, back)
            if not clear or list(hits) != [j]:
                continue
            flag, peak, visits, slot = any_hit_walk(tr, o, d, 0.0, t_hi, back)
            if slot != slot_of[j] or not visits or visits[-1][1] < 0 or slot not in tr.slots(visits[-1][0]):
                continue
            k = visits[-1][1]
            if k in found:
                continue
            # the near miss: along the first edge to u = -2 margin
            _, u, _, _ = crossings(tri[j:j + 1], o, d)
            o_miss = o - (u[0] + 2.0 * margin) * (v1 - v0)
            hits_m, clear_m = decided(tri, o_miss, d, 0.0, t_hi, margin, back)
            if not clear_m or len(hits_m):
                continue
            flag_m, peak_m, _, _ = any_hit_walk(tr, o_miss, d, 0.0, t_hi, back)
            found[k] = [(o, d, 0.0, t_hi, "keyed", k, j, peak, flag), (o_miss, d, 0.0, t_hi, "missed", k, j, peak_m, flag_m)]
    for k in sorted(found):
        rows += found[k]
    if back:
        # the same lines the other way, from four times as far as the plane of triangle j back through it and past the origin:
        # the triangles' backs.  (From the far end of the chain the barycentrics of a small triangle are lost in the rounding of
        # the origin, in the oracle's arithmetic as in the kernel's.)  `key` is what the restated walk says of THIS segment.
        for o, d, _, _, kind, _, j, _, _ in [r for r in rows if r[4] != "through"]:
            t_j = float(crossings(tri[j:j + 1], o, d)[3][0])
            start, hi = o + 4.0 * t_j * d, 8.0 * t_j
            hits, clear = decided(tri, start, -d, 0.0, hi, margin, True)
            if not clear or list(hits) != ([j] if kind == "keyed" else []):
                continue
            flag, peak, visits, _ = any_hit_walk(tr, start, -d, 0.0, hi, True)
            rows.append((start, -d, 0.0, hi, kind + "_back", visits[-1][1] if flag and visits else -1, j, peak, flag))
    return Segments(name, rows)


def covered(keys, top):
    """The share of the indices 0 .. top that occur in `keys`, and the missing ones."""
    have = set(int(k) for k in keys)
    missing = [k for k in range(top + 1) if k not in have]
    return 1.0 - len(missing) / (top + 1), missing


# ---- points ----
class Points:
    """q (N_POINTS, 3), peak and key per point from the restated nearest-first walk (key: the stack index the winner's leaf was
    popped from, -1 for a descent), restated: the walk's distance."""

    def __init__(self, name, q, peak, key, restated):
        self.name, self.q = name, np.ascontiguousarray(q)
        self.peak, self.key, self.restated = np.array(peak), np.array(key), np.array(restated)


_OFFSETS = [np.array(v, dtype=np.float64) for v in ((0, 1, 0), (1, 0, 0), (1, 1, 0), (1, -1, 0), (0, 1, 1), (-1, -1, 1))]


@functools.lru_cache(maxsize=None)
def points(name):
    """N_POINTS points of a case, in this order: (1) keyed points, one for every stack index the search reaches; (2) points
    with the largest peak the search finds (at least 8); (3) the rest of the candidates in the order they were tried.
    Candidates (numpy.random.default_rng(7)): the centroid of every triangle j moved by 1 and by 3 s_j along six directions
    (the moves that reach the most indices: the point then lies beside the chain, level with triangles some nodes up or down
    the spine), points of the size of the largest triangles around the whole chain, and points inside the smallest boxes."""
    r, n, _ = CHAINS[name]
    tr, tri, s = tree(name), chain_triangles(r, n), scales(r, n)
    rng = np.random.default_rng(7)
    cand = [rng.normal(size=3) * s[0] * 10.0 ** rng.uniform(-2, 1) for _ in range(24)]
    cand += [tri[j].mean(axis=0) + v * s[j] * m for j in range(n - 1, -1, -1) for m in (3.0, 1.0) for v in _OFFSETS]
    cand += [np.array([rng.uniform(-1.0, 0.4), rng.uniform(-1.5, 3.2), rng.uniform(-1.4, 1.4)]) * s[-1] * 10.0 ** rng.uniform(-1.5, 0.3)
             for _ in range(600)]
    walked = [nearest_first_walk(tr, q) for q in cand]
    top = max(w[2] for w in walked)
    first_of = {}
    for i, w in enumerate(walked):
        if w[3] >= 0:
            first_of.setdefault(w[3], i)
    pick = [first_of[k] for k in sorted(first_of)]
    pick += [i for i, w in enumerate(walked) if w[2] == top and i not in pick][:16]
    pick += [i for i in range(len(cand)) if i not in set(pick)][:N_POINTS - len(pick)]
    assert len(pick) == N_POINTS
    return Points(name, np.array([cand[i] for i in pick]), [walked[i][2] for i in pick], [walked[i][3] for i in pick],
                  [walked[i][0] for i in pick])


# ---- the bake ----
class BakeGroup:
    """Points on one triangle: positions, normals, the call's bias and max_distance (from the triangle's scale), and per shape
    of BAKE_SHAPES the reference's (samples, count, visibility, bent)."""

    def __init__(self, desc, s, pos, nrm):
        self.s, self.pos, self.nrm = s, np.ascontiguousarray(pos), np.ascontiguousarray(nrm)
        self.bias, self.max_distance = 2.0 ** -10 * s, 64.0 * s
        self.shapes = []
        for _, samples in BAKE_SHAPES:
            d = np.array([[bake_ref.direction(BAKE_SEED, i, k, self.nrm[i]) for k in range(samples)] for i in range(len(pos))])
            o = np.repeat(self.pos, samples, axis=0)
            hit = unculled_hits(desc, o, d.reshape(-1, 3), self.bias, self.max_distance)["klass"] == SURFACE
            free = ~hit.reshape(len(pos), samples)
            count = free.sum(axis=1)
            bent = (d * free[..., None]).sum(axis=1) / float(samples)
            self.shapes.append((samples, count, count / float(samples), bent))


@functools.lru_cache(maxsize=None)
def bake_groups(name):
    """8 points on the chain's triangles at three scales - 3 on the second largest triangle, 3 on the middle one, 2 on the
    smallest - each group baked by a call of its own (bias and max_distance are per call).  The normals look along the chain,
    (-1, 0.3, 0.1) towards the larger triangles and (1, 0.3, -0.1) towards the smaller ones, so that a good part of every
    hemisphere is covered by them.  At the smallest scale nothing occludes a direction of unit length (tri_test's absolute
    determinant rule, see direction_scale): those two points are fully visible in the reference, and their walks still
    enter every small box."""
    r, n, _ = CHAINS[name]
    tri, s, desc = chain_triangles(r, n), scales(r, n), host_scene(name).desc
    weights = np.array([[0.05, 0.05, 0.9], [0.1, 0.2, 0.7], [0.2, 0.1, 0.7]])
    normals = np.array([[-1.0, -0.2, 0.1], [-1.0, 0.0, -0.1], [-1.0, -0.1, 0.0]])
    return [BakeGroup(desc, s[j], weights[:k] @ tri[j], normals[:k]) for j, k in ((n - 2, 3), (n // 2, 3), (0, 2))]
