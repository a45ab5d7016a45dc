"""Generated scenes that put the re-built primitive groups (OP_GROUP, group_search in csrc/rt_wavefront.h) at their limits and
offsets, with ray sets judged by the oracle (tests/test_group_cases_host.py, tests/test_gpu_groups.py).

Every other scene of the suite that reaches k_wf_prims<GROUPS> has ONE bare group of 15 to 455 primitives that needs at most 14
stack levels: every base of try_emit_group (node root, primitive base, guard base, rank base) is zero there, the ray that
group_search is given is the world ray, and neither limit of plan_wavefront (16 stack levels, 24 KB = 384 nodes) is near.

Scenes (written into a temporary directory; numbers with repr, so the files hold the generator's bits; a lamp quad and a sky
in each, so that frames are lit):
  two_groups          A: 40 spheres in a `bvh xyz`; B: a `bvh xz` of 30 spheres, a hollow glass ball (a list of the outer sphere and
                      an inner one with NEGATIVE radius: inverted box, reachable through the list's box), one sphere with
                      negative radius alone in a bvh of its own (unreachable in the reference: that node's box is inverted;
                      the compiler drops it, and the inverted box stays in the unions of the reference's ancestors, which
                      become guards of the primitives beside it) and a list of two quads, one of them `backface`.  Two exactly coincident spheres with different materials: dupa in A, dupb in B.
  two_groups_swapped  the same with B before A in `world`: the tie goes to the other group.
  instanced           one 30-sphere bvh under two transforms (one with a non-uniform scale) beside a bare 40-sphere group: three
                      groups, two of them over the same sphere records.
  stack16, stack_over the geometric chain along x with ratio 3: the shortest chain whose group needs exactly 16 stack levels, and
                      the shortest that needs 17 or more.
  chain15_16          the chain with ratio 1.5, long enough to need 16 levels (a narrower range of scales).
  lattice900, lattice1000   900 / 1000 uniformly random spheres in one `bvh xyz`: under / over the stack limit.
  nodes_at_limit, nodes_over   the regular grid 16 x 8 x 12 (r = 0.2, step 0.5) and a second group of random spheres: 380..384 and
                      385..400 nodes in all, <= 16 levels in both, so that the node limit alone decides.
  ground              a radius-1000 sphere centred at y = -1000 in one bvh with 60 spheres of radius 0.2 resting on it.
  far                 group A of two_groups with every centre moved by (4096, 0, -4096).

Ray sets per scene:
  target   K = 4 rays per sphere instance: origin c + 1.25 |r| u, direction -u * uniform(0.5, 2), u a random unit vector (the
           four are the corners of a randomly rotated tetrahedron; origin and direction are taken through the instance's
           transform); per quad two rays at its centre, one from each side;
  grazing  (scenes with fewer than 200 primitives) two per sphere instance, from 50 radii away, passing the centre at distance
           r (1 -+ 1e-7): along the faces and corners of the boxes above the sphere;
  camera rays, follow-ups and segments of ray_query_cases.Cases at -w=24.
The yardstick is pyoracle.world_hits (the world built once per call)."""
import atexit
import functools
import pathlib
import shutil
import tempfile

import numpy as np

from oracle import pyoracle
from rust_raytracer_amd import api
from ray_query_cases import SURFACE, T_MAX, T_MIN, Cases, leaf_nodes
from special_ray_cases import EDGE_SHARE, expected

K_TARGET = 4
GRAZE = 1e-7
FAR_OFFSET = (4096.0, 0.0, -4096.0)
MATERIALS = ("m0: lambertian (constant 0.7,0.7,0.7)\nm1: metal (constant 0.8,0.8,0.9) (constant 0.1)\n"
             "m2: glossy (constant 0.8,0.2,0.2) (constant 0.1)\nm3: lambertian (constant 0.2,0.7,0.3)\nm4: glass\n")
NAMES = ("two_groups", "two_groups_swapped", "instanced", "stack16", "stack_over", "chain15_16", "lattice900", "lattice1000",
         "nodes_at_limit", "nodes_over", "ground", "far")
GROUP_FORM = ("two_groups", "two_groups_swapped", "instanced", "stack16", "chain15_16", "lattice900", "nodes_at_limit", "ground", "far")
OP_FORM = ("stack_over", "lattice1000", "nodes_over")   # over a limit of plan_wavefront: the scene keeps the op form

# chain lengths and the size of the second group of nodes_*: what the generators need to sit where the names say; asserted by
# tests/test_group_cases_host.py on the compiler's own figures
CHAIN3_AT, CHAIN3_OVER, CHAIN15_AT = 24, 25, 27
SECOND_AT, SECOND_OVER = 138, 140
LATTICE_SEED = 101   # 900 random spheres need 17 levels under most seeds and 16 under a few


def _v(x):
    return ",".join(repr(float(c)) for c in x)


def _sphere(name, c, r, mat):
    return f"{name}: sphere {_v(c)} {float(r)!r} $m{mat}\n"


def _config(pos, target, focal=35):
    return (f"@config output_width = 32\n@config aspect_ratio = 1\n@config focal_length = {focal}\n"
            f"@config camera_pos = {_v(pos)}\n@config camera_target = {_v(target)}\n")


def _tail(world, lamp_centre, lamp_half):
    h = float(lamp_half)
    return (f"lamp: plane {_v(lamp_centre)} {_v((h, 0, 0))} {_v((0, 0, h))} (emissive (constant 8,8,8)) backface\n"
            "sky: sky (constant 0.3,0.4,0.6)\n"
            f"world: list {world} $lamp $sky\nlights: list $lamp\n")


def _random_spheres(rng, n, lo, hi, r_lo, r_hi, prefix, offset=(0.0, 0.0, 0.0)):
    """(text, names) of n spheres with centres uniform in [lo, hi] and radii uniform in [r_lo, r_hi]."""
    text, names = "", []
    for i in range(n):
        c = rng.uniform(lo, hi) + np.array(offset)
        text += _sphere(f"{prefix}{i}", c, rng.uniform(r_lo, r_hi), i % 4)
        names.append(f"${prefix}{i}")
    return text, names


def _group_a(offset=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(101)
    text, names = _random_spheres(rng, 39, (-6.0, 0.3, -2.0), (-1.5, 2.5, 2.0), 0.15, 0.4, "a", offset)
    c = np.array([0.0, 1.5, 0.0]) + np.array(offset)
    text += _sphere("dupa", c, 0.5, 0)
    return text + f"ga: bvh xyz {' '.join(names)} $dupa\n"


def _group_b():
    rng = np.random.default_rng(102)
    text, names = _random_spheres(rng, 29, (1.5, 0.3, -2.0), (6.0, 2.5, 2.0), 0.15, 0.4, "b")
    text += _sphere("dupb", (0.0, 1.5, 0.0), 0.5, 1)
    # a hollow glass ball: the inner surface has a negative radius, its box is inverted; inside a list it can be reached
    text += _sphere("shell", (3.5, 3.2, 0.5), 0.5, 4) + _sphere("hollow", (3.5, 3.2, 0.5), -0.375, 4) + "ball: list $shell $hollow\n"
    # one alone in a bvh of its own: that node has the inverted box, no ray passes it, and the compiler drops the sphere
    text += _sphere("lost", (5.0, 3.0, -1.0), -0.25, 2) + "lostbox: bvh x $lost\n"
    text += ("qa: plane 2.5,1.0,2.5 0.5,0,0 0,0.5,0 $m3 backface\nqb: plane 4.5,1.25,-2.5 0,0.5,0 0.25,0,0.5 $m1\n"
             "quads: list $qa $qb\n")
    return text + f"gb: bvh xz {' '.join(names)} $dupb $ball $lostbox $quads\n"


def _chain(ratio, n):
    """Sphere i has radius ratio^i / 8 and touches sphere i - 1 along x.  A tree over it can only peel one sphere at a time."""
    text, names, x, r = "", [], 0.0, 0.125
    for i in range(n):
        text += _sphere(f"c{i}", (x, 0.0, 0.0), r, i % 4)
        names.append(f"$c{i}")
        x += r + r * ratio
        r *= ratio
    return text + f"chain: bvh x {' '.join(names)}\n", x, r


def _grid():
    text, names = "", []
    for i in range(16):
        for j in range(8):
            for k in range(12):
                text += _sphere(f"g{i}_{j}_{k}", (0.5 * i - 3.75, 0.5 * j + 0.25, 0.5 * k - 2.75), 0.2, (i + j + k) % 4)
                names.append(f"$g{i}_{j}_{k}")
    return text + f"grid: bvh xyz {' '.join(names)}\n"


def scene_text(name):
    if name in ("two_groups", "two_groups_swapped"):
        world = "$ga $gb" if name == "two_groups" else "$gb $ga"
        return _config((0, 3, 12), (0, 1.5, 0)) + MATERIALS + _group_a() + _group_b() + _tail(world, (0, 6, 0), 2)
    if name == "far":
        off = np.array(FAR_OFFSET)
        return (_config(off + (-3.5, 3, 10), off + (-3.5, 1.5, 0)) + MATERIALS + _group_a(FAR_OFFSET)
                + _tail("$ga", off + (-3, 6, 0), 2))
    if name == "instanced":
        rng = np.random.default_rng(103)
        base, bn = _random_spheres(rng, 30, (-1.5, -1.0, -1.5), (1.5, 1.0, 1.5), 0.15, 0.35, "i")
        bare, en = _random_spheres(rng, 40, (-2.0, 2.5, -2.0), (2.0, 4.5, 2.0), 0.15, 0.35, "e")
        return (_config((0, 3, 14), (0, 1.5, 0)) + MATERIALS + base + f"base: bvh xyz {' '.join(bn)}\n"
                "ta: transform $base t=3,1,-2 ry=30 s=1.5,0.75,1\ntb: transform $base t=-4,0.5,1 rz=20\n"
                + bare + f"bare: bvh xyz {' '.join(en)}\n" + _tail("$ta $tb $bare", (0, 7, 0), 2))
    if name in ("stack16", "stack_over", "chain15_16"):
        ratio, n = {"stack16": (3.0, CHAIN3_AT), "stack_over": (3.0, CHAIN3_OVER), "chain15_16": (1.5, CHAIN15_AT)}[name]
        text, x, r = _chain(ratio, n)
        # the camera looks along the chain's flank from beyond its large end; the lamp hangs above the large end
        return (_config((0.6 * x, 0.8 * r, 2.5 * r), (0.3 * x, 0, 0)) + MATERIALS + text
                + _tail("$chain", (0.8 * x, 3.0 * r, 0), 0.5 * r))
    if name in ("lattice900", "lattice1000"):
        rng = np.random.default_rng(LATTICE_SEED)
        text, names = _random_spheres(rng, 900 if name == "lattice900" else 1000, (-5.0, 0.2, -5.0), (5.0, 6.0, 5.0), 0.1, 0.3, "s")
        return (_config((0, 4, 16), (0, 3, 0)) + MATERIALS + text + f"field: bvh xyz {' '.join(names)}\n"
                + _tail("$field", (0, 9, 0), 3))
    if name in ("nodes_at_limit", "nodes_over"):
        rng = np.random.default_rng(105)
        n2 = SECOND_AT if name == "nodes_at_limit" else SECOND_OVER
        text, names = _random_spheres(rng, n2, (-4.0, 4.6, -3.0), (4.0, 6.5, 3.0), 0.12, 0.3, "r")
        return (_config((0, 4, 15), (0, 3, 0)) + MATERIALS + _grid() + text + f"second: bvh xyz {' '.join(names)}\n"
                + _tail("$grid $second", (0, 9, 0), 3))
    if name == "ground":
        rng = np.random.default_rng(106)
        text = _sphere("earth", (0.0, -1000.0, 0.0), 1000.0, 3)
        names = ["$earth"]
        placed = []
        while len(placed) < 60:                                     # apart from each other: every one can be seen from all round
            x, z = rng.uniform(-6.0, 6.0, size=2)
            if all((x - a) ** 2 + (z - b) ** 2 >= 0.7 ** 2 for a, b in placed):
                placed.append((x, z))
        for i, (x, z) in enumerate(placed):
            y = np.sqrt(1000.2 ** 2 - x * x - z * z) - 1000.0      # resting on the big sphere
            text += _sphere(f"p{i}", (x, y, z), 0.2, i % 3)
            names.append(f"$p{i}")
        return (_config((0, 3, 13), (0, 0.2, 0)) + MATERIALS + text + f"field: bvh xyz {' '.join(names)}\n"
                + _tail("$field", (0, 8, 0), 2))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _tmp():
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="group_cases_"))
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    return tmp


@functools.lru_cache(maxsize=None)
def scene_path(name):
    path = _tmp() / f"scene_{name}"
    path.write_text(scene_text(name))
    return str(path)


@functools.lru_cache(maxsize=None)
def host_scene(name):
    """The scene at the settings of ray_query_cases (the ray sets)."""
    return api.HostScene([scene_path(name), "-w=24", "-s=1", "--seed=31"])


@functools.lru_cache(maxsize=None)
def frame_scene(name):
    """The scene at 32 x 32, 4 samples per pixel (the frames)."""
    return api.HostScene([scene_path(name), "-w=32", "-s=4", "--seed=7"])


@functools.lru_cache(maxsize=None)
def program(name):
    """(ops, info) of api.scene_program."""
    return api.scene_program(host_scene(name).desc)


# ---- the primitives, per path that reaches them ----
class Instance:
    """One (leaf node, path to it) of a sphere or quad."""

    def __init__(self, node, kind, m, p, material):
        self.node, self.kind, self.m, self.p, self.material = node, kind, m, np.array(p), material
        self.inv = np.linalg.inv(m)
        self.stretch = float(np.linalg.svd(m[:3, :3], compute_uv=False).max())

    def to_world(self, pts, w=1.0):
        pts = np.atleast_2d(pts)
        return pts @ self.m[:3, :3].T + w * self.m[:3, 3]

    def distance(self, pts):
        """Distance (a length in world space, an upper bound under a non-uniform scale) of world points from the surface."""
        q = np.atleast_2d(pts) @ self.inv[:3, :3].T + self.inv[:3, 3]
        if self.kind == api.RT_NODE_SPHERE:
            return np.abs(np.linalg.norm(q - self.p[:3], axis=1) - abs(self.p[3])) * self.stretch
        c, hu, hv = self.p[0:3], self.p[3:6], self.p[6:9]
        n = np.cross(hu, hv)
        n /= np.linalg.norm(n)
        q = q - c
        a, b = q @ hu / hu.dot(hu), q @ hv / hv.dot(hv)
        out = np.maximum(np.abs(a) - 1.0, 0.0) * np.linalg.norm(hu) + np.maximum(np.abs(b) - 1.0, 0.0) * np.linalg.norm(hv)
        return (np.abs(q @ n) + out) * self.stretch


def instances(desc):
    d = desc.contents
    out = []
    for n, mats in leaf_nodes(desc).items():
        node = d.nodes[n]
        if node.type in (api.RT_NODE_SPHERE, api.RT_NODE_PLANE):
            out += [Instance(n, node.type, m, list(node.p), node.material) for m in mats]
    return out


def _unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


TETRAHEDRON = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)


def _target_directions(rng):
    """K_TARGET unit vectors, each uniformly distributed: the corners of a tetrahedron under a random rotation.  No half space
    holds them all, so a sphere that rests on another (scene `ground`) is aimed at from its free side at least once."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return TETRAHEDRON @ (q * np.sign(np.diag(r))).T


def _perpendicular(u):
    axis = np.eye(3)[np.argmin(np.abs(u), axis=1)]
    w = np.cross(u, axis)
    return w / np.linalg.norm(w, axis=1)[:, None]


class Case:
    """A scene, its ray sets and the oracle's answers, computed once."""

    def __init__(self, name):
        self.name, self.hs = name, host_scene(name)
        self.desc = self.hs.desc
        self.inst = instances(self.desc)
        self.n_prims = len(self.inst) - 1                     # all but the lamp
        rng = np.random.default_rng(17)
        o, d, label, target = [], [], [], []
        for k, e in enumerate(self.inst):
            if e.kind == api.RT_NODE_SPHERE:
                c, r = e.p[:3], abs(e.p[3])
                u = _target_directions(rng)
                o.append(e.to_world(c + 1.25 * r * u))
                d.append(e.to_world(-u * rng.uniform(0.5, 2.0, size=(K_TARGET, 1)), 0.0))
                label += ["t"] * K_TARGET
                target += [k] * K_TARGET
            else:
                c, hu, hv = e.p[0:3], e.p[3:6], e.p[6:9]
                n = np.cross(hu, hv)
                n *= 1.25 * np.linalg.norm(hu) / np.linalg.norm(n)
                o.append(e.to_world(np.array([c + n, c - n])))
                d.append(e.to_world(np.array([-n, n]) * rng.uniform(0.5, 2.0, size=(2, 1)), 0.0))
                label += ["t", "t"]
                target += [k, k]
        if self.n_prims < 200:
            for k, e in enumerate(self.inst):
                if e.kind != api.RT_NODE_SPHERE:
                    continue
                c, r = e.p[:3], abs(e.p[3])
                u = _unit_vectors(rng, 2)
                w = _perpendicular(u)
                off = r * np.array([[1.0 - GRAZE], [1.0 + GRAZE]])
                o.append(e.to_world(c + off * w - 50.0 * r * u))
                d.append(e.to_world(u * rng.uniform(0.5, 2.0, size=(2, 1)), 0.0))
                label += ["g", "g"]
                target += [k, k]
        self.cases = Cases(self.hs)
        o += [self.cases.cam_o, self.cases.fu_o]
        d += [self.cases.cam_d, self.cases.fu_d]
        label += ["c"] * len(self.cases.cam_o) + ["f"] * len(self.cases.fu_o)
        target += [-1] * (len(self.cases.cam_o) + len(self.cases.fu_o))
        self.o, self.d = np.ascontiguousarray(np.concatenate(o)), np.ascontiguousarray(np.concatenate(d))
        self.label, self.target = np.array(label), np.array(target)
        out, self.near = pyoracle.world_hits(self.desc, self.o, self.d, T_MIN, np.inf)
        self.want = expected(out, self.near)
        surf = self.want["klass"] == SURFACE
        self.extent = max(1.0, float(np.abs(self.want["pos"][surf]).max()))
        # on target: the oracle's hit lies on the surface the ray was aimed at, with that primitive's material
        self.on_target = np.zeros(len(self.o), dtype=bool)
        for k, e in enumerate(self.inst):
            sel = np.flatnonzero((self.target == k) & surf)
            if len(sel):
                self.on_target[sel] = (self.want["material"][sel] == e.material) & (e.distance(self.want["pos"][sel]) <= 1e-9 * self.extent)

        # segments: those of Cases over (T_MIN, T_MAX), and the target rays that are on target (thinned to 300) over (T_MIN, 0.5 t)
        # and (T_MIN, 1.5 t) of the oracle's t
        hit = np.flatnonzero(self.on_target & (self.label == "t"))
        hit = hit[::max(1, -(-len(hit) // 300))]
        self.seg_o = np.ascontiguousarray(np.concatenate([self.cases.seg_o, self.o[hit], self.o[hit]]))
        self.seg_d = np.ascontiguousarray(np.concatenate([self.cases.seg_d, self.d[hit], self.d[hit]]))
        self.seg_hi = np.concatenate([np.full(len(self.cases.seg_o), T_MAX), 0.5 * self.want["t"][hit], 1.5 * self.want["t"][hit]])
        out, _ = pyoracle.world_hits(self.desc, self.seg_o, self.seg_d, T_MIN, self.seg_hi)
        self.seg_occluded = out[:, 10] >= 0
        assert (self.seg_occluded[:len(self.cases.seg_o)] == self.cases.seg_occluded).all()   # one oracle, two entry points

    def of(self, label):
        return self.label == label

    def tol(self):
        return 1e-9 * self.extent

    def surface_distance(self, nodes, pos):
        """Per hit: the distance of pos from the nearest instance of node nodes[i]."""
        by_node = {}
        for e in self.inst:
            by_node.setdefault(e.node, []).append(e)
        out = np.full(len(nodes), np.inf)
        for n in np.unique(nodes):
            sel = np.flatnonzero(nodes == n)
            for e in by_node.get(int(n), []):
                out[sel] = np.minimum(out[sel], e.distance(pos[sel]))
        return out


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---- f32 ----
@functools.lru_cache(maxsize=None)
def f32_set(name, n_rays=240, n_segments=120):
    """A seeded sample of the scene's rays and segments as an f32_ray_bounds.RaySet (the rule walks every primitive per ray)."""
    import f32_ray_bounds as fb
    c = case(name)
    if c.n_prims >= 500:
        n_rays, n_segments = n_rays // 2, n_segments // 2
    rng = np.random.default_rng(23)
    # What an f32 set can hold, decided on the rays alone:
    #  * range: sphere_test squares d . (o - c), so |d| times the scene's extent has to stay below 2^60 (the camera rays and the
    #    segments between hit points of the ratio-3 chains have |d| ~ 1e11 at coordinates ~ 1e11: 1e44 is no f32);
    #  * a grazing ray passes its sphere at 1e-7 r, less than rounding its origin to f32 moves it (u L): to f32 it is a tangent.
    #    Where the oracle hits, its normal is that of a point f32 cannot place (sphere normal ratios 10 090 on `instanced` and
    #    7 286 on `ground` against K_DIR = 4096); where it misses, the f32 kernels return the tangent point with the face the
    #    reference's rule gives an exact tangent (dot = 0: not front), the answer to the tangent ray and to none of the rule's
    #    eight copies (`two_groups`: surface, material 1, back face against the sky).  The rule has no notion of a tangent, as
    #    it has none of a tie: grazing rays are left to f64;
    #  * a follow-up starts ON a surface, where t_min = 0.001 is all that keeps it from hitting that surface again (on the
    #    radius-1000 sphere, on the chains' large spheres and 4096 units out, 8 u L is as much): follow-ups may flip, like the
    #    rays on edges and rims of special_ray_cases.f32_set, and take the same share of the sample.
    # f64 holds every ray.
    in_range = np.linalg.norm(c.d, axis=1) * np.maximum(np.abs(c.o).max(axis=1), c.extent) < 2.0 ** 60
    edge = c.label == "f"
    graze, rest = np.flatnonzero(edge & in_range), np.flatnonzero(in_range & (c.label != "g") & (c.label != "f"))
    n_graze = min(len(graze), int(round(EDGE_SHARE * n_rays)))
    sel = np.sort(np.concatenate([rng.choice(graze, size=n_graze, replace=False),
                                  rng.choice(rest, size=min(n_rays - n_graze, len(rest)), replace=False)]))
    # the segments of Cases join two points ON surfaces: the same share; the rest are the target rays' own
    seg_ok = np.linalg.norm(c.seg_d, axis=1) * np.maximum(np.abs(c.seg_o).max(axis=1), c.extent) < 2.0 ** 60
    n_on = len(c.cases.seg_o)
    on, own = np.flatnonzero(seg_ok[:n_on]), n_on + np.flatnonzero(seg_ok[n_on:])
    n_edge = min(len(on), int(round(EDGE_SHARE * n_segments)))
    seg = np.sort(np.concatenate([rng.choice(on, size=n_edge, replace=False),
                                  rng.choice(own, size=min(n_segments - n_edge, len(own)), replace=False)]))
    return fb.RaySet(name, c.hs, fb.Geometry(c.desc), c.o[sel], c.d[sel], c.want[sel], c.seg_o[seg], c.seg_d[seg], c.seg_occluded[seg],
                     c.extent, T_MIN, c.seg_hi[seg])


def fast_oracle(desc, o, d, t_min=T_MIN, t_max=float("inf")):
    """pyoracle.world_hits in the shape f32_ray_bounds wants of an oracle call."""
    return expected(*pyoracle.world_hits(desc, o, d, t_min, t_max))


@functools.lru_cache(maxsize=None)
def fragile_shares(name):
    """(closest-hit share, segment share) of f32_set(name) that the f32 rule could excuse at all: rays with a copy that the oracle
    answers differently."""
    import f32_ray_bounds as fb
    rs = f32_set(name)
    return (fb.fragile_share_closest(rs.geom, rs.o, rs.d, rs.hits, rs.extent, oracle=fast_oracle),
            fb.fragile_share_segments(rs.geom, rs.seg_o, rs.seg_d, rs.seg_occluded, rs.seg_lo, rs.seg_hi, rs.seg_hi / T_MAX, oracle=fast_oracle))
