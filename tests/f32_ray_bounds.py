"""A per-ray yardstick for f32 ray-query answers (tests/test_f32_ray_bounds_host.py, tests/test_gpu_f32_rays.py).

An f32 answer is modelled as the EXACT answer to a slightly moved problem; no ray is discarded.  With u = 2^-24 and, per ray,
L = the largest magnitude among the origin's coordinates, the oracle hit position's coordinates and the world-space numbers
that define the primitive the oracle hit (triangle vertices, sphere centre +- radius, quad corners; for a miss or an environment
hit: the origin and the ray set's extent), every ray has eight copies at delta = 8 u L: the origin moved +-delta along two unit
vectors perpendicular to the direction, and the direction tilted so that the point at the oracle's t (a segment's end point;
for a miss the point at the extent) moves +-delta along the same two vectors.  8 is derived: rounding o and d to f32 moves a
point by at most sqrt(3) u L each, rounding the vertex / centre tables moves the surface by as much, one level of f32
transform by at most 3 u L: (2 sqrt(3) + 3) u L ~ 6.5 u L.

Closest hit, every ray:
  fit        class, material and front face equal the oracle's for the ray itself or for one of its copies (then the ray is
             EXCUSED; the copies are asked for lazily, only where the answer to the ray itself differs); else the ray fails.
  soundness  whatever fit: node is a reachable leaf of the right type with that material; o + t d (f64, from the f32 t) lies
             within the position bound of pos; pos lies in triangle prim / on the sphere / on the quad within that bound;
             u, v in [0, 1]; a miss or an environment hit carries the exact field values the f64 test demands.
  closeness  (not excused)  |pos - pos_ref| <= K_POS u L / max(|d^ . n^|, 1/64) with n^ the hit primitive's geometric normal;
             normal and (u, v) within K_DIR[kind] u L / s of the oracle's, kind = sphere / quad / mesh, s = the primitive's
             shortest edge or radius (u modulo 1 on spheres).
Occlusion: the answer equals the oracle's for the segment or for one of its copies.
At most CAP of a ray set may be excused (a condition, not a measurement).

K_POS and K_DIR are the smallest powers of two that are at least 4 times the largest ratio measured on the MI355X against the
oracle over all ray sets of tests/test_gpu_f32_rays.py (DESIGN.md section 14 has the table; the kernels are deterministic, the
factor covers a later compiler that reorders f32 arithmetic).  K_DIR is above 2^10 for one thing, named there: the normal of
a small sphere hit at grazing incidence far from the origin, where sphere_test's discriminant cancels."""
import atexit
import functools
import pathlib
import shutil
import tempfile

import numpy as np

from rust_raytracer_amd import api
from ray_query_cases import (ENVIRONMENT, MISS, SURFACE, T_MAX, T_MIN, Cases, cases, inside_triangle, klass_of, leaf_nodes,
                             oracle_hits, triangle_world)

U = 2.0 ** -24
DELTA = 8.0
CAP = 0.10
COS_FLOOR = 1.0 / 64
K_POS = 2.0 ** 9     # largest measured position ratio 105 (sphere_field)
# normal and (u, v) per kind of primitive.  Spheres: 748 and 140 measured (sphere_field, the grazing hit of DESIGN.md section 14).
# Quads and triangles: no ray set's largest ratio was on one of them except two_meshes' (mesh normal 25.2, quad uv 3.2), so
# the largest ratios of the sets that hold them bound theirs: normal <= 66.1 (nested_transform), (u, v) <= 140 (sphere_field).
K_DIR = {"sphere": {"normal": 2.0 ** 12, "uv": 2.0 ** 10},
         "quad": {"normal": 2.0 ** 9, "uv": 2.0 ** 10},
         "mesh": {"normal": 2.0 ** 9, "uv": 2.0 ** 10}}
KINDS = {api.RT_NODE_SPHERE: "sphere", api.RT_NODE_PLANE: "quad", api.RT_NODE_MESH: "mesh"}
FLT_MAX = float(np.finfo(np.float32).max)


def _unit(v):
    return v / np.linalg.norm(v)


class Geometry:
    """The primitives of a description in world space: one entry per (leaf node, path to it)."""

    def __init__(self, desc):
        self.desc = desc
        d = desc.contents
        self.leaves = leaf_nodes(desc)
        self.entries = []   # dicts: node, kind, material, m, and world-space data
        for n, mats in self.leaves.items():
            node = d.nodes[n]
            for m in mats:
                e = {"node": n, "type": node.type, "material": node.material, "m": m}
                if node.type == api.RT_NODE_MESH:
                    mesh = d.meshes[node.mesh]
                    pos = np.ctypeslib.as_array(mesh.positions, shape=(3 * mesh.n_positions,)).reshape(-1, 3)
                    idx = np.ctypeslib.as_array(mesh.tri_pos, shape=(3 * mesh.n_triangles,)).reshape(-1, 3)
                    e["tri"] = (pos @ m[:3, :3].T + m[:3, 3])[idx]          # (T, 3, 3)
                elif node.type in (api.RT_NODE_SPHERE, api.RT_NODE_PLANE):
                    e["inv"] = np.linalg.inv(m)
                    e["scale"] = abs(np.linalg.det(m[:3, :3])) ** (1.0 / 3.0)            # of sizes
                    e["stretch"] = float(np.linalg.svd(m[:3, :3], compute_uv=False).max())  # of distances: an upper bound
                    e["p"] = np.array(list(node.p))
                else:
                    continue
                self.entries.append(e)

    # distance (a length in world space) of p from every primitive of an entry, and the prim ids
    @staticmethod
    def _distance(e, p):
        if e["type"] == api.RT_NODE_MESH:
            tri = e["tri"]
            a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
            q = p - a
            g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
            b1, b2 = (q * e1).sum(1), (q * e2).sum(1)
            det = np.maximum(g11 * g22 - g12 * g12, 1e-300)
            s, t = (g22 * b1 - g12 * b2) / det, (g11 * b2 - g12 * b1) / det
            resid = np.linalg.norm(a + s[:, None] * e1 + t[:, None] * e2 - p, axis=1)
            out = np.maximum(np.maximum(-s, -t), np.maximum(s + t - 1.0, 0.0)) * np.sqrt(np.maximum(g11, g22))
            return resid + out
        po = (e["inv"] @ np.append(p, 1.0))[:3]
        pp = e["p"]
        if e["type"] == api.RT_NODE_SPHERE:
            return np.array([abs(np.linalg.norm(po - pp[:3]) - abs(pp[3])) * e["stretch"]])
        c, hu, hv = pp[0:3], pp[3:6], pp[6:9]
        q = po - c
        n = _unit(np.cross(hu, hv))
        a, b = q.dot(hu) / hu.dot(hu), q.dot(hv) / hv.dot(hv)
        out = max(0.0, abs(a) - 1.0) * np.linalg.norm(hu) + max(0.0, abs(b) - 1.0) * np.linalg.norm(hv)
        return np.array([(abs(q.dot(n)) + out) * e["stretch"]])

    def locate(self, p, material=None):
        """(entry, prim, distance) of the primitive nearest to p among the leaves with that material (None: all leaves)."""
        best = (None, -1, np.inf)
        for e in self.entries:
            if material is not None and e["material"] != material:
                continue
            dist = self._distance(e, p)
            k = int(np.argmin(dist))
            if dist[k] < best[2]:
                best = (e, k if e["type"] == api.RT_NODE_MESH else -1, float(dist[k]))
        return best

    def entries_of(self, node):
        return [e for e in self.entries if e["node"] == node]

    @staticmethod
    def numbers(e, prim):
        """The world-space numbers that define the primitive."""
        if e["type"] == api.RT_NODE_MESH:
            return e["tri"][prim].ravel()
        m, pp = e["m"], e["p"]
        if e["type"] == api.RT_NODE_SPHERE:
            c = (m @ np.append(pp[:3], 1.0))[:3]
            r = abs(pp[3]) * e["scale"]
            return np.concatenate([c - r, c + r])
        c, hu, hv = pp[0:3], pp[3:6], pp[6:9]
        corners = np.array([c + a * hu + b * hv for a in (-1, 1) for b in (-1, 1)])
        return (corners @ m[:3, :3].T + m[:3, 3]).ravel()

    @staticmethod
    def size(e, prim):
        """Shortest edge, or radius."""
        if e["type"] == api.RT_NODE_MESH:
            t = e["tri"][prim]
            return float(min(np.linalg.norm(t[1] - t[0]), np.linalg.norm(t[2] - t[1]), np.linalg.norm(t[0] - t[2])))
        pp = e["p"]
        if e["type"] == api.RT_NODE_SPHERE:
            return abs(pp[3]) * e["scale"]
        return 2.0 * min(np.linalg.norm(pp[3:6]), np.linalg.norm(pp[6:9])) * e["scale"]

    @staticmethod
    def geometric_normal(e, prim, p):
        if e["type"] == api.RT_NODE_MESH:
            t = e["tri"][prim]
            return _unit(np.cross(t[1] - t[0], t[2] - t[0]))
        m, pp = e["m"], e["p"]
        if e["type"] == api.RT_NODE_SPHERE:
            return _unit(e["inv"][:3, :3].T @ ((e["inv"] @ np.append(p, 1.0))[:3] - pp[:3]))
        return _unit(np.linalg.inv(m[:3, :3]).T @ np.cross(pp[3:6], pp[6:9]))

    def on_primitive(self, node, prim, p, tol):
        for e in self.entries_of(node):
            if e["type"] == api.RT_NODE_MESH:
                m = e["m"]
                if inside_triangle(p, triangle_world(self.desc, node, prim, m), tol):
                    return True
            elif self._distance(e, p)[0] <= tol:
                return True
        return False


def copies(o, d, t_point, delta):
    """The eight perturbed copies of a ray: (8, 3) origins and directions."""
    dh = _unit(d)
    axis = np.eye(3)[int(np.argmin(np.abs(dh)))]
    e1 = _unit(np.cross(dh, axis))
    e2 = np.cross(dh, e1)
    oo, dd = [], []
    for e in (e1, e2):
        for s in (1.0, -1.0):
            oo.append(o + s * delta * e)
            dd.append(d)
    for e in (e1, e2):
        for s in (1.0, -1.0):
            oo.append(o)
            dd.append(d + (s * delta / t_point) * e)
    return np.array(oo), np.array(dd)


def _key(klass, material, front, face=True):
    return (int(klass), int(material), bool(front) if (klass != MISS and face) else False)


def _front(got):
    return (got["flags"] & api.RT_RAY_FRONT_FACE) != 0


class Report:
    def __init__(self, label, n):
        self.label, self.n = label, n
        self.excused, self.failures = [], []
        self.r_pos = self.r_sound = 0.0
        self.r_kind = {k: {"normal": 0.0, "uv": 0.0} for k in K_DIR}   # largest normal and (u, v) ratio per kind of primitive

    @property
    def r_dir(self):
        return max(max(v.values()) for v in self.r_kind.values())

    def _field(self, kind, name, ratio):
        self.r_kind[kind][name] = max(self.r_kind[kind][name], float(ratio))

    @property
    def share(self):
        return len(self.excused) / max(self.n, 1)

    def line(self):
        return (f"{self.label}: {self.n} rays, {len(self.excused)} excused ({self.share:.2%}), {len(self.failures)} failures, "
                f"ratios pos {self.r_pos:.3g} sound {self.r_sound:.3g}; normal, uv: "
                + "; ".join(f"{k} {v['normal']:.3g}, {v['uv']:.3g}" for k, v in self.r_kind.items()))

    def check(self, k_pos=None, k_dir=None, show=True):
        """Prints the figures, then asserts: nothing failed, the excused share is under the cap, the ratios under the bounds
        (k_dir: one number for every kind and field, in place of K_DIR)."""
        k_pos = K_POS if k_pos is None else k_pos
        if show:
            print(self.line())
        assert not self.failures, f"{self.label}: {len(self.failures)} rays fail, first: {self.failures[:5]}"
        assert self.share <= CAP, f"{self.label}: {self.share:.2%} of the rays excused, cap {CAP:.0%}"
        assert self.r_pos <= k_pos and self.r_sound <= k_pos, f"{self.label}: position ratio {max(self.r_pos, self.r_sound):.4g} > {k_pos}"
        for kind, fields in self.r_kind.items():
            for name, r in fields.items():
                k = K_DIR[kind][name] if k_dir is None else k_dir
                assert r <= k, f"{self.label}: {kind} {name} ratio {r:.4g} > {k}"
        return self


def ray_scale(geom, o, ref, extent):
    """L of a closest-hit ray and, for a surface hit, the entry and prim the oracle hit."""
    if ref["klass"] != SURFACE:
        return max(float(np.abs(o).max()), extent), None, -1
    e, prim, _ = geom.locate(ref["pos"], int(ref["material"]))
    L = max(float(np.abs(o).max()), float(np.abs(ref["pos"]).max()), float(np.abs(geom.numbers(e, prim)).max()))
    return L, e, prim


def check_closest(geom, o, d, got, want, extent, label, t_min=T_MIN, oracle=None, face=True, uv=True):
    """The yardstick on closest-hit answers `got` (api.RtRayHit) to the rays (o, d), whose oracle answers are `want`
    (ray_query_cases.Expected).  `extent`: max |P| of the ray set.  face / uv = False: the records carry no front-face flag /
    no (u, v) (path vertices, vertex_records).  Returns a Report."""
    desc = geom.desc
    if oracle is None:
        oracle = lambda oo, dd: oracle_hits(desc, oo, dd, t_min)
    assert got.dtype == api.RtRayHit and len(got) == len(want) == len(o)
    nodes = desc.contents.nodes
    rep = Report(label, len(got))
    gk, gfront = klass_of(got), _front(got)
    assert (got["_reserved"] == 0).all()
    for i in range(len(got)):
        g, w = got[i], want[i]
        fail = lambda why: rep.failures.append((i, why))
        L, ref_e, ref_prim = ray_scale(geom, o[i], w, extent)
        # ---- fit
        key = _key(gk[i], g["material"], gfront[i], face)
        excused = key != _key(w["klass"], w["material"], w["front"], face)
        if excused:
            t_point = float(w["t"]) if w["klass"] == SURFACE else extent / np.linalg.norm(d[i])
            co, cd = copies(o[i], d[i], t_point, DELTA * U * L)
            alt = oracle(co, cd)
            if not any(key == _key(a["klass"], a["material"], a["front"], face) for a in alt):
                fail(f"answer {key} fits neither the oracle's {_key(w['klass'], w['material'], w['front'], face)} nor a copy's")
                continue
            rep.excused.append(i)
        # ---- soundness
        if gk[i] == MISS:
            if not (g["t"] == np.inf and g["flags"] == 0 and g["node"] == -1 and g["prim"] == -1 and g["material"] == -1 and
                    (g["pos"] == 0).all() and (g["normal"] == 0).all() and g["u"] == 0 and g["v"] == 0):
                fail("a miss with fields set")
            continue
        n = int(g["node"])
        if n not in geom.leaves or nodes[n].material != g["material"]:
            fail(f"node {n} is no reachable leaf with material {int(g['material'])}")
            continue
        if gk[i] == ENVIRONMENT:
            ty = nodes[n].type
            if not (ty in (api.RT_NODE_SKY, api.RT_NODE_SUN) and g["prim"] == -1 and (ty == api.RT_NODE_SKY) == (g["t"] == np.inf)
                    and g["t"] >= FLT_MAX):
                fail("environment hit with wrong node type, prim or t")
            continue
        ty = nodes[n].type
        is_mesh = ty == api.RT_NODE_MESH
        if not (ty in (api.RT_NODE_SPHERE, api.RT_NODE_PLANE, api.RT_NODE_MESH) and (g["prim"] >= 0) == is_mesh):
            fail(f"surface hit on node {n} of type {ty} with prim {int(g['prim'])}")
            continue
        prim = int(g["prim"])
        ents = geom.entries_of(n)
        if is_mesh and not prim < len(ents[0]["tri"]):
            fail(f"prim {prim} out of range")
            continue
        pos = g["pos"]
        dh = _unit(d[i])
        # the instance (path to the node) nearest to pos
        ge = min(ents, key=lambda e: geom._distance(e, pos)[prim if is_mesh else 0])
        Ls = max(L, float(np.abs(pos).max()), float(np.abs(geom.numbers(ge, prim)).max()))
        cos_g = max(abs(dh.dot(geom.geometric_normal(ge, prim, pos))), COS_FLOOR)
        r = np.linalg.norm(o[i] + g["t"] * d[i] - pos) * cos_g / (U * Ls)
        rep.r_sound = max(rep.r_sound, r)
        bound = K_POS * U * Ls / cos_g
        if not r <= K_POS:
            fail(f"o + t d is {r:.4g} u L / cos from pos")
        if not geom.on_primitive(n, prim, pos, bound):
            fail(f"pos does not lie on node {n} prim {prim} within {bound:.3g}")
        if uv and not (0.0 <= g["u"] <= 1.0 and 0.0 <= g["v"] <= 1.0):
            fail(f"u, v = {g['u']}, {g['v']} outside [0, 1]")
        # ---- closeness
        if excused:
            continue
        cos_r = max(abs(dh.dot(geom.geometric_normal(ref_e, ref_prim, w["pos"]))), COS_FLOOR)
        rep.r_pos = max(rep.r_pos, float(np.linalg.norm(pos - w["pos"])) * cos_r / (U * L))
        s = geom.size(ref_e, ref_prim)
        du = abs(g["u"] - w["u"]) if uv else 0.0
        if ref_e["type"] == api.RT_NODE_SPHERE:
            du = min(du, 1.0 - du)
        k, kind = s / (U * L), KINDS[ref_e["type"]]
        rep._field(kind, "normal", float(np.abs(g["normal"] - w["normal"]).max()) * k)
        if uv:
            rep._field(kind, "uv", max(du, abs(g["v"] - w["v"])) * k)
    return rep


def segment_scale(geom, o, d, occluded, t_min, t_max, t_end, oracle=oracle_hits):
    """L of a segment: its end points and the primitives it starts on, ends on and (oracle) is blocked by."""
    end = o + t_end * d
    L = max(float(np.abs(o).max()), float(np.abs(end).max()))
    pts = [o, end]
    if occluded:
        pts.append(oracle(geom.desc, o[None], d[None], t_min, t_max)["pos"][0])
    for p in pts:
        e, prim, _ = geom.locate(p)
        L = max(L, float(np.abs(geom.numbers(e, prim)).max()))
    return L


def check_occlusion(geom, o, d, got, want, label, t_min=T_MIN, t_max=T_MAX, t_end=1.0, oracle=oracle_hits):
    """The yardstick on occlusion answers (bool arrays) to the segments (o, d) over (t_min, t_max); o + t_end d is a
    segment's end point.  t_max and t_end: one number, or one per segment.  oracle: the yardstick, called like
    ray_query_cases.oracle_hits (the default; tests/special_ray_cases.py passes the unculled one)."""
    t_max, t_end = np.broadcast_to(np.asarray(t_max, dtype=np.float64), (len(o),)), np.broadcast_to(np.asarray(t_end, dtype=np.float64), (len(o),))
    desc = geom.desc
    rep = Report(label, len(got))
    assert got.dtype == bool and len(got) == len(want) == len(o)
    for i in np.nonzero(got != want)[0]:
        L = segment_scale(geom, o[i], d[i], want[i], t_min, t_max[i], t_end[i], oracle)
        co, cd = copies(o[i], d[i], t_end[i], DELTA * U * L)
        alt = oracle(desc, co, cd, t_min, t_max[i])["klass"] != MISS
        if (alt == got[i]).any():
            rep.excused.append(int(i))
        else:
            rep.failures.append((int(i), f"occluded = {bool(got[i])} fits neither the oracle's answer nor a copy's"))
    return rep


def fragile_share_closest(geom, o, d, want, extent, t_min=T_MIN, oracle=oracle_hits):
    """Share of rays with a copy whose oracle answer differs in class, material or face: an upper bound on what can be excused."""
    n = 0
    for i in range(len(o)):
        w = want[i]
        L, _, _ = ray_scale(geom, o[i], w, extent)
        t_point = float(w["t"]) if w["klass"] == SURFACE else extent / np.linalg.norm(d[i])
        co, cd = copies(o[i], d[i], t_point, DELTA * U * L)
        key = _key(w["klass"], w["material"], w["front"])
        n += any(key != _key(a["klass"], a["material"], a["front"]) for a in oracle(geom.desc, co, cd, t_min))
    return n / max(len(o), 1)


def fragile_share_segments(geom, o, d, want, t_min=T_MIN, t_max=T_MAX, t_end=1.0, oracle=oracle_hits):
    n = 0
    t_max, t_end = np.broadcast_to(np.asarray(t_max, dtype=np.float64), (len(o),)), np.broadcast_to(np.asarray(t_end, dtype=np.float64), (len(o),))
    for i in range(len(o)):
        L = segment_scale(geom, o[i], d[i], want[i], t_min, t_max[i], t_end[i], oracle)
        co, cd = copies(o[i], d[i], t_end[i], DELTA * U * L)
        n += ((oracle(geom.desc, co, cd, t_min, t_max[i])["klass"] != MISS) != want[i]).any()
    return n / max(len(o), 1)


def vertex_records(geom, t, pos, material, normal):
    """Path vertices (t, pos, material, normal per bounce, material < 0: a miss) in the shape of api.RtRayHit for
    check_closest(face=False, uv=False): node and prim are the primitive with that material nearest to pos."""
    out = np.zeros(len(t), dtype=api.RtRayHit)
    out["t"], out["material"], out["node"], out["prim"] = np.inf, -1, -1, -1
    nodes = geom.desc.contents.nodes
    for g, tt, p, m, n in zip(out, t, pos, material, normal):
        if m < 0:
            continue
        g["t"], g["pos"], g["normal"], g["material"], g["flags"] = tt, p, n, int(m), api.RT_RAY_HIT
        if tt >= FLT_MAX:
            g["flags"] |= api.RT_RAY_ENVIRONMENT
            ty = api.RT_NODE_SKY if tt == np.inf else api.RT_NODE_SUN
            g["node"] = next((k for k in geom.leaves if nodes[k].material == m and nodes[k].type == ty), -1)
        else:
            e, prim, _ = geom.locate(p, int(m))
            if e is not None:
                g["node"], g["prim"] = e["node"], prim
    return out


def as_ray_hits(geom, want):
    """The oracle's answers in the shape of api.RtRayHit, node and prim found by geometry: what a perfect kernel returns."""
    out = np.zeros(len(want), dtype=api.RtRayHit)
    out["t"], out["material"], out["node"], out["prim"] = np.inf, -1, -1, -1
    nodes = geom.desc.contents.nodes
    for g, w in zip(out, want):
        if w["klass"] == MISS:
            continue
        g["t"], g["material"] = w["t"], w["material"]
        g["flags"] = api.RT_RAY_HIT | (api.RT_RAY_FRONT_FACE if w["front"] else 0) | (api.RT_RAY_ENVIRONMENT if w["klass"] == ENVIRONMENT else 0)
        for f in ("pos", "normal", "u", "v"):
            g[f] = w[f]
        if w["klass"] == ENVIRONMENT:
            sky = w["t"] == np.inf
            g["node"] = next(n for n in geom.leaves if nodes[n].material == w["material"] and
                             nodes[n].type == (api.RT_NODE_SKY if sky else api.RT_NODE_SUN))
        else:
            e, prim, _ = geom.locate(w["pos"], int(w["material"]))
            g["node"], g["prim"] = e["node"], prim
    return out


# ---- ray sets ----
FLT_EPSILON = float(np.finfo(np.float32).eps)


class RaySet:
    """Closest-hit rays and segments of one description with the oracle's answers and the geometry to judge them by."""

    def __init__(self, label, hs, geom, o, d, hits, seg_o, seg_d, seg_occluded, extent, seg_lo=T_MIN, seg_hi=T_MAX):
        self.label, self.hs, self.geom, self.extent = label, hs, geom, extent
        self.o, self.d, self.hits = o, d, hits
        self.seg_o, self.seg_d, self.seg_occluded, self.seg_lo, self.seg_hi = seg_o, seg_d, seg_occluded, seg_lo, seg_hi

    def closest(self, got):
        return check_closest(self.geom, self.o, self.d, got, self.hits, self.extent, self.label + " closest")

    def occlusion(self, got):
        return check_occlusion(self.geom, self.seg_o, self.seg_d, got, self.seg_occluded, self.label + " segments",
                               self.seg_lo, self.seg_hi, self.seg_hi / T_MAX)

    def small_det_hits(self):
        """(mesh, quad) counts of oracle hits whose object-space determinant - |d . (e1 x e2)| = |d| * 2 area * cos of a triangle,
        |d . n^| of a quad - is below FLT_EPSILON, the absolute threshold the f32 kernels used to apply."""
        n = [0, 0]
        for d, w in zip(self.d, self.hits):
            if w["klass"] != SURFACE:
                continue
            e, prim, _ = self.geom.locate(w["pos"], int(w["material"]))
            if e["type"] == api.RT_NODE_MESH:
                t = e["tri"][prim]
                n[0] += abs(d.dot(np.cross(t[1] - t[0], t[2] - t[0]))) / abs(np.linalg.det(e["m"][:3, :3])) < FLT_EPSILON
            elif e["type"] == api.RT_NODE_PLANE:
                n[1] += abs((e["inv"][:3, :3] @ d).dot(_unit(np.cross(e["p"][3:6], e["p"][6:9])))) < FLT_EPSILON
        return tuple(n)

    def mesh_hits(self):
        mats = {e["material"] for e in self.geom.entries if e["type"] == api.RT_NODE_MESH}
        return int(((self.hits["klass"] == SURFACE) & np.isin(self.hits["material"], list(mats))).sum())

    def assert_not_vacuous(self, surface=0.3, mesh=0):
        """Conditions on the oracle's answers alone."""
        assert (self.hits["klass"] == SURFACE).mean() >= surface, f"{self.label}: too few surface hits"
        assert self.mesh_hits() >= mesh, f"{self.label}: {self.mesh_hits()} mesh hits"
        assert self.seg_occluded.mean() >= 0.1 and (~self.seg_occluded).mean() >= 0.1, f"{self.label}: one-sided segments"


def _from_cases(label, c):
    extent = float(np.abs(c.P).max())
    return RaySet(label, c.hs, Geometry(c.hs.desc), c.ab_o, c.ab_d, c.ab_hits, c.seg_o, c.seg_d, c.seg_occluded, extent)


@functools.lru_cache(maxsize=None)
def scene_set(name):
    """(a) the three ray sets of ray_query_cases for one of its scenes."""
    return _from_cases(name, cases(name))


@functools.lru_cache(maxsize=None)
def short_set(name, log2_scale):
    """(b) the camera rays plus LIFTED follow-ups (origin cam_o + 0.98 t cam_d, so that the fixed t_min = 0.001, in units of
    |d|, does not turn every on-surface start into a self-hit; the recipe's random direction), every direction scaled by
    2^log2_scale (exact in both precisions), and the segments scaled the same way over the same geometric interval."""
    c, base = cases(name), scene_set(name)
    s = 2.0 ** log2_scale
    surf = c.cam_hits["klass"] == SURFACE
    lifted = c.cam_o[surf] + 0.98 * c.cam_hits["t"][surf, None] * c.cam_d[surf]
    o, d = np.concatenate([c.cam_o, lifted]), np.concatenate([c.cam_d, c.fu_d]) * s
    seg_d, lo, hi = c.seg_d * s, T_MIN / s, T_MAX / s
    occ = oracle_hits(c.hs.desc, c.seg_o, seg_d, lo, hi)["klass"] != MISS
    return RaySet(f"{name} x 2^{log2_scale}", c.hs, base.geom, o, d, oracle_hits(c.hs.desc, o, d), c.seg_o, seg_d, occ,
                  base.extent, lo, hi)


GRID_SCENE = ("@config output_width = 40\n@config aspect_ratio = 1\n@config focal_length = 40\n"
              "@config camera_pos = 0,1.5,3\n@config camera_target = 0,0,0\n"
              "grid: transform (mesh grid.obj (glossy (constant 0.7,0.6,0.3) (constant 0.3))) s=50\n"
              "lamp: plane -0.5,2,-0.5 1,0,0 0,0,1 (emissive (constant 8,8,8)) backface\n"
              "sky: sky (constant 0.3,0.4,0.6)\nworld: list $grid $lamp $sky\nlights: list $lamp\n")


@functools.lru_cache(maxsize=None)
def grid_scene_path():
    """(c) small units under a transform: the 24 x 24 bumpy grid of tests/test_gpu_parity.py at scale 0.02 (object-space
    2 area ~ 3.3e-6) under s=50, a backface lamp at y = 2 and a sky."""
    from test_gpu_parity import _bumpy_grid_obj
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="f32_rays_"))
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    _bumpy_grid_obj(tmp / "grid.obj", 24, (0.0, 0.0, 0.0), (0.02, 0.02, 0.02))
    (tmp / "scene").write_text(GRID_SCENE)
    return str(tmp / "scene")


@functools.lru_cache(maxsize=None)
def grid_set():
    return _from_cases("scaled_grid", Cases(api.HostScene([grid_scene_path(), "-w=24", "-s=1", "--seed=31"])))


def fragile_shares(rs):
    """(closest-hit share, segment share) of a RaySet."""
    return (fragile_share_closest(rs.geom, rs.o, rs.d, rs.hits, rs.extent),
            fragile_share_segments(rs.geom, rs.seg_o, rs.seg_d, rs.seg_occluded, rs.seg_lo, rs.seg_hi, rs.seg_hi / T_MAX))
