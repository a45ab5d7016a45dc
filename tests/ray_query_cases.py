"""Ray sets and oracle answers for the ray-query tests (tests/test_ray_query_host.py, tests/test_gpu_ray_query.py).

Per scene, at -w=24 -s=1 --seed=31 (texture_mix: -w=12), with rng = numpy.random.default_rng(31):
  (a) camera rays   pyoracle.get_ray(camera, params, 0, x, y, 0, 0) for every pixel, row-major;
  (b) follow-ups    one per surface hit of (a), in order: origin = the oracle's hit position, direction = a normalised
                    rng.normal(3) times rng.uniform(0.5, 2) (not unit length, back faces included);
  (c) segments      perm = rng.permutation(len(P)) over those hit positions P: P[i] -> P[perm[i]], d = the difference (not
                    normalised), t_min = 1e-3, t_max = 0.999; i == perm[i] and |d| <= 1e-6 are skipped.
The yardstick is pyoracle.world_hit per ray; a segment is occluded iff world_hit(desc, o, d, 1e-3, 0.999) is not None.
Everything is computed once per scene and shared (the oracle rebuilds its world for every ray)."""
import functools
import os
import sys

import numpy as np

from oracle import pyoracle
from rust_raytracer_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = sys.float_info.max
T_MIN, T_MAX = 1e-3, 0.999

SCENES = {
    "cornell": "scenes/cornell", "light_test": "scenes/light_test",
    "two_meshes": "tests/scenes/two_meshes", "nested_transform": "tests/scenes/nested_transform", "sun_sky": "tests/scenes/sun_sky",
    "sphere_field": "tests/scenes/sphere_field", "hollow_glass": "tests/scenes/hollow_glass", "texture_mix": "tests/scenes/texture_mix",
    "smoke": "tests/scenes/smoke",
}
WIDTHS = {"texture_mix": 12}

MISS, SURFACE, ENVIRONMENT = 0, 1, 2
# what the oracle says about a ray, in the shape of api.RtRayHit plus the class
Expected = np.dtype([("klass", "i4"), ("t", "f8"), ("pos", "f8", (3,)), ("normal", "f8", (3,)), ("u", "f8"), ("v", "f8"),
                     ("front", "?"), ("material", "i4")])


def host_scene(name):
    return api.HostScene([SCENES[name], f"-w={WIDTHS.get(name, 24)}", "-s=1", "--seed=31"])


def oracle_hits(desc, origins, dirs, t_min=T_MIN, t_max=float("inf")):
    out = np.zeros(len(origins), dtype=Expected)
    out["material"] = -1
    out["t"] = np.inf
    for i, (o, d) in enumerate(zip(origins, dirs)):
        h = pyoracle.world_hit(desc, o, d, t_min, t_max)
        if h is None:
            continue
        e = out[i]
        e["klass"] = ENVIRONMENT if (h["t"] == np.inf or h["t"] == DBL_MAX) else SURFACE
        e["t"], e["pos"], e["normal"] = h["t"], h["pos"], h["normal"]
        e["u"], e["v"] = h["uv"]
        e["front"], e["material"] = h["front_face"], h["material"]
    return out


def camera_rays(hs):
    """Ray set (a): origins and directions, (n, 3) each."""
    cam, prm = hs.camera, hs.params
    rays = np.array([pyoracle.get_ray(cam, prm, 0, x, y, 0, 0) for y in range(cam.image_height) for x in range(cam.image_width)])
    return np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:])


class Cases:
    """The three ray sets of a scene with the oracle's answers."""

    def __init__(self, hs):
        self.hs = hs
        cam, prm = hs.camera, hs.params
        self.cam_o, self.cam_d = camera_rays(hs)
        self.cam_hits = oracle_hits(hs.desc, self.cam_o, self.cam_d)
        rng = np.random.default_rng(31)
        P = self.cam_hits["pos"][self.cam_hits["klass"] == SURFACE]
        self.P = P
        fd = []
        for _ in range(len(P)):
            v = rng.normal(size=3)
            fd.append(v / np.linalg.norm(v) * rng.uniform(0.5, 2))
        self.fu_o, self.fu_d = np.ascontiguousarray(P), np.array(fd).reshape(-1, 3)
        self.fu_hits = oracle_hits(hs.desc, self.fu_o, self.fu_d)
        perm = rng.permutation(len(P))
        so, sd = [], []
        for i in range(len(P)):
            d = P[perm[i]] - P[i]
            if i == perm[i] or np.linalg.norm(d) <= 1e-6:
                continue
            so.append(P[i])
            sd.append(d)
        self.seg_o, self.seg_d = np.array(so).reshape(-1, 3), np.array(sd).reshape(-1, 3)
        self.seg_occluded = oracle_hits(hs.desc, self.seg_o, self.seg_d, T_MIN, T_MAX)["klass"] != MISS
        self.extent = max(1.0, float(np.abs(P).max())) if len(P) else 1.0

    @property
    def ab_o(self):
        return np.concatenate([self.cam_o, self.fu_o])

    @property
    def ab_d(self):
        return np.concatenate([self.cam_d, self.fu_d])

    @property
    def ab_hits(self):
        return np.concatenate([self.cam_hits, self.fu_hits])

    def assert_not_vacuous(self):
        """The ray sets test something (conditions on the oracle's answers, not tolerances)."""
        assert (self.cam_hits["klass"] == SURFACE).mean() >= 0.5
        assert (self.fu_hits["klass"] == SURFACE).mean() >= 0.1
        assert self.seg_occluded.mean() >= 0.1
        assert (~self.seg_occluded).mean() >= 0.1


@functools.lru_cache(maxsize=None)
def cases(name):
    return Cases(host_scene(name))


# ---- the description's tree ----
def _mat4(t):
    return np.array(list(t.m)).reshape(4, 4)


def leaf_nodes(desc):
    """{node index: [world matrix, ...]} of every Sphere / Plane / Mesh / Sky / Sun node reachable from world_root (one matrix per
    path that reaches it)."""
    d = desc.contents
    leaves = {}

    def walk(n, m):
        node = d.nodes[n]
        if node.type in (api.RT_NODE_SPHERE, api.RT_NODE_PLANE, api.RT_NODE_MESH, api.RT_NODE_SKY, api.RT_NODE_SUN):
            leaves.setdefault(n, []).append(m)
            return
        if node.type == api.RT_NODE_TRANSFORM:
            m = m @ _mat4(d.transforms[node.transform])
        for k in range(node.n_children):
            walk(d.child_indices[node.first_child + k], m)

    walk(d.world_root, np.eye(4))
    return leaves


def triangle_world(desc, node, prim, m):
    """The three world-space corners of triangle `prim` (RtMesh.tri_pos order) of mesh node `node` under world matrix m."""
    d = desc.contents
    mesh = d.meshes[d.nodes[node].mesh]
    assert 0 <= prim < mesh.n_triangles
    idx = [mesh.tri_pos[3 * prim + k] for k in range(3)]
    pts = np.array([[mesh.positions[3 * i + a] for a in range(3)] + [1.0] for i in idx])
    return (pts @ m.T)[:, :3]


def inside_triangle(p, tri, tol):
    """p lies in the triangle's plane and inside its edges, within tol (a length)."""
    a, e1, e2 = tri[0], tri[1] - tri[0], tri[2] - tri[0]
    st, *_ = np.linalg.lstsq(np.stack([e1, e2], axis=1), p - a, rcond=None)
    resid = np.linalg.norm(a + st[0] * e1 + st[1] * e2 - p)
    rel = tol / max(min(np.linalg.norm(e1), np.linalg.norm(e2)), 1e-300)
    return resid <= tol and st[0] >= -rel and st[1] >= -rel and st[0] + st[1] <= 1 + rel


# ---- comparisons ----
def close(a, b, rel=1e-12, floor=1e-15):
    """The bar of tests/test_gpu_parity.py; non-finite values must be the same kind."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    ok = np.where(fin, np.abs(a - np.where(fin, b, 0.0)) <= np.maximum(rel * np.abs(np.where(fin, b, 0.0)), floor), False)
    same_kind = (np.isnan(a) & np.isnan(b)) | (~fin & (a == b))
    return ok | same_kind


def klass_of(hits):
    """MISS / SURFACE / ENVIRONMENT from the flags of an api.RtRayHit array."""
    hit = (hits["flags"] & api.RT_RAY_HIT) != 0
    env = (hits["flags"] & api.RT_RAY_ENVIRONMENT) != 0
    return np.where(hit, np.where(env, ENVIRONMENT, SURFACE), MISS)


def assert_hits_equal_oracle(got, want, desc=None, extent=1.0, tied=None, exact=None):
    """f64: class, material and front face equal for every ray, the reals at the parity bar; with `desc` also node and prim.
    tied (bool per ray, tests/special_ray_cases.py): rays on which several primitives of the winning object tie, where normal,
    u and v depend on which of them wins and are left to the caller.  exact (bool per ray): t and pos must be the oracle's bits."""
    assert got.dtype == api.RtRayHit and len(got) == len(want)
    np.testing.assert_array_equal(klass_of(got), want["klass"])
    hit = want["klass"] != MISS
    np.testing.assert_array_equal(got["material"], want["material"])
    np.testing.assert_array_equal(((got["flags"] & api.RT_RAY_FRONT_FACE) != 0)[hit], want["front"][hit])
    assert (got["_reserved"] == 0).all()
    miss = got[~hit]
    assert (miss["t"] == np.inf).all() and (miss["flags"] == 0).all() and (miss["node"] == -1).all() and (miss["prim"] == -1).all()
    assert (miss["pos"] == 0).all() and (miss["normal"] == 0).all() and (miss["u"] == 0).all() and (miss["v"] == 0).all()
    for f in ("t", "pos", "normal", "u", "v"):
        sel = hit if (tied is None or f in ("t", "pos")) else hit & ~tied
        ok = close(got[f][sel], want[f][sel])
        assert ok.all(), f"{f}: {int((~ok).sum())} values beyond 1e-12 relative"
    if exact is not None:
        for f in ("t", "pos"):
            assert got[f][hit & exact].tobytes() == want[f][hit & exact].tobytes(), f"{f}: not the oracle's bits"
    if desc is None:
        return
    d = desc.contents
    leaves = leaf_nodes(desc)
    for g, w in zip(got[hit], want[hit]):
        n = int(g["node"])
        assert n in leaves, f"node {n} is no reachable leaf"
        node = d.nodes[n]
        assert node.material == g["material"]
        if w["klass"] == ENVIRONMENT:
            assert node.type in (api.RT_NODE_SKY, api.RT_NODE_SUN) and g["prim"] == -1
            assert (node.type == api.RT_NODE_SKY) == (g["t"] == np.inf)
        elif node.type == api.RT_NODE_MESH:
            assert any(inside_triangle(g["pos"], triangle_world(desc, n, int(g["prim"]), m), 1e-9 * extent) for m in leaves[n]), \
                f"hit of node {n} does not lie in its triangle {int(g['prim'])}"
        else:
            assert node.type in (api.RT_NODE_SPHERE, api.RT_NODE_PLANE) and g["prim"] == -1
