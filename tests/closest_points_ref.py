"""Brute-force f64 reference for the point queries (include/rt_mi355.h rt_closest_points), shared by
tests/test_closest_points_host.py and tests/test_gpu_closest_points.py.

The candidates are the world-space primitives of a description as f32_ray_bounds.Geometry lists them (ray_query_cases.leaf_nodes
and its matrices): every mesh triangle, every sphere (world centre, radius |r| * s) and every parallelogram (its two world-space
triangles).  All distances are taken in WORLD space, so the reference does not share the kernel's object-space route; that is only
possible because the point queries refuse transform chains that are not similarities.

closest_on_triangles is the definition, vectorised over triangles: the plane distance where the projection lies inside all three
edges, otherwise the nearest of the three edge segments with the parameter clamped to [0, 1] (a zero-length edge: 0)."""
import numpy as np

from rust_raytracer_amd import api
from f32_ray_bounds import Geometry


def closest_on_segments(a, e, q):
    """a, e: (T, 3); q: (3,) -> (squared distance (T,), closest points (T, 3))."""
    ee = (e * e).sum(-1)
    t = np.where(ee > 0.0, ((q - a) * e).sum(-1) / np.where(ee > 0.0, ee, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    c = a + e * t[:, None]
    r = q - c
    return (r * r).sum(-1), c


def closest_on_triangles(tri, q):
    """tri: (T, 3, 3) corners, q: (3,) -> (distance (T,), closest points (T, 3)), in the arithmetic of `tri` / `q` (f64 or f32)."""
    tri = np.asarray(tri)
    q = np.asarray(q, dtype=tri.dtype)
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    p = q - v0
    n = np.cross(e1, e2)
    nn = (n * n).sum(-1)
    a = (np.cross(p, e2) * n).sum(-1)
    b = (np.cross(e1, p) * n).sum(-1)
    inside = (nn > 0) & (a >= 0) & (b >= 0) & (a + b <= nn)
    safe = np.where(nn > 0, nn, 1).astype(tri.dtype)
    h = (p * n).sum(-1)
    d_in = np.abs(h) / np.sqrt(safe)
    c_in = q - n * (h / safe)[:, None]
    d2, c = closest_on_segments(v0, e1, q)
    for aa, ee in ((v0, e2), (v0 + e1, e2 - e1)):
        d2k, ck = closest_on_segments(aa, ee, q)
        take = d2k < d2
        d2 = np.where(take, d2k, d2)
        c = np.where(take[:, None], ck, c)
    return np.where(inside, d_in, np.sqrt(d2)), np.where(inside[:, None], c_in, c)


def closest_on_sphere(centre, radius, q):
    """-> (distance, closest point, outward unit normal); q at the centre: towards +x."""
    centre = np.asarray(centre)
    q = np.asarray(q, dtype=centre.dtype)
    v = q - centre
    length = np.sqrt((v * v).sum())
    out = v / length if length > 0 else np.array([1.0, 0.0, 0.0], dtype=centre.dtype)
    r = abs(radius)
    return abs(length - r), centre + out * r, out


def parallelogram_triangles(c, hu, hv):
    """The two triangles (c-u-v, 2u, 2v) and (c+u+v, -2u, -2v) of centre +- u +- v as (2, 3, 3) corners."""
    c, hu, hv = (np.asarray(x, dtype=np.float64) for x in (c, hu, hv))
    lo, hi = c - hu - hv, c + hu + hv
    return np.array([[lo, lo + 2 * hu, lo + 2 * hv], [hi, hi - 2 * hu, hi - 2 * hv]])


class Reference:
    """The world-space candidates of a description.  prims: one row per candidate (entry index, node, prim: the triangle of a
    mesh, else -1)."""

    def __init__(self, desc):
        self.geom = Geometry(desc)
        self.desc = desc
        tris, ids = [], []
        self.spheres = []   # (entry index, world centre, world radius, row in prims)
        rows = 0
        for k, e in enumerate(self.geom.entries):
            m = e["m"]
            if e["type"] == api.RT_NODE_MESH:
                t = e["tri"]
                tris.append(t)
                ids.append(np.stack([np.full(len(t), k), np.full(len(t), e["node"]), np.arange(len(t))], axis=1))
                rows += len(t)
            elif e["type"] == api.RT_NODE_PLANE:
                pp = e["p"]
                t = parallelogram_triangles(pp[0:3], pp[3:6], pp[6:9]) @ m[:3, :3].T + m[:3, 3]
                tris.append(t)
                ids.append(np.array([[k, e["node"], -1], [k, e["node"], -1]]))
                rows += 2
        self.tri = np.concatenate(tris) if tris else np.zeros((0, 3, 3))
        self.tri_ids = np.concatenate(ids) if ids else np.zeros((0, 3), dtype=np.int64)
        for k, e in enumerate(self.geom.entries):
            if e["type"] == api.RT_NODE_SPHERE:
                pp, m = e["p"], e["m"]
                self.spheres.append((k, (m @ np.append(pp[:3], 1.0))[:3], abs(pp[3]) * e["scale"]))
        self.sphere_ids = np.array([[k, self.geom.entries[k]["node"], -1] for k, _, _ in self.spheres], dtype=np.int64).reshape(-1, 3)
        self.ids = np.concatenate([self.tri_ids, self.sphere_ids]).astype(np.int64)
        pts = [self.tri.reshape(-1, 3)] + [np.array([c - r, c + r]) for _, c, r in self.spheres]
        pts = np.concatenate(pts) if len(self.ids) else np.zeros((0, 3))
        self.lo, self.hi = (pts.min(0), pts.max(0)) if len(pts) else (np.zeros(3), np.zeros(3))
        self.extent = float(np.abs(pts).max()) if len(pts) else 1.0

    def distances(self, q):
        """(distance to every candidate (N,), closest point on every candidate (N, 3)), rows as in self.ids."""
        q = np.asarray(q, dtype=np.float64)
        d, c = closest_on_triangles(self.tri, q) if len(self.tri) else (np.zeros(0), np.zeros((0, 3)))
        ds, cs = [], []
        for _, centre, radius in self.spheres:
            dk, ck, _ = closest_on_sphere(centre, radius, q)
            ds.append(dk)
            cs.append(ck)
        return np.concatenate([d, np.array(ds)]), np.concatenate([c, np.array(cs).reshape(-1, 3)])

    def query(self, q, tol=0.0):
        """-> (d_ref, set of (node, prim) within tol of the minimum, all distances); nothing to find: (inf, empty set, [])."""
        d, _ = self.distances(q)
        if len(d) == 0 or not np.isfinite(d).any():
            return np.inf, set(), d
        d_ref = float(np.nanmin(d))
        near = np.nonzero(d <= d_ref + tol)[0]
        return d_ref, {(int(self.ids[k, 1]), int(self.ids[k, 2])) for k in near}, d

    def rows_of(self, node, prim):
        """Rows of self.ids that belong to the primitive (every instance of it; both halves of a quad)."""
        key = (int(node), int(prim))
        if not hasattr(self, "_rows"):
            self._rows = {}
        if key not in self._rows:
            self._rows[key] = np.nonzero((self.ids[:, 1] == key[0]) & (self.ids[:, 2] == key[1]))[0]
        return self._rows[key]

    def distance_to(self, q, node, prim):
        """The reference distance from the point q to the primitive (node, prim) (0 when q lies on it): the nearest of its
        instances and, for a quad, halves."""
        q = np.asarray(q, dtype=np.float64)
        rows = self.rows_of(node, prim)
        t_rows = rows[rows < len(self.tri)]
        best = np.inf
        if len(t_rows):
            best = float(closest_on_triangles(self.tri[t_rows], q)[0].min())
        for r in rows[rows >= len(self.tri)]:
            _, centre, radius = self.spheres[r - len(self.tri)]
            best = min(best, float(closest_on_sphere(centre, radius, q)[0]))
        return best

    def normal(self, node, prim, p):
        """Geometric unit normal of (node, prim) at p, world space (spheres: away from the centre); several instances: all."""
        out = []
        for e in self.geom.entries_of(node):
            if e["type"] == api.RT_NODE_SPHERE:
                c = (e["m"] @ np.append(e["p"][:3], 1.0))[:3]
                v = np.asarray(p) - c
                out.append(v / np.linalg.norm(v))
            else:
                out.append(Geometry.geometric_normal(e, prim, p))
        return out


def point_sets(ref, rng):
    """The point sets of the GPU test, in order, as {name: (n, 3)}: box, near (on random primitives, displaced by
    rng.normal(3) * 1e-3 * extent), far (1e4 * extent from the centre), vertices (16 exact world-space mesh vertices, if there
    are meshes), centres (every sphere centre)."""
    ext = ref.extent
    centre, half = 0.5 * (ref.lo + ref.hi), 0.5 * (ref.hi - ref.lo)
    sets = {"box": centre + (rng.uniform(-1.0, 1.0, size=(256, 3)) * 1.5) * half}
    near = []
    n_t, n_s = len(ref.tri), len(ref.spheres)
    for _ in range(256):
        k = int(rng.integers(n_t + n_s))
        if k < n_t:
            w = rng.dirichlet([1.0, 1.0, 1.0])
            p = w @ ref.tri[k]
        else:
            _, c, r = ref.spheres[k - n_t]
            v = rng.normal(size=3)
            p = c + r * v / np.linalg.norm(v)
        near.append(p + rng.normal(size=3) * 1e-3 * ext)
    sets["near"] = np.array(near)
    v = rng.normal(size=(16, 3))
    sets["far"] = centre + 1e4 * ext * v / np.linalg.norm(v, axis=1, keepdims=True)
    mesh_rows = np.nonzero(ref.tri_ids[:, 2] >= 0)[0]
    if len(mesh_rows):
        pick = rng.choice(mesh_rows, size=16)
        sets["vertices"] = ref.tri[pick, rng.integers(3, size=16)].copy()
    if n_s:
        sets["centres"] = np.array([c for _, c, _ in ref.spheres])
    return sets
