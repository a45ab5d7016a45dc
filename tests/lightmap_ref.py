"""The texel rule of rt_lightmap_texels (include/rt_mi355.h) in numpy: all triangles x all texels,
elementwise f64 operations in the stated order (numpy rounds every operation once, like the library built with
-ffp-contract=off), the dilation of rt_lightmap_dilate, and the scenes of tests/test_lightmap_host.py and
tests/test_gpu_lightmap.py: a small OBJ with `vt` lines written to a temporary directory and a DSL scene around it, as
tests/deep_stack_cases.py builds its chains.

The parity bar is the project's f64 bar, 1e-12 * max(1, extent) on pos / normal / u / v (extent: the largest |world coordinate|
of the mesh); prim, count and flags must be equal."""
import atexit
import functools
import os
import pathlib
import shutil
import tempfile

import numpy as np

from rust_raytracer_amd import api

REPO = pathlib.Path(__file__).resolve().parent.parent
CUBE = REPO / "tests" / "scenes" / "cube.obj"
MONKEY = REPO / "scenes" / "resource" / "monkey_low.obj"
HIT_FRONT = api.RT_RAY_HIT | api.RT_RAY_FRONT_FACE


# ---- the rule ----
def centres(n):
    return (np.arange(n, dtype=np.float64) + 0.5) / np.float64(n)


def edge(su, sv, tu, tv, qu, qv):
    return (tu - su) * (qv - sv) - (tv - sv) * (qu - su)


def cedge(su, sv, tu, tv, qu, qv):
    ordered = (su < tu) | ((su == tu) & (sv <= tv))
    return np.where(ordered, edge(su, sv, tu, tv, qu, qv), -edge(tu, tv, su, sv, qu, qv))


def weights(a, b, c, pu, pv):
    """a, b, c: (..., 2) corners, pu / pv broadcastable against a[..., 0] -> (A, w_a, w_b, w_c) with A's sign taken out."""
    A = cedge(a[..., 0], a[..., 1], b[..., 0], b[..., 1], c[..., 0], c[..., 1])
    wa = cedge(b[..., 0], b[..., 1], c[..., 0], c[..., 1], pu, pv)
    wb = cedge(c[..., 0], c[..., 1], a[..., 0], a[..., 1], pu, pv)
    wc = cedge(a[..., 0], a[..., 1], b[..., 0], b[..., 1], pu, pv)
    neg = A < 0
    A = np.where(neg, -A, A) + np.zeros_like(wa)
    return A, np.where(neg, -wa, wa), np.where(neg, -wb, wb), np.where(neg, -wc, wc)


def coverage(uv, live, w, h, chunk=64):
    """uv: (T, 3, 2) corners, live: (T,) the triangle has UV indices -> (count (h, w) uint32, lowest covering triangle (h, w)
    int64, -1 where there is none)."""
    pu, pv = centres(w)[None, None, :], centres(h)[None, :, None]
    count = np.zeros((h, w), dtype=np.uint32)
    prim = np.full((h, w), -1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(0, len(uv), chunk):
            t = uv[t0:t0 + chunk]
            A, wa, wb, wc = weights(t[:, 0, None, None, :], t[:, 1, None, None, :], t[:, 2, None, None, :], pu, pv)
            cov = (A > 0) & (wa >= 0) & (wb >= 0) & (wc >= 0) & live[t0:t0 + chunk, None, None]
            count += cov.sum(axis=0).astype(np.uint32)
            first = np.where(cov.any(axis=0), t0 + cov.argmax(axis=0), -1)
            prim = np.where((prim < 0) & (first >= 0), first, prim)
    return count, prim


def _unit(v):
    return v / np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])[..., None]


def _apply(m, v, w):
    """Rows 0 .. 2 of the row-major 4 x 4 `m` times (v, w), summed left to right (mat4.rs:342-353)."""
    return np.stack([m[4 * r] * v[..., 0] + m[4 * r + 1] * v[..., 1] + m[4 * r + 2] * v[..., 2] + m[4 * r + 3] * w for r in range(3)], axis=-1)


class Mesh:
    """The arrays of mesh node `node` of a description and the transforms above it, innermost first."""

    def __init__(self, desc, node):
        d = desc.contents if hasattr(desc, "contents") else desc
        n = d.nodes[node]
        assert n.type == 3, "not an RT_NODE_MESH"
        m = d.meshes[n.mesh]
        arr = np.ctypeslib.as_array
        self.node, self.material, self.flat = node, n.material, bool(m.flags & 1)
        self.positions = arr(m.positions, shape=(m.n_positions, 3)).copy()
        self.normals = arr(m.normals, shape=(m.n_normals, 3)).copy()
        self.uvs = arr(m.uvs, shape=(m.n_uvs, 3)).copy()
        self.tri_pos = arr(m.tri_pos, shape=(m.n_triangles, 3)).copy()
        self.tri_nrm = arr(m.tri_nrm, shape=(m.n_triangles, 3)).copy()
        self.tri_uv = arr(m.tri_uv, shape=(m.n_triangles, 3)).copy()
        self.live = (self.tri_uv >= 0).all(axis=1)
        self.uv = self.uvs[np.where(self.tri_uv >= 0, self.tri_uv, 0)][..., :2]   # (T, 3, 2); dead triangles: any numbers
        self.chain = self._chain(d, node)
        world = self.positions
        for m4 in self.chain:
            world = _apply(m4, world, 1.0)
        self.extent = float(np.abs(world).max())
        self.tol = 1e-12 * max(1.0, self.extent)

    @staticmethod
    def _chain(d, node):
        """The `m` arrays of the RT_NODE_TRANSFORMs on the way from the world root down to `node`, innermost first."""
        def walk(i, above):
            n = d.nodes[i]
            if i == node:
                return above
            here = [np.array(d.transforms[n.transform].m[:])] + above if n.type == 5 else above
            for k in range(n.n_children):
                got = walk(d.child_indices[n.first_child + k], here)
                if got is not None:
                    return got
            return None
        got = walk(d.world_root, [])
        assert got is not None, "node is not reachable from the world root"
        return got


def rasterise(mesh, w, h):
    """-> an (h, w) array of api.RtRayHit and the (h, w) uint32 counts: what rt_lightmap_texels must give."""
    count, prim = coverage(mesh.uv, mesh.live, w, h)
    out = np.zeros((h, w), dtype=api.RtRayHit)
    out["t"] = np.inf
    out["material"] = out["node"] = out["prim"] = -1
    ys, xs = np.nonzero(prim >= 0)
    if len(ys) == 0:
        return out, count
    t = prim[ys, xs]
    uv = mesh.uv[t]
    A, _, wb, wc = weights(uv[:, 0], uv[:, 1], uv[:, 2], centres(w)[xs], centres(h)[ys])
    bu, bv = wb / A, wc / A
    bw = 1.0 - bu - bv
    p0, p1, p2 = (mesh.positions[mesh.tri_pos[t, k]] for k in range(3))
    e1, e2 = p1 - p0, p2 - p0
    pos = p0 + (e1 * bu[:, None] + e2 * bv[:, None])
    if mesh.flat:
        normal = _unit(np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                                 e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=-1))
    else:
        n0, n1, n2 = (mesh.normals[mesh.tri_nrm[t, k]] for k in range(3))
        normal = n0 * bw[:, None] + n1 * bu[:, None] + n2 * bv[:, None]
    for m4 in mesh.chain:
        pos = _apply(m4, pos, 1.0)
        normal = _unit(_apply(m4, normal, 0.0))
    if not mesh.chain:
        normal = _unit(normal)
    rec = np.zeros(len(t), dtype=api.RtRayHit)
    rec["pos"], rec["normal"] = pos, normal
    rec["u"] = uv[:, 0, 0] * bw + uv[:, 1, 0] * bu + uv[:, 2, 0] * bv
    rec["v"] = uv[:, 0, 1] * bw + uv[:, 1, 1] * bu + uv[:, 2, 1] * bv
    rec["material"], rec["node"], rec["prim"], rec["flags"] = mesh.material, mesh.node, t, HIT_FRONT
    out[ys, xs] = rec
    return out, count


def compare(got, got_count, ref, ref_count, tol):
    """The bar of this module's docstring; raises AssertionError naming the first field that misses it."""
    assert got.shape == ref.shape and got_count.shape == ref_count.shape
    bad = np.argwhere(got_count != ref_count)
    assert len(bad) == 0, f"count differs at {len(bad)} texels, first (y, x) = {bad[0]}: {got_count[tuple(bad[0])]} != {ref_count[tuple(bad[0])]}"
    for f in ("prim", "flags", "material", "node", "_reserved"):
        bad = np.argwhere(got[f] != ref[f])
        assert len(bad) == 0, f"{f} differs at {len(bad)} texels, first (y, x) = {bad[0]}: {got[f][tuple(bad[0])]} != {ref[f][tuple(bad[0])]}"
    assert np.array_equal(got["t"], ref["t"]), "t differs"
    for f in ("pos", "normal", "u", "v"):
        err = float(np.abs(got[f] - ref[f]).max()) if got.size else 0.0
        print(f"  {f}: max |difference| {err:.3e} (bar {tol:.3e})")
        assert err <= tol, f"{f}: max |difference| {err:.3e} above {tol:.3e}"


# ---- dilation ----
def dilate(rgba, cov, passes):
    """rt_lightmap_dilate: (h, w, 4) float64, (h, w) coverage -> the same after `passes` passes (coverage as 0 / 1 bytes)."""
    img = np.array(rgba, dtype=np.float64)
    c = np.asarray(cov) != 0
    h, w = c.shape
    for _ in range(passes):
        pad_c = np.zeros((h + 2, w + 2), dtype=bool)
        pad_c[1:-1, 1:-1] = c
        pad_i = np.zeros((h + 2, w + 2, 4))
        pad_i[1:-1, 1:-1] = img
        total, n = np.zeros((h, w, 4)), np.zeros((h, w))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                nc = pad_c[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                total = total + np.where(nc[..., None], pad_i[1 + dy:1 + dy + h, 1 + dx:1 + dx + w], 0.0)
                n = n + nc
        fill = ~c & (n > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            img = np.where(fill[..., None], total / n[..., None], img)
        c = c | fill
    return img, c.astype(np.uint8)


# ---- scenes ----
@functools.lru_cache(maxsize=None)
def _tmp():
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="lightmap_"))
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    return tmp


_HEAD = ("@config output_width = 32\n@config aspect_ratio = 1\n@config focal_length = 40\n@config camera_pos = 0,1.5,6\n"
         "@config camera_target = 0,0.5,0\nwhite: lambertian (constant 0.73,0.73,0.73)\n"
         "light: plane 0,4,0 1.5,0,0 0,0,1.5 (emissive (constant 10,10,10)) backface\n")


def _rel(path):
    return os.path.relpath(str(path), str(_tmp()))


def scene_text(name, body, world):
    """Writes `_HEAD + body` with the world list `world` (the light is added) and returns the file's path."""
    p = _tmp() / name
    p.write_text(_HEAD + body + f"world: list {world} $light\nlights: list $light\n")
    return str(p)


def new_host_scene(name, body, world):
    return api.HostScene([scene_text(name, body, world), "-w=32", "-s=2", "--seed=5"])


def mesh_nodes(desc):
    d = desc.contents
    return [i for i in range(d.n_nodes) if d.nodes[i].type == 3]


def write_obj(name, v, vt, vn, faces):
    """faces: per face three (v, vt or None, vn) triples, 1-based."""
    lines = [f"v {float(a)!r} {float(b)!r} {float(c)!r}" for a, b, c in v]
    lines += [f"vt {float(a)!r} {float(b)!r}" for a, b in vt]
    lines += [f"vn {float(a)!r} {float(b)!r} {float(c)!r}" for a, b, c in vn]
    for f in faces:
        lines.append("f " + " ".join(f"{a}//{c}" if b is None else f"{a}/{b}/{c}" for a, b, c in f))
    path = _tmp() / name
    path.write_text("\n".join(lines) + "\n")
    return path


CUBE_BODY = "m: transform (mesh {obj} $white) s=0.7 ry=25 t=0.2,0.5,-0.1\n"
MONKEY1_BODY = "m: transform (mesh {obj} $white) s=0.8 ry=30 t=-1.1,0.8,0\n"
MONKEY2_BODY = "m: transform (transform (mesh {obj} $white) s=0.8,1.1,0.9 ry=30 t=-1.1,0.8,0) rx=-15 rz=10 t=0.5,0.2,1\n"


@functools.lru_cache(maxsize=None)
def host_scene(name):
    """Shared scenes: nobody writes into them."""
    if name == "cube":
        return new_host_scene("cube", CUBE_BODY.format(obj=_rel(CUBE)), "$m")
    if name == "monkey1":
        return new_host_scene("monkey1", MONKEY1_BODY.format(obj=_rel(MONKEY)), "$m")
    if name == "monkey2":
        return new_host_scene("monkey2", MONKEY2_BODY.format(obj=_rel(MONKEY)), "$m")
    if name == "monkey0":   # no transform at all: the normal is normalised once at the end
        return new_host_scene("monkey0", f"m: mesh {_rel(MONKEY)} $white\n", "$m")
    if name == "crafted":
        return new_host_scene("crafted", f"m: transform (mesh {_rel(crafted_obj())} $white) s=1.5 rx=20 t=0,0.3,0\n", "$m")
    if name == "grid":
        return new_host_scene("grid", f"m: transform (mesh {_rel(grid_obj())} $white) ry=10 t=0,0.5,0\n", "$m")
    if name == "octahedron":
        return new_host_scene("octahedron", f"m: transform (mesh {_rel(octahedron_obj())} $white) s=0.9 ry=33 rx=12 t=0.1,1,0.2\n", "$m")
    if name == "two":       # two meshes, like tests/scenes/two_meshes, with a floor to occlude and bounce
        return new_host_scene("two", "floor: plane 0,0,0 5,0,0 0,0,-5 $white\n" + MONKEY1_BODY.format(obj=_rel(MONKEY)) +
                              f"m2: transform (mesh {_rel(CUBE)} (lambertian (constant 0.2,0.5,0.8))) s=0.5 ry=-40 t=1.2,0.5,0.3\n", "$floor $m $m2")
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, w, h, flat=False):
    """(records, counts, Mesh) of the first mesh node of a shared scene, computed once.  flat: as if RT_MESH_FLAT_SHADING were set."""
    hs = host_scene(name)
    mesh = Mesh(hs.desc, mesh_nodes(hs.desc)[0])
    mesh.flat = mesh.flat or flat
    rec, cnt = rasterise(mesh, w, h)
    return rec, cnt, mesh


def crafted_obj():
    """One OBJ with everything the binning and the raster kernel can get wrong at once; positions are the UVs lifted onto a
    gentle surface z = 0.3 u v, normals tilted per vertex.  In file order:
      * two overlapping charts over [0.55, 0.95] x [0.05, 0.45]: chart B (a quad, two triangles) FIRST in the file, then, far
        later in the file, chart A over the same square; the lowest index must win wherever both cover;
      * a fan of 300 thin triangles around (0.2578125, 0.2578125), the middle of tile (1, 1) of a 64-texel map: that tile's list
        is longer than one LDS batch of 256;
      * a triangle whose UV box edges lie on tile borders (0.25 / 0.5 at 64 texels) and a triangle whose vertices are texel
        centres of a 64 x 64 map;
      * triangles partly below 0 and above 1, and one wholly outside;
      * a face without vt, and a face of zero UV area."""
    path = _tmp() / "crafted.obj"
    if path.exists():
        return path
    vt, faces = [], []

    def tri(a, b, c, with_vt=True):
        k = len(vt)
        vt.extend([a, b, c])
        faces.append([(k + 1, k + 1 if with_vt else None, k + 1), (k + 2, k + 2 if with_vt else None, k + 2), (k + 3, k + 3 if with_vt else None, k + 3)])

    lo, hi = (0.55, 0.05), (0.95, 0.45)
    tri(lo, (hi[0], lo[1]), hi)                       # chart B
    tri(lo, hi, (lo[0], hi[1]))
    c = (0.2578125, 0.2578125)
    ring = [(c[0] + 0.2 * np.cos(2 * np.pi * k / 300), c[1] + 0.2 * np.sin(2 * np.pi * k / 300)) for k in range(300)]
    for k in range(300):                              # the fan: shared edges, no cracks, every triangle touches the centre tile
        tri(c, ring[k], ring[(k + 1) % 300])
    tri((0.25, 0.5), (0.5, 0.5), (0.5, 0.75))         # box edges on tile borders of a 64-texel map (and of a 48 x 80 one in v)
    tri((8.5 / 64, 40.5 / 64), (14.5 / 64, 40.5 / 64), (8.5 / 64, 47.5 / 64))   # vertices on texel centres of 64 x 64
    tri((-0.2, 0.8), (0.1, 0.8), (0.1, 0.95))         # partly below 0
    tri((0.9, 0.7), (1.3, 0.7), (0.9, 1.2))           # partly above 1
    tri((1.5, 1.5), (1.8, 1.5), (1.5, 1.9))           # wholly outside
    tri((0.6, 0.6), (0.8, 0.6), (0.8, 0.8), with_vt=False)   # no vt: covers nothing
    tri((0.6, 0.6), (0.7, 0.7), (0.8, 0.8))           # zero UV area
    tri((0.95, 0.05), (0.95, 0.45), (0.55, 0.45))     # chart A, listed last: other diagonal, overlaps both triangles of chart B
    tri((0.95, 0.05), (0.55, 0.45), (0.55, 0.05))
    v = [(a, b, 0.3 * a * b) for a, b in vt]
    vn = [tuple(_unit(np.array([0.2 * np.sin(7 * a), 0.2 * np.cos(5 * b), 1.0]))) for a, b in vt]
    return write_obj("crafted.obj", v, vt, vn, faces)


GRID_N = 8


def grid_uv():
    """(9, 9, 2): the UVs of the 8 x 8 quad grid over [0.1, 0.9]^2 at non-dyadic coordinates: multiples of 1/7 and 1/11,
    scaled in."""
    u = 0.1 + 0.8 * np.array([0.0, 1 / 11, 2 / 7, 4 / 11, 3 / 7, 6 / 11, 5 / 7, 9 / 11, 1.0])
    v = 0.1 + 0.8 * np.array([0.0, 1 / 7, 3 / 11, 3 / 7, 5 / 11, 4 / 7, 8 / 11, 6 / 7, 1.0])
    return np.stack(np.meshgrid(u, v, indexing="xy"), axis=-1)   # [row j, column i] = (u_i, v_j)


def grid_masks(w, h):
    """(inside, clear, outside) masks of the texel centres of a w x h map over the grid: strictly inside the outline; in the
    interior of one of a quad's two triangles (off every grid line and off the quad's diagonal by a clear margin); clearly
    outside the outline."""
    g = grid_uv()
    pu, pv = np.meshgrid(centres(w), centres(h), indexing="xy")
    inside = (pu > g[0, 0, 0]) & (pu < g[0, -1, 0]) & (pv > g[0, 0, 1]) & (pv < g[-1, 0, 1])
    col = np.clip(np.searchsorted(g[0, :, 0], pu) - 1, 0, GRID_N - 1)
    row = np.clip(np.searchsorted(g[:, 0, 1], pv) - 1, 0, GRID_N - 1)
    u0, u1, v0, v1 = g[0, col, 0], g[0, col + 1, 0], g[row, 0, 1], g[row + 1, 0, 1]
    s, t = (pu - u0) / (u1 - u0), (pv - v0) / (v1 - v0)
    clear = inside & (np.minimum.reduce([s, 1 - s, t, 1 - t, np.abs(s - t)]) > 1e-9)
    outside = (pu < g[0, 0, 0] - 1e-9) | (pu > g[0, -1, 0] + 1e-9) | (pv < g[0, 0, 1] - 1e-9) | (pv > g[-1, 0, 1] + 1e-9)
    return inside, clear, outside


def moved_obj(src, name, amplitude=0.06):
    """`src` with every vertex moved smoothly and every vt moved a little; everything else line by line as it was (the structure
    rt_scene_update asks for)."""
    out = []
    for line in open(src).read().splitlines():
        if line.startswith("v "):
            x, y, z = (float(t) for t in line.split()[1:4])
            x, y, z = x + amplitude * np.sin(5 * y + 1), y + amplitude * np.sin(4 * z + 2), z + amplitude * np.sin(6 * x + 3)
            line = f"v {float(x)!r} {float(y)!r} {float(z)!r}"
        elif line.startswith("vt "):
            a, b = (float(t) for t in line.split()[1:3])
            line = f"vt {float(a + 0.004 * np.sin(9 * b))!r} {float(b + 0.004 * np.sin(7 * a))!r}"
        out.append(line)
    path = _tmp() / name
    path.write_text("\n".join(out) + "\n")
    return path


def grid_obj():
    path = _tmp() / "grid.obj"
    if path.exists():
        return path
    g = grid_uv().reshape(-1, 2)
    n = GRID_N + 1
    faces = []
    for j in range(GRID_N):
        for i in range(GRID_N):
            a, b, c, d = j * n + i + 1, j * n + i + 2, (j + 1) * n + i + 2, (j + 1) * n + i + 1
            faces.append([(a, a, 1), (b, b, 1), (c, c, 1)])
            faces.append([(a, a, 1), (c, c, 1), (d, d, 1)])
    return write_obj("grid.obj", [(a, 0.1 * np.sin(5 * a + 3 * b), b) for a, b in g], [tuple(x) for x in g], [(0.0, 1.0, 0.0)], faces)


def octahedron_obj():
    """A convex mesh with a non-overlapping UV layout: the eight faces of an octahedron, each its own right triangle in a
    4 x 2 layout of cells, inset a little.  Counter-clockwise seen from outside; flat normals per face."""
    path = _tmp() / "octahedron.obj"
    if path.exists():
        return path
    ax = [np.array(p, dtype=np.float64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    v, vt, vn, faces = [], [], [], []
    k = 0
    for sx in (0, 1):
        for sy in (2, 3):
            for sz in (4, 5):
                a, b, c = ax[sx], ax[sy], ax[sz]
                if np.dot(np.cross(b - a, c - a), a + b + c) < 0:
                    b, c = c, b
                cu, cv = (k % 4) * 0.25, (k // 4) * 0.5
                base = len(v)
                v += [tuple(a), tuple(b), tuple(c)]
                vt += [(cu + 0.02, cv + 0.03), (cu + 0.23, cv + 0.03), (cu + 0.02, cv + 0.47)]
                vn.append(tuple(_unit(a + b + c)))
                faces.append([(base + 1, base + 1, k + 1), (base + 2, base + 2, k + 1), (base + 3, base + 3, k + 1)])
                k += 1
    return write_obj("octahedron.obj", v, vt, vn, faces)
