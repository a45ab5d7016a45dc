"""Scenes for the rt_scene_update tests (tests/test_scene_update_host.py, tests/test_gpu_scene_update.py): numeric variants
of tests/scenes/two_meshes and tests/scenes/smoke, and the 24 x 24 grid of tests/test_gpu_mesh_cones.py deformed in five ways
that keep its structure (vertex, normal, uv and face lines in the same order; only the `v` values differ)."""
import os
import re

import numpy as np

from rust_raytracer_amd import api
from test_gpu_mesh_cones import bumpy_grid_obj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONKEY = os.path.join(REPO, "scenes", "resource", "monkey_low.obj")
GRID_N = 24
GRID_CASES = ("phase", "fold_twist", "far", "tiny", "collapsed")
ATTR_CASE = "attributes"   # the same positions, other vertex normals and another uv: a mesh can move through those alone


def base_height(x, z):
    return 0.25 * np.sin(3.1 * x) * np.cos(2.3 * z) + 0.05 * np.sin(17 * x + 5 * z)


def grid_vertices(case):
    """(n + 1)^2 x 3 vertex positions of the grid in bumpy_grid_obj's order, for "base" or one of GRID_CASES."""
    n = GRID_N
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="xy")  # row j, column i: index j (n + 1) + i
    x, z = -1 + 2 * i / n, -1 + 2 * j / n
    y = base_height(x, z)
    if case == "phase":       # (i) the bump, phase-shifted
        y = 0.25 * np.sin(3.1 * x + 0.9) * np.cos(2.3 * z - 0.4) + 0.05 * np.sin(17 * x + 5 * z + 1.0)
    elif case == "fold_twist":  # (ii) y = |x|, then twisted by 180 degrees along z
        y = np.abs(x)
        ang = np.pi * (z + 1) / 2
        x, y = x * np.cos(ang) - y * np.sin(ang), x * np.sin(ang) + y * np.cos(ang)
    v = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    if case == "far":         # (iii) S grows from about 1 to 2000: a stale pad would under-cover
        v = v + np.array([1000.0, 0.0, -2000.0])
    elif case == "tiny":      # (iv)
        v = v * 0.02
    elif case == "collapsed":  # (v) twelve vertices onto their right-hand neighbours: zero-area triangles and slivers
        for q in range(12):
            jj, ii = 2 + (q * 5) % 20, 1 + (q * 7) % 21
            v[jj * (n + 1) + ii] = v[jj * (n + 1) + ii + 1]
    return v


def grid_obj(path, case):
    """The grid's OBJ with the structure bumpy_grid_obj writes."""
    bumpy_grid_obj(path, GRID_N, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    if case == "base":
        return
    v = iter(grid_vertices(case))
    lines, k = [], 0
    for line in path.read_text().splitlines():
        if line.startswith("v ") and case != ATTR_CASE:
            p = next(v)
            line = f"v {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}"
        elif line.startswith("vn ") and case == ATTR_CASE:   # one per vertex: tilted, a different tilt for each
            k += 1
            nx, nz = 0.4 * np.sin(0.7 * k), 0.4 * np.cos(1.3 * k)
            line = f"vn {float(nx)!r} 1 {float(nz)!r}"
        elif line.startswith("vt ") and case == ATTR_CASE:
            line = "vt 0.25 0.75"
        lines.append(line)
    path.write_text("\n".join(lines) + "\n")


def grid_camera(case):
    """(offset, size, camera_pos, camera_target) for grid_scene: the camera moves with the mesh (AWKWARD of test_gpu_mesh_cones)."""
    if case == "far":
        return (1000.0, 0.0, -2000.0), 1.0, "1000,1.5,-1997", "1000,0,-2000"
    if case == "tiny":
        return (0.0, 0.0, 0.0), 0.02, "0,0.03,0.06", "0,0,0"
    return (0.0, 0.0, 0.0), 1.0, "0,1.5,3", "0,0,0"


def grid_host_scene(tmp_path, case, view=None):
    """HostScene of the grid `case`, seen by the camera of `view` (default: its own)."""
    from test_gpu_mesh_cones import grid_scene
    d = tmp_path / f"grid_{case}_{view or case}"
    d.mkdir(exist_ok=True)
    grid_obj(d / "grid.obj", case)
    offset, s, cam, target = grid_camera(view or case)
    return grid_scene(d, "grid.obj", offset, s, cam, target)


def mesh_arrays(desc, mesh=0):
    """(positions (n, 3), tri_pos (t, 3)) of RtMesh `mesh`, copied."""
    m = desc.contents.meshes[mesh]
    pos = np.ctypeslib.as_array(m.positions, shape=(m.n_positions, 3)).copy()
    tri = np.ctypeslib.as_array(m.tri_pos, shape=(m.n_triangles, 3)).copy()
    return pos, tri


def displaced_obj(src, dst, amplitude=0.06):
    """`src` with every vertex moved smoothly; everything else line by line as it was."""
    out = []
    for line in open(src).read().splitlines():
        if line.startswith("v "):
            x, y, z = (float(t) for t in line.split()[1:4])
            x, y, z = x + amplitude * np.sin(5 * y + 1), y + amplitude * np.sin(4 * z + 2), z + amplitude * np.sin(6 * x + 3)
            line = f"v {float(x)!r} {float(y)!r} {float(z)!r}"
        out.append(line)
    dst.write_text("\n".join(out) + "\n")


def two_meshes_variant(tmp_path, name, numeric=True, m1=None, m2=None, args=("-w=64", "-s=16", "--seed=32")):
    """tests/scenes/two_meshes with other numbers (transforms, colours, roughness, light) and / or other OBJ files."""
    text = open(os.path.join(REPO, "tests", "scenes", "two_meshes")).read()
    rel = lambda p: os.path.relpath(str(p), str(tmp_path))
    objs = [rel(m1 or MONKEY), rel(m2 or MONKEY)]
    text = re.sub(r"\.\./\.\./scenes/resource/monkey_low\.obj", lambda _m: objs.pop(0), text)
    if numeric:
        for old, new in (("s=0.8 ry=30 t=-1.1,0.8,0", "s=0.9 ry=75 t=-1.0,0.9,0.2"), ("s=0.7 ry=-40 t=1.2,0.7,0.3", "s=0.6 ry=10 t=1.1,0.6,-0.2"),
                         ("constant 0.2,0.5,0.8) (constant 0.1)", "constant 0.8,0.3,0.2) (constant 0.35)"),
                         ("constant 0.9,0.7,0.3) (constant 0.1)", "constant 0.4,0.9,0.5) (constant 0.25)"),
                         ("constant 0.73,0.73,0.73", "constant 0.5,0.6,0.7"),
                         ("plane 0,4,0 1.5,0,0 0,0,1.5 (emissive (constant 10,10,10))", "plane 0.5,3.5,0.4 1.0,0,0 0,0,2.0 (emissive (constant 12,9,7))")):
            assert old in text, old
            text = text.replace(old, new)
    path = tmp_path / name
    path.write_text(text)
    hs = api.HostScene([str(path)] + list(args))
    if numeric:   # the scene language has no ior for a glossy material: another one goes straight into the description
        d = hs.desc.contents
        glossy = [k for k in range(d.n_materials) if d.materials[k].type == api.RT_MAT_GLOSSY]
        assert glossy
        for k in glossy:
            d.materials[k].ior = 1.9 if d.materials[k].ior != 1.9 else 1.4
    return hs


def smoke_variant(tmp_path, name, monkey_obj, args=("-w=48", "-s=16", "--seed=5")):
    """tests/scenes/smoke with the monkey (the mesh boundary of a volume) replaced and its transform changed."""
    text = open(os.path.join(REPO, "tests", "scenes", "smoke")).read()
    old = "../../scenes/resource/monkey_low.obj $white) s=70 ry=180 t=150,400,250"
    assert old in text
    text = text.replace(old, f"{os.path.relpath(str(monkey_obj), str(tmp_path))} $white) s=80 ry=150 t=170,380,240")
    path = tmp_path / name
    path.write_text(text)
    return api.HostScene([str(path)] + list(args))


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())
