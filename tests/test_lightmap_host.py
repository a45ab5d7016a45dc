"""The texel rule of lightmaps (include/rt_mi355.h rt_lightmap_texels) without a GPU:
rt_lightmap_texels_desc - the rule of csrc/rt_lightmap.h by brute force on the host - against the numpy restatement of
tests/lightmap_ref.py.  prim, count and flags must be equal; pos, normal, u and v within 1e-12 * max(1, scene extent)."""
import numpy as np
import pytest

import lightmap_ref as lr
from rust_raytracer_amd import api

CASES = [("cube", 16, 16), ("cube", 37, 21), ("cube", 1, 1), ("monkey1", 100, 60), ("monkey2", 64, 64), ("monkey0", 33, 47),
         ("crafted", 64, 64), ("crafted", 48, 80), ("grid", 64, 64), ("octahedron", 40, 24)]


def first_mesh(name):
    hs = lr.host_scene(name)
    return hs, lr.mesh_nodes(hs.desc)[0]


@pytest.mark.parametrize("name,w,h", CASES)
def test_desc_matches_numpy_rule(name, w, h):
    hs, node = first_mesh(name)
    ref, ref_count, mesh = lr.reference(name, w, h)
    got, got_count = api.lightmap_texels_desc(hs.desc, node, w, h, counts=True)
    lr.compare(got, got_count, ref, ref_count, mesh.tol)


def test_flat_shading_on_the_description():
    hs = lr.new_host_scene("monkey1_flat", lr.MONKEY1_BODY.format(obj=lr._rel(lr.MONKEY)), "$m")
    hs.desc.contents.meshes[0].flags |= api.RT_MESH_FLAT_SHADING
    node = lr.mesh_nodes(hs.desc)[0]
    mesh = lr.Mesh(hs.desc, node)
    assert mesh.flat
    ref, ref_count = lr.rasterise(mesh, 64, 40)
    got, got_count = api.lightmap_texels_desc(hs.desc, node, 64, 40, counts=True)
    lr.compare(got, got_count, ref, ref_count, mesh.tol)
    smooth, _, _ = lr.reference("monkey1", 64, 40)
    assert np.abs(smooth["normal"] - ref["normal"]).max() > 1e-3, "flat shading changed no normal"


def test_cube_diagonal_ties_and_counts():
    """All six faces of the cube map onto the whole square, each as two triangles that share the diagonal u = v: a centre off the
    diagonal is covered by one triangle of every face (count 6), a centre exactly on it - x == y at 16 x 16 - by all twelve
    (count 12), and goes to triangle 0; prim is 0 or 1 everywhere."""
    hs, node = first_mesh("cube")
    for w, h in ((16, 16), (37, 21), (1, 1)):
        got, count = api.lightmap_texels_desc(hs.desc, node, w, h, counts=True)
        assert set(np.unique(got["prim"])) <= {0, 1}
        assert (got["flags"] == lr.HIT_FRONT).all() and (got["t"] == 0).all()
        y, x = np.mgrid[0:h, 0:w]
        on_diagonal = (2 * x + 1) * h == (2 * y + 1) * w   # centres with u == v exactly
        assert (count[~on_diagonal] == 6).all()
        assert (count[on_diagonal] == 12).all() and (got["prim"][on_diagonal] == 0).all()
        if (w, h) == (16, 16):
            assert np.array_equal(on_diagonal, x == y)
    assert on_diagonal.all()   # 1 x 1: the one centre is on it


def test_no_cracks_in_the_rule():
    """The 8 x 8 quad grid at non-dyadic UVs: every centre strictly inside the outline is covered, every centre in the interior
    of a triangle exactly once - first by the numpy rule, then by the library's."""
    hs, node = first_mesh("grid")
    w = h = 64
    inside, clear, outside = lr.grid_masks(w, h)
    assert inside.sum() > 2000 and clear.sum() > 2000
    for count in (lr.reference("grid", w, h)[1], api.lightmap_texels_desc(hs.desc, node, w, h, counts=True)[1]):
        assert (count[inside] >= 1).all(), "a crack: an inside centre that no triangle covers"
        assert (count[clear] == 1).all()
        assert (count[outside] == 0).all()


def test_crafted_mesh_holds_what_it_claims():
    """The crafted OBJ really exercises the mechanisms: one tile of the 64 x 64 map holds more than one LDS batch of triangles,
    the overlap goes to the lower index, the faces that cover nothing cover nothing."""
    rec, count, mesh = lr.reference("crafted", 64, 64)
    fan = np.arange(2, 302)
    assert count[16, 16] >= 1 and len(mesh.uv) == 311
    lo = mesh.uv[fan].min(axis=(1))
    hi = mesh.uv[fan].max(axis=(1))
    in_tile = ((lo[:, 0] * 64 < 32) & (hi[:, 0] * 64 > 16) & (lo[:, 1] * 64 < 32) & (hi[:, 1] * 64 > 16)).sum()
    assert in_tile > 256, "the centre tile's list fits one batch"
    chart = rec[4:28, 36:60]   # inside [0.55, 0.95] x [0.05, 0.45]
    assert set(np.unique(chart["prim"])) == {0, 1} and (count[4:28, 36:60] >= 2).all()
    assert not np.isin(rec["prim"], [307, 308]).any()       # no vt, zero area
    assert not (rec["prim"] == 306).any()                   # wholly outside
    assert (rec["prim"] == 304).any() and (rec["prim"] == 305).any()   # clipped by the square, not dropped
    assert (rec["prim"] == 303).sum() >= 20                 # vertices on texel centres: the corner centres are covered
    assert rec["prim"][40, 8] == 303 and rec["prim"][40, 14] == 303 and rec["prim"][47, 8] == 303


def test_dilation_reference_by_hand():
    img = np.zeros((3, 3, 4))
    cov = np.zeros((3, 3), dtype=np.uint8)
    img[0, 0] = [1, 2, 3, 4]
    img[2, 2] = [3, 2, 1, 0]
    cov[0, 0] = cov[2, 2] = 1
    out, c = lr.dilate(img, cov, 1)
    assert np.array_equal(out[1, 1], [2, 2, 2, 2]) and np.array_equal(out[0, 1], [1, 2, 3, 4]) and c[0, 2] == 0 and c.sum() == 7
    out2, c2 = lr.dilate(img, cov, 2)
    assert c2.all() and np.array_equal(out2[0, 2], (out[0, 1] + out[1, 1] + out[1, 2]) / 3)
    out0, c0 = lr.dilate(img, cov * 7, 0)
    assert np.array_equal(out0, img) and np.array_equal(c0, cov)


LIGHTMAP_MESSAGE = "Lightmap must be <k>:<width>[x<height>][:<passes>]"


@pytest.mark.parametrize("value", ["0", "0:", "a:16", "0:16x", "0:0", "0:16385", "0:16x0", "0:16:-1", "0:16:x", "0:16:2000", "-1:16"])
def test_lightmap_flag_malformed(value):
    with pytest.raises(RuntimeError, match="Lightmap must be"):
        api.HostScene(["scenes/cornell", "-w=16", f"--lightmap={value}"])


@pytest.mark.parametrize("other", ["--gpus=2", "--progressive=2", "--noise-threshold=0.1", "--pick=1,1", "--ao=4", "--probe=0,0,0", "--irradiance",
                                   "--sh-probe=0,0,0", "--nearest=0,0,0", "--pipeline=mega"])
def test_lightmap_flag_refused_combinations(other):
    with pytest.raises(RuntimeError, match="--lightmap bakes a lightmap"):
        api.HostScene(["scenes/cornell", "-w=16", "--lightmap=0:16", other])


def test_lightmap_flag_parsed_and_refused_with_sequence(tmp_path):
    import os
    import subprocess
    repo = str(lr.REPO)
    rtrace = os.path.join(repo, "rust_raytracer_amd", "rtrace")
    api.HostScene(["scenes/cornell", "-w=16", "--lightmap=3:48x20:5"])   # well-formed values load
    api.HostScene(["scenes/cornell", "-w=16", "--lightmap=0:64"])
    r = subprocess.run([rtrace, os.path.join(repo, "scenes/cornell"), "-w=16", "-s=4", "--lightmap=0:16", "--sequence=scenes/cornell"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--lightmap" in r.stderr and "--sequence" in r.stderr
    r = subprocess.run([rtrace, os.path.join(repo, "scenes/cornell"), "-w=16", "-s=4", "--max-depth=0", "--lightmap=0:16"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--lightmap needs a depth" in r.stderr, r.stderr


def _raw(desc, node, instance, w, h, hits, counts):
    lib = api.load_device_lib()
    st = lib.rt_lightmap_texels_desc(desc, node, instance, w, h, None if hits is None else hits.ctypes.data,
                                     None if counts is None else counts.ctypes.data)
    return st, lib.rt_last_error().decode()


def test_desc_refusals_leave_the_outputs_alone():
    hs, node = first_mesh("cube")
    d = hs.desc.contents
    hits = np.zeros(16 * 16, dtype=api.RtRayHit)
    hits["prim"] = 77
    counts = np.full(16 * 16, 99, dtype=np.uint32)
    not_mesh = next(i for i in range(d.n_nodes) if d.nodes[i].type != 3)
    cases = [((node, 0, 0, 16), api.RT_E_INVALID, "width"), ((node, 0, 16, 0), api.RT_E_INVALID, "height"),
             ((node, 0, 16385, 16), api.RT_E_INVALID, "width"), ((node, 0, 16, 16385), api.RT_E_INVALID, "height"),
             ((d.n_nodes, 0, 16, 16), api.RT_E_INVALID, "node"), ((not_mesh, 0, 16, 16), api.RT_E_INVALID, "node"),
             ((node, 1, 16, 16), api.RT_E_INVALID, "instance")]
    for args, status, word in cases:
        st, msg = _raw(hs.desc, *args, hits, counts)
        assert st == status and word in msg and msg.startswith("rt_lightmap_texels_desc"), (args, st, msg)
        assert (hits["prim"] == 77).all() and (counts == 99).all()
    st, msg = _raw(hs.desc, node, 0, 16, 16, None, counts)
    assert st == api.RT_E_INVALID and "hits_out" in msg
    st, msg = _raw(hs.desc, node, 0, 16, 16, hits, None)   # counts are optional
    assert st == api.RT_OK and (hits["prim"] != 77).all()


def test_desc_refuses_a_mesh_without_uvs_and_a_volume_boundary():
    obj = lr.write_obj("no_vt.obj", [(0, 0, 0), (1, 0, 0), (0, 1, 0)], [], [(0, 0, 1)], [[(1, None, 1), (2, None, 1), (3, None, 1)]])
    hs = lr.new_host_scene("no_vt", f"m: mesh {lr._rel(obj)} $white\n", "$m")
    hits = np.zeros(16, dtype=api.RtRayHit)
    hits["prim"] = 77
    st, msg = _raw(hs.desc, lr.mesh_nodes(hs.desc)[0], 0, 4, 4, hits, None)
    assert st == api.RT_E_UNSUPPORTED and "uv" in msg and (hits["prim"] == 77).all(), msg
    fog = lr.new_host_scene("fog", f"fog: isotropic (constant 0.9,0.9,1)\nm: volume (mesh {lr._rel(lr.CUBE)} $white) $fog 0.5\n", "$m")
    st, msg = _raw(fog.desc, lr.mesh_nodes(fog.desc)[0], 0, 4, 4, hits, None)
    assert st == api.RT_E_UNSUPPORTED and "volume" in msg and (hits["prim"] == 77).all(), msg
