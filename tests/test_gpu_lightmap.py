"""Lightmaps on the GPU (rt_lightmap_texels, rt_lightmap_dilate, rt_bake_lightmap): the device
rasteriser against both references - the numpy rule of tests/lightmap_ref.py and the library's own brute force
(rt_lightmap_texels_desc) - on the smallest inputs where each mechanism can fail: the tie and min-index rules and partial
tiles (cube), a real atlas under one and two transforms (monkey), a tile list longer than one LDS batch, box edges on tile
borders, clipping, faces that cover nothing, overlapping charts and the fill order of the atomics (crafted), cracks (grid),
the records against rt_trace_rays (octahedron), rt_scene_update, dilation, the bake in one call, and every refusal.

prim, count and flags must be equal; pos, normal, u and v within 1e-12 * max(1, scene extent), the project's f64 bar."""
import os

import numpy as np
import pytest

import lightmap_ref as lr
from rust_raytracer_amd import api

pytestmark = pytest.mark.gpu

HIT = api.RT_RAY_HIT


@pytest.fixture(scope="module", autouse=True)
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


_scenes = {}


def device_scene(name):
    """One DeviceScene per shared scene for the whole module (a rasterisation leaves a scene as it was)."""
    if name not in _scenes:
        _scenes[name] = api.DeviceScene(lr.host_scene(name).desc, 0)
    return _scenes[name]


def node_of(name):
    return lr.mesh_nodes(lr.host_scene(name).desc)[0]


def check_both(name, w, h):
    """Device records and counts of the first mesh of `name` against the numpy rule and the host brute force."""
    got, count = device_scene(name).lightmap_texels(node_of(name), w, h, counts=True)
    ref, ref_count, mesh = lr.reference(name, w, h)
    print(f"{name} {w} x {h} against the numpy rule:")
    lr.compare(got, count, ref, ref_count, mesh.tol)
    host, host_count = api.lightmap_texels_desc(lr.host_scene(name).desc, node_of(name), w, h, counts=True)
    print(f"{name} {w} x {h} against rt_lightmap_texels_desc:")
    lr.compare(got, count, host, host_count, mesh.tol)
    return got, count


@pytest.mark.parametrize("w,h", [(16, 16), (37, 21), (1, 1)])
def test_cube_ties_min_index_and_partial_tiles(w, h):
    """Every face of the cube maps onto the whole square as two triangles that share the diagonal u = v: one triangle of each
    face covers a centre off the diagonal (count 6), all twelve a centre exactly on it (x == y at 16 x 16), which goes to
    triangle 0; prim is 0 or 1 everywhere."""
    got, count = check_both("cube", w, h)
    assert set(np.unique(got["prim"])) <= {0, 1} and (got["flags"] == lr.HIT_FRONT).all()
    y, x = np.mgrid[0:h, 0:w]
    on_diagonal = (2 * x + 1) * h == (2 * y + 1) * w
    assert (count[~on_diagonal] == 6).all() and (count[on_diagonal] == 12).all() and (got["prim"][on_diagonal] == 0).all()
    if (w, h) == (16, 16):
        assert np.array_equal(on_diagonal, x == y)


@pytest.mark.parametrize("name", ["monkey1", "monkey2"])
@pytest.mark.parametrize("w,h", [(128, 128), (100, 60)])
def test_monkey_atlas(name, w, h):
    got, count = check_both(name, w, h)
    share = float((count > 0).mean())
    assert 0.5 < share < 0.8, share   # the atlas covers 0.688 of the square
    st = device_scene(name).lightmap_stats()
    assert (st.width, st.height, st.texels) == (w, h, w * h) and st.covered_texels == int((count > 0).sum())
    assert st.tile_refs >= 967 and st.raster_ms > 0 and st.bin_ms > 0


def test_monkey_without_a_transform_and_flat_shading():
    check_both("monkey0", 33, 47)
    hs = lr.new_host_scene("monkey1_flat_gpu", lr.MONKEY1_BODY.format(obj=lr._rel(lr.MONKEY)), "$m")
    hs.desc.contents.meshes[0].flags |= api.RT_MESH_FLAT_SHADING
    node = lr.mesh_nodes(hs.desc)[0]
    mesh = lr.Mesh(hs.desc, node)
    ref, ref_count = lr.rasterise(mesh, 100, 60)
    scene = api.DeviceScene(hs.desc, 0)
    got, count = scene.lightmap_texels(node, 100, 60, counts=True)
    scene.close()
    lr.compare(got, count, ref, ref_count, mesh.tol)
    assert np.abs(ref["normal"] - lr.reference("monkey1", 100, 60)[0]["normal"]).max() > 1e-3


@pytest.mark.parametrize("w,h", [(64, 64), (48, 80)])
def test_crafted_mesh_twice(w, h):
    """A tile list longer than one LDS batch, box edges on tile borders, vertices on texel centres, clipping at 0 and 1, faces
    that cover nothing, overlapping charts; twice in one process, byte for byte: the fill order of the atomics must not show."""
    got, count = check_both("crafted", w, h)
    again, count_again = device_scene("crafted").lightmap_texels(node_of("crafted"), w, h, counts=True)
    assert got.tobytes() == again.tobytes() and count.tobytes() == count_again.tobytes()
    assert device_scene("crafted").lightmap_stats().tile_refs > 300


def test_no_cracks():
    got, count = check_both("grid", 64, 64)
    inside, clear, outside = lr.grid_masks(64, 64)
    assert (count[inside] >= 1).all(), "a crack: an inside centre that no triangle covers"
    assert (count[clear] == 1).all() and (count[outside] == 0).all()
    assert ((got["flags"] & HIT) != 0)[inside].all()


def test_records_against_trace_rays():
    """On a convex mesh nothing can lie in front: for every covered texel with count == 1 the ray from pos + n d along -n (n: the
    triangle's geometric normal on the record's side, d = 1e-3 of the extent) reports the same prim, node and material and a
    position within 1e-9 * extent."""
    w, h = 64, 32
    got, count = check_both("octahedron", w, h)
    rec, _, mesh = lr.reference("octahedron", w, h)
    pick = (count == 1) & ((got["flags"] & HIT) != 0)
    assert pick.sum() > 300
    r = got[pick]
    world = mesh.positions
    for m4 in mesh.chain:
        world = lr._apply(m4, world, 1.0)
    p0, p1, p2 = (world[mesh.tri_pos[r["prim"], k]] for k in range(3))
    n = lr._unit(np.cross(p1 - p0, p2 - p0))
    n = np.where((n * r["normal"]).sum(axis=1)[:, None] < 0, -n, n)
    d = 1e-3 * mesh.extent
    hits = device_scene("octahedron").trace_rays(r["pos"] + n * d, -n)
    assert np.array_equal(hits["prim"], r["prim"]) and np.array_equal(hits["node"], r["node"]) and np.array_equal(hits["material"], r["material"])
    err = float(np.abs(hits["pos"] - r["pos"]).max())
    print(f"position of the ray's hit against the record: max |difference| {err:.3e} (bar {1e-9 * mesh.extent:.3e})")
    assert err <= 1e-9 * mesh.extent


def test_after_scene_update():
    """A scene moved by rt_scene_update rasterises its new vertices: byte-identical to a freshly created scene, different from
    before."""
    w, h = 100, 60
    before_hs = lr.new_host_scene("update_a", lr.MONKEY1_BODY.format(obj=lr._rel(lr.MONKEY)), "$m")
    moved = lr.moved_obj(lr.MONKEY, "monkey_moved.obj")
    after_hs = lr.new_host_scene("update_b", lr.MONKEY1_BODY.format(obj=lr._rel(moved)), "$m")
    node = lr.mesh_nodes(before_hs.desc)[0]
    scene = api.DeviceScene(before_hs.desc, 0)
    before, before_count = scene.lightmap_texels(node, w, h, counts=True)
    info = scene.update(after_hs.desc)
    assert info["n_meshes_refit"] == 1
    after, after_count = scene.lightmap_texels(node, w, h, counts=True)
    fresh_scene = api.DeviceScene(after_hs.desc, 0)
    fresh, fresh_count = fresh_scene.lightmap_texels(node, w, h, counts=True)
    scene.close()
    fresh_scene.close()
    assert after.tobytes() == fresh.tobytes() and after_count.tobytes() == fresh_count.tobytes()
    assert before.tobytes() != after.tobytes()
    mesh = lr.Mesh(after_hs.desc, node)
    ref, ref_count = lr.rasterise(mesh, w, h)
    lr.compare(after, after_count, ref, ref_count, mesh.tol)


def _masks(h, w):
    y, x = np.mgrid[0:h, 0:w]
    one = np.zeros((h, w), dtype=np.uint8)
    one[h // 2, w // 2] = 1
    corner = np.zeros((h, w), dtype=np.uint8)
    corner[0, 0] = 1
    return {"empty": np.zeros((h, w), dtype=np.uint8), "full": np.ones((h, w), dtype=np.uint8), "isolated": one,
            "checkerboard": ((x + y) % 2).astype(np.uint8) * 255, "corner": corner}


@pytest.mark.parametrize("h,w", [(21, 37), (9, 1)])
@pytest.mark.parametrize("passes", [0, 1, 3])
def test_dilation(h, w, passes):
    rng = np.random.default_rng(17)
    for name, mask in _masks(h, w).items():
        img = rng.normal(size=(h, w, 4))   # uncovered texels hold numbers too: they must not be read
        ref, ref_cov = lr.dilate(img, mask, passes)
        got, got_cov = api.lightmap_dilate(img, mask, passes)
        assert np.array_equal(got_cov, ref_cov), name
        assert got.tobytes() == ref.tobytes(), name


def _params(hs, s, t):
    p = type(hs.params).from_buffer_copy(hs.params)
    p.sqrt_spt, p.thread_count = s, t
    return p


@pytest.mark.parametrize("kind", ["irradiance", "visibility"])
def test_bake_lightmap(kind):
    """rt_bake_lightmap at 32 x 32, S = 2, T = 1: the coverage is the rasterisation's; before dilation every covered texel equals
    the host variant of the bake on the records' pos and normal at the same index, bit for bit (a point's answer depends on
    its index and inputs alone), every other texel is 0; the final image is the numpy dilation of that."""
    w = h = 32
    hs, scene, node = lr.host_scene("two"), device_scene("two"), node_of("two")
    rec = scene.lightmap_texels(node, w, h)
    covered = (rec["flags"] & HIT) != 0
    assert 100 < covered.sum() < w * h
    pos, nrm = rec["pos"].reshape(-1, 3), rec["normal"].reshape(-1, 3)
    if kind == "irradiance":
        params = _params(hs, 2, 1)
        want = scene.bake_irradiance(np.where(covered.reshape(-1, 1), pos, 0.0), np.where(covered.reshape(-1, 1), nrm, [0.0, 1.0, 0.0]), params)
        want = want.reshape(h, w, 4)
    else:
        params = api.RtBakeParams.defaults(samples=16, seed=3)
        vis = scene.bake_visibility(np.where(covered.reshape(-1, 1), pos, 0.0), np.where(covered.reshape(-1, 1), nrm, [0.0, 1.0, 0.0]), samples=16, seed=3)
        want = np.zeros((h, w, 4))
        want[..., :3] = vis["visibility"].reshape(h, w, 1)
    want = np.where(covered[..., None], want, 0.0)
    raw, cov = scene.bake_lightmap(node, w, h, params, kind=kind, dilate=0)
    assert np.array_equal(cov != 0, covered)
    assert raw.tobytes() == want.tobytes()
    assert np.abs(raw[covered][:, :3]).max() > 0
    for passes in (1, 2):
        final, cov2 = scene.bake_lightmap(node, w, h, params, kind=kind, dilate=passes)
        ref, _ = lr.dilate(want, covered, passes)
        assert np.array_equal(cov2, cov) and final.tobytes() == ref.tobytes(), passes


def _raw_texels(scene, node, instance, w, h, hits, counts):
    st = scene._lib.rt_lightmap_texels(scene._h, node, instance, w, h, None if hits is None else hits.ctypes.data,
                                       None if counts is None else counts.ctypes.data)
    return st, scene._lib.rt_last_error().decode()


def test_refusals():
    hs, scene, node = lr.host_scene("cube"), device_scene("cube"), node_of("cube")
    d = hs.desc.contents
    scene.lightmap_texels(node, 16, 16, counts=True)   # the workspace exists from here on
    hits = np.zeros(256 * 256, dtype=api.RtRayHit)
    hits["prim"] = 77
    counts = np.full(256 * 256, 99, dtype=np.uint32)
    not_mesh = next(i for i in range(d.n_nodes) if d.nodes[i].type != 3)
    cases = [((node, 0, 0, 16), api.RT_E_INVALID, "width"), ((node, 0, 16, 0), api.RT_E_INVALID, "height"),
             ((node, 0, 16385, 16), api.RT_E_INVALID, "width"), ((node, 0, 16, 16385), api.RT_E_INVALID, "height"),
             ((d.n_nodes, 0, 16, 16), api.RT_E_INVALID, "node"), ((not_mesh, 0, 16, 16), api.RT_E_INVALID, "node"),
             ((node, 1, 16, 16), api.RT_E_INVALID, "instance")]
    for args, status, word in cases:
        live = api.live_resources()
        st, msg = _raw_texels(scene, *args, hits, counts)
        assert st == status and word in msg and msg.startswith("rt_lightmap_texels:"), (args, st, msg)
        assert (hits["prim"] == 77).all() and (counts == 99).all() and api.live_resources() == live
    live = api.live_resources()
    st, msg = _raw_texels(scene, node, 0, 16, 16, None, counts)
    assert st == api.RT_E_INVALID and "hits_out" in msg and (counts == 99).all() and api.live_resources() == live
    # the reference cap: 12 triangles over all 256 tiles of a 256 x 256 map
    os.environ["RT_LIGHTMAP_MAX_REFS"] = "300"
    try:
        st, msg = _raw_texels(scene, node, 0, 256, 256, hits, counts)
    finally:
        del os.environ["RT_LIGHTMAP_MAX_REFS"]
    assert st == api.RT_E_UNSUPPORTED and "3072" in msg and "300" in msg and "RT_LIGHTMAP_MAX_REFS" in msg, msg
    assert (hits["prim"] == 77).all() and (counts == 99).all() and api.live_resources() == live
    st, msg = _raw_texels(scene, node, 0, 256, 256, hits, counts)   # read at each call: allowed again
    assert st == api.RT_OK and (hits["prim"] != 77).all() and (counts != 99).all()


def _raw_bake(scene, node, instance, w, h, kind, rp, bp, passes, rgba, cov):
    import ctypes as C
    st = scene._lib.rt_bake_lightmap(scene._h, node, instance, w, h, kind, None if rp is None else C.byref(rp), None if bp is None else C.byref(bp),
                                     passes, None if rgba is None else rgba.ctypes.data, None if cov is None else cov.ctypes.data)
    return st, scene._lib.rt_last_error().decode()


def test_bake_and_dilate_refusals():
    hs, scene, node = lr.host_scene("two"), device_scene("two"), node_of("two")
    scene.bake_lightmap(node, 16, 16, _params(hs, 1, 1), dilate=2)   # the workspace exists from here on
    rgba = np.full((16, 16, 4), 5.0)
    cov = np.full((16, 16), 9, dtype=np.uint8)
    good = _params(hs, 1, 1)
    depth0, mega, zero_s = _params(hs, 1, 1), _params(hs, 1, 1), _params(hs, 0, 1)
    depth0.max_depth = 0
    mega.pipeline = api.RT_PIPELINE_MEGAKERNEL
    bad_samples = api.RtBakeParams.defaults(samples=0)
    cases = [((node, 0, 16, 16, 2, good, None, 2), api.RT_E_INVALID, "kind"), ((node, 0, 16, 16, 0, good, None, -1), api.RT_E_INVALID, "dilate_passes"),
             ((node, 0, 0, 16, 0, good, None, 2), api.RT_E_INVALID, "width"), ((node, 7, 16, 16, 0, good, None, 2), api.RT_E_INVALID, "instance"),
             ((node, 0, 16, 16, 0, None, None, 2), api.RT_E_INVALID, "params"), ((node, 0, 16, 16, 0, zero_s, None, 2), api.RT_E_INVALID, "sqrt_spt"),
             ((node, 0, 16, 16, 0, depth0, None, 2), api.RT_E_UNSUPPORTED, "max_depth"), ((node, 0, 16, 16, 0, mega, None, 2), api.RT_E_UNSUPPORTED, "MEGAKERNEL"),
             ((node, 0, 16, 16, 1, None, bad_samples, 2), api.RT_E_INVALID, "samples")]
    for args, status, word in cases:
        live = api.live_resources()
        st, msg = _raw_bake(scene, *args, rgba, cov)
        assert st == status and word in msg, (args[:5], st, msg)
        assert (rgba == 5.0).all() and (cov == 9).all() and api.live_resources() == live, msg
    for out in ((None, cov), (rgba, None)):
        st, msg = _raw_bake(scene, node, 0, 16, 16, 0, good, None, 2, *out)
        assert st == api.RT_E_INVALID and "NULL" in msg
    # dilation by itself
    lib = scene._lib
    img, c = np.zeros((4, 4, 4)), np.zeros((4, 4), dtype=np.uint8)
    for args, word in (((img.ctypes.data, c.ctypes.data, 4, 4, -1, rgba.ctypes.data, cov.ctypes.data), "passes"),
                       ((None, c.ctypes.data, 4, 4, 1, rgba.ctypes.data, cov.ctypes.data), "rgba"),
                       ((img.ctypes.data, None, 4, 4, 1, rgba.ctypes.data, cov.ctypes.data), "coverage"),
                       ((img.ctypes.data, c.ctypes.data, 0, 4, 1, rgba.ctypes.data, cov.ctypes.data), "w "),
                       ((img.ctypes.data, c.ctypes.data, 4, 16385, 1, rgba.ctypes.data, cov.ctypes.data), "h ")):
        live = api.live_resources()
        st = lib.rt_lightmap_dilate(0, *args)
        msg = lib.rt_last_error().decode()
        assert st == api.RT_E_INVALID and word in msg, msg
        assert (rgba == 5.0).all() and (cov == 9).all() and api.live_resources() == live


def test_refuses_meshes_without_uvs_volume_boundaries_and_volumes():
    obj = lr.write_obj("no_vt_gpu.obj", [(0, 0, 0), (1, 0, 0), (0, 1, 0)], [], [(0, 0, 1)], [[(1, None, 1), (2, None, 1), (3, None, 1)]])
    plain = lr.new_host_scene("no_vt_gpu", f"m: mesh {lr._rel(obj)} $white\n", "$m")
    fog = lr.new_host_scene("fog_gpu", f"fog: isotropic (constant 0.9,0.9,1)\nm: volume (mesh {lr._rel(lr.CUBE)} $white) $fog 0.5\n"
                            f"m2: transform (mesh {lr._rel(lr.CUBE)} $white) t=3,0,0\n", "$m $m2")
    hits = np.zeros(16, dtype=api.RtRayHit)
    hits["prim"] = 77
    rgba, cov = np.full((4, 4, 4), 5.0), np.full((4, 4), 9, dtype=np.uint8)
    for hs, k, word in ((plain, 0, "uv"), (fog, 0, "volume")):
        scene = api.DeviceScene(hs.desc, 0)
        live = api.live_resources()
        st, msg = _raw_texels(scene, lr.mesh_nodes(hs.desc)[k], 0, 4, 4, hits, None)
        assert st == api.RT_E_UNSUPPORTED and word in msg and (hits["prim"] == 77).all() and api.live_resources() == live, msg
        scene.close()
    # the mesh beside the volume rasterises, but a scene with volumes has no hit-record bakes
    scene = api.DeviceScene(fog.desc, 0)
    free = lr.mesh_nodes(fog.desc)[1]
    assert ((scene.lightmap_texels(free, 8, 8)["flags"] & HIT) != 0).all()
    live = api.live_resources()
    st, msg = _raw_bake(scene, free, 0, 4, 4, 0, _params(fog, 1, 1), None, 1, rgba, cov)
    assert st == api.RT_E_UNSUPPORTED and "volumes" in msg and (rgba == 5.0).all() and (cov == 9).all() and api.live_resources() == live, msg
    scene.close()


def test_resources_come_back():
    hs, node = lr.host_scene("two"), node_of("two")
    start = api.live_resources()
    for _ in range(3):
        scene = api.DeviceScene(hs.desc, 0)
        scene.bake_lightmap(node, 24, 20, _params(hs, 1, 1), dilate=2)
        scene.bake_lightmap(node, 24, 20, None, kind="visibility", dilate=1)
        scene.lightmap_texels(node, 40, 12, counts=True)
        scene.close()
    assert api.live_resources() == start


def test_rtrace_lightmap_writes_the_map(tmp_path):
    """rtrace --lightmap writes out_lightmap.png (and no frame): what rt_bake_lightmap gives for the same mesh op, through the
    output stage of out.png."""
    import subprocess
    scene_path = lr.scene_text("two_cli", "floor: plane 0,0,0 5,0,0 0,0,-5 $white\n" + lr.MONKEY1_BODY.format(obj=lr._rel(lr.MONKEY)) +
                               f"m2: transform (mesh {lr._rel(lr.CUBE)} (lambertian (constant 0.2,0.5,0.8))) s=0.5 ry=-40 t=1.2,0.5,0.3\n", "$floor $m $m2")
    args = [scene_path, "-w=32", "-s=4", "--seed=5", "--lightmap=1:24x16:1"]
    rtrace = os.path.join(str(lr.REPO), "rust_raytracer_amd", "rtrace")
    r = subprocess.run([rtrace] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out_lightmap.png").exists() and not (tmp_path / "out.png").exists()
    assert "Lightmap of mesh 1" in r.stdout and "24x16 texels, 384 covered" in r.stdout   # the cube's faces cover the whole square
    hs = api.HostScene(args)
    scene = api.DeviceScene(hs.desc, 0)
    rgba, cov = scene.bake_lightmap(lr.mesh_nodes(hs.desc)[1], 24, 16, hs.params, dilate=1)
    scene.close()
    assert cov.all()
    lib = api.load_host_lib()
    png = tmp_path / "check.png"
    assert lib.rth_save_png(str(png).encode(), rgba.ctypes.data, 24, 16) == 0
    assert png.read_bytes() == (tmp_path / "out_lightmap.png").read_bytes()
    r = subprocess.run([rtrace, scene_path, "-w=32", "-s=4", "--lightmap=2:16"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "there is no mesh 2" in r.stderr


def test_device_variants_on_caller_buffers():
    """The _device entry points on the caller's own HBM buffers (torch) give what the host variants give."""
    import torch
    w, h = 37, 21
    scene, node = device_scene("cube"), node_of("cube")
    want, want_count = scene.lightmap_texels(node, w, h, counts=True)
    d_hits = torch.zeros(w * h * 96, dtype=torch.uint8, device="cuda:0")
    d_counts = torch.zeros(w * h, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    scene.lightmap_texels_device(node, w, h, d_hits.data_ptr(), d_counts.data_ptr())
    assert d_hits.cpu().numpy().tobytes() == want.tobytes()
    assert d_counts.cpu().numpy().view(np.uint32).tobytes() == want_count.tobytes()
