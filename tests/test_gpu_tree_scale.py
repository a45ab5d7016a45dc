"""Device refit (rt_refit.hip behind rt_scene_update) and the device BVH builder (rt_bvh_device.hip behind
RT_SCENE_BVH_ON_DEVICE) held to the host at 131 072 triangles, the fixture of tests/tree_scale_cases.py: there k_refit_up<2>
runs 159 workgroups, k_refit_up<4> 78, k_refit_tris and k_fit_boxes 512, so a node's entries written in one workgroup are
read by the thread of another that arrives last at the parent's counter - a hand-off the 1 152-triangle grids of
tests/test_gpu_scene_update.py never perform.  No RT_WF_* or RT_BVH_* variable is set: the default plan runs, which at this
size is the headline's (slabs on every child in f64), with the spill path of k_wf_mesh (stack 28 > 12 LDS levels).

Tables are compared as digests over all their bytes and as exports (assert_same_tables); check_tree establishes on the
device's export that the tree loses no triangle.  Answers: trace_rays / occluded against a fresh scene (bytes) and the
oracle (class, material, front face exactly; t and pos at 1e-12), frames bit for bit and at assert_f64_parity.

"A fresh scene's digests" of a deformation means the host derivation on the same tree: DeviceScene(a) updated before anything
is on the device materialises through DeviceScene<R>::build.  DeviceScene(b) itself builds another tree (SAH over b's
vertices), so only its answers are compared, never its tables.  Every test prints its figures before it asserts."""
import time

import numpy as np
import pytest

from rust_raytracer_amd import api
import tree_scale_cases as tc
from test_gpu_parity import assert_f64_parity
from test_gpu_scene_update import assert_same_tables

pytestmark = pytest.mark.gpu

PRECISIONS = {"f64": api.RT_PRECISION_F64, "f32": api.RT_PRECISION_F32}
PIPELINES = {"wavefront": api.RT_PIPELINE_WAVEFRONT, "megakernel": api.RT_PIPELINE_MEGAKERNEL}


@pytest.fixture(scope="module", autouse=True)
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def digests(scene, f32):
    return dict(zip(tc.DIGESTS, scene.debug_mesh_digest(f32)[:7]))


def assert_same_digests(got, want, what):
    differ = [name for name in tc.DIGESTS if got[name] != want[name]]
    print(f"{what}: " + ", ".join(f"{name} {got[name]:016x}" for name in tc.DIGESTS))
    assert not differ, f"{what}: tables {differ} differ"


def host_derived(case, f32, flagged=False):
    """Digests of the base tree carrying `case`, derived on the host: updated before anything was on the device."""
    def make():
        a = tc.host_scene("base")
        scene = tc.flagged_scene(a) if flagged else api.DeviceScene(a.desc, 0)
        if case != "base":
            info = scene.update(tc.host_scene(case).desc)
            assert info["n_meshes_refit"] == 1 and info["refit_kernel_ms"] == 0.0
        out = digests(scene, f32)
        scene.close()
        return out
    return cached(("host_derived", case, f32, flagged), make)


def checked(t, what):
    slack = tc.check_tree(t["children"], t["boxes"], t["tris"], t["order"], tc.N_TRIS)
    print(f"{what}: check_tree passes on {len(t['children'])} nodes, largest slack {slack:.4g} object units")
    return slack


def refitted(case, precs=("f64", "f32")):
    """DeviceScene(base) with `precs` on the device, then updated to `case` by the kernels."""
    scene = api.DeviceScene(tc.host_scene("base").desc, 0)
    for prec in precs:
        scene.debug_mesh_digest(prec == "f32")
    info = scene.update(tc.host_scene(case).desc)
    assert info["n_meshes_refit"] == 1 and info["n_triangles_refit"] == tc.N_TRIS and info["refit_kernel_ms"] > 0
    return scene


def answers(scene, rays, prec):
    return scene.trace_rays(rays.o, rays.d, PRECISIONS[prec]), scene.occluded(rays.seg_o, rays.seg_d, tc.T_MIN, tc.T_MAX, PRECISIONS[prec])


def frame(scene, hs, prec, pipe):
    p = hs.params.copy()
    p.precision, p.pipeline = PRECISIONS[prec], PIPELINES[pipe]
    out = scene.render(hs.camera, p)
    assert scene.stats().pipeline_used == PIPELINES[pipe]
    return out


def fresh(case, what, prec=None, pipe=None):
    """Answers ("rays": (hits, occluded) per precision) or one frame of a fresh host-built DeviceScene(case)."""
    def make():
        hs = tc.host_scene(case)
        scene = api.DeviceScene(hs.desc, 0)
        try:
            if what == "rays":
                return {p: answers(scene, tc.ray_sets(case), p) for p in PRECISIONS}
            return frame(scene, hs, prec, pipe)
        finally:
            scene.close()
    return cached(("fresh", case, what, prec, pipe), make)


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def rays_differing(a, b):
    return np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))


# ---- R1: refit tables ----
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", tc.DEFORMATIONS)
def test_refit_tables(case, f32):
    a, b = tc.host_scene("base"), tc.host_scene(case)
    scene = api.DeviceScene(a.desc, 0)
    # this precision is on the device from here on, so the update runs the kernels; a fresh scene holds the builder's tables
    assert_same_tables(scene.debug_mesh(0, f32), cached(("host export", f32), lambda: api.scene_refit_mesh(a.desc, a.desc, 0, f32)))
    info = scene.update(b.desc)
    print(f"{case} {'f32' if f32 else 'f64'}: {info}")
    by_kernels = digests(scene, f32)
    exported = scene.debug_mesh(0, f32)
    scene.close()
    if case == "smooth" and not f32:                 # one observation for DESIGN.md section 13, no benchmark
        t0 = time.perf_counter()
        other = api.DeviceScene(b.desc, 0)
        t1 = time.perf_counter()
        other.debug_mesh_digest(f32)
        t2 = time.perf_counter()
        other.close()
        print(f"timing, measured once: refit_kernel_ms {info['refit_kernel_ms']:.3f}, update total_ms {info['total_ms']:.3f}; "
              f"DeviceScene(b) creation {1e3 * (t1 - t0):.1f} ms wall, its f64 tables on the device {1e3 * (t2 - t1):.1f} ms more")
    assert info["n_meshes_refit"] == 1 and info["n_triangles_refit"] == 131072 and info["refit_kernel_ms"] > 0
    assert_same_digests(by_kernels, host_derived(case, f32), f"{case}: kernels vs host derivation")
    assert_same_tables(exported, api.scene_refit_mesh(a.desc, b.desc, 0, f32))
    checked(exported, f"{case} refitted on the device")


# ---- R2: no drift ----
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_refit_no_drift(f32):
    """a -> smooth -> a -> weld on one scene: arrival counters left over from an earlier update would serve a node early."""
    scene = api.DeviceScene(tc.host_scene("base").desc, 0)
    scene.debug_mesh_digest(f32)
    got = {}
    for step, case in enumerate(("smooth", "base", "weld"), start=2):
        info = scene.update(tc.host_scene(case).desc)
        assert info["n_meshes_refit"] == 1 and info["refit_kernel_ms"] > 0
        got[step] = digests(scene, f32)
    scene.close()
    assert_same_digests(got[3], host_derived("base", f32), "a -> smooth -> a vs a fresh scene of a")
    assert_same_digests(got[4], host_derived("weld", f32), "a -> smooth -> a -> weld vs weld derived on the host")
    assert_same_digests(got[2], host_derived("smooth", f32), "a -> smooth vs smooth derived on the host")


# ---- R3: answers ----
@pytest.mark.parametrize("case", ["smooth", "weld"])
def test_refit_ray_answers(case):
    rays = tc.ray_sets(case)
    scene = refitted(case)
    got = {prec: answers(scene, rays, prec) for prec in PRECISIONS}
    scene.close()
    want = fresh(case, "rays")
    for prec in PRECISIONS:
        differ = rays_differing(got[prec][0], want[prec][0])
        print(f"{case} {prec}: {len(rays.o)} rays, {len(differ)} differ from the fresh scene's bytes {differ[:5]}, "
              f"{int((got[prec][1] != want[prec][1]).sum())} of {len(rays.seg_o)} occlusion flags differ")
    for prec in PRECISIONS:
        assert same_bytes(got[prec][0], want[prec][0]), f"{prec}: trace_rays, refitted vs fresh"
        np.testing.assert_array_equal(got[prec][1], want[prec][1], err_msg=f"{prec}: occluded, refitted vs fresh")
    tc.assert_answers_equal_oracle(got["f64"][0], rays.hits)
    np.testing.assert_array_equal(got["f64"][1], rays.seg_occluded)


@pytest.mark.parametrize("pipe", sorted(PIPELINES))
@pytest.mark.parametrize("case", ["smooth", "weld"])
def test_refit_frames(case, pipe):
    hs = tc.host_scene(case)
    scene = refitted(case)
    got = {prec: frame(scene, hs, prec, pipe) for prec in PRECISIONS}
    scene.close()
    for prec in PRECISIONS:
        want = fresh(case, "frame", prec, pipe)
        n = int((got[prec].view(np.uint64) != want.view(np.uint64)).any(axis=2).sum())
        print(f"{case} {pipe} {prec}: {n} pixels differ from the fresh scene's frame")
        assert n == 0 and got[prec].shape == want.shape
    assert_f64_parity(got["f64"], tc.oracle_frame(case))


# ---- B1: the device builder ----
def test_device_builder_tables():
    a = tc.host_scene("base")
    for prec in PRECISIONS:
        f32 = prec == "f32"
        first, second = tc.flagged_scene(a), tc.flagged_scene(a)
        d1, d2 = digests(first, f32), digests(second, f32)
        exported = first.debug_mesh(0, f32)
        first.close()
        second.close()
        assert_same_digests(d1, d2, f"device-built {prec}: two creations")
        print(f"device-built {prec}: worst-case stack {tc.worst_stack(exported['children'])}")
        checked(exported, f"device-built {prec}")
        assert d1 != host_derived("base", f32)        # another tree than the host's


def compare_with_host_built(got, want, what):
    """The device-built tree against the host-built one on the same rays: what a hit is may differ only in which of tied
    triangles it names (include/rt_mi355.h: two triangles at exactly equal t: either)."""
    other = got["prim"] != want["prim"]
    print(f"{what}: {int(other.sum())} of {len(got)} rays name another prim than the host-built tree")
    for f in ("t", "pos", "material", "node", "flags"):
        assert same_bytes(np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])), f"{what}: {f}"
    for f in ("normal", "u", "v"):
        assert same_bytes(np.ascontiguousarray(got[f][~other]), np.ascontiguousarray(want[f][~other])), f"{what}: {f} where prim is equal"


def test_device_builder_answers():
    a, rays = tc.host_scene("base"), tc.ray_sets("base")
    scene = tc.flagged_scene(a)
    levels = tc.worst_stack(scene.debug_mesh(0, False)["children"]) + 1
    # rt_scene_mesh_stats compiles with the host builder whatever the description's flag: its figure is the host tree's.  What
    # the library decides by is the tree it holds, so the branch below reads the stack off the device's export.
    a.desc.contents.flags |= api.RT_SCENE_BVH_ON_DEVICE
    try:
        stats_levels = api.scene_mesh_stats(a.desc)["bvh4_stack"] + 1
    finally:
        a.desc.contents.flags &= ~api.RT_SCENE_BVH_ON_DEVICE
    print(f"device-built tree: {levels} stack levels (scene_mesh_stats of the flagged description: {stats_levels})")
    want = fresh("base", "rays")
    try:
        for prec in PRECISIONS:
            got = scene.trace_rays(rays.o, rays.d, PRECISIONS[prec])
            compare_with_host_built(got, want[prec][0], f"trace_rays {prec}")
            if prec == "f64":
                tc.assert_answers_equal_oracle(got, rays.hits)
        if levels <= 64:
            print("occlusion: the device-built tree fits the kernel's stack, flags compared with the oracle's")
            for prec in PRECISIONS:
                seg = scene.occluded(rays.seg_o, rays.seg_d, tc.T_MIN, tc.T_MAX, PRECISIONS[prec])
                np.testing.assert_array_equal(seg, want[prec][1], err_msg=f"{prec}: occluded, device-built vs host-built")
                if prec == "f64":
                    np.testing.assert_array_equal(seg, rays.seg_occluded)
        else:
            print("occlusion: the device-built tree is deeper than the kernel's stack, RT_E_UNSUPPORTED expected")
            with pytest.raises(api.RtError) as e:
                scene.occluded(rays.seg_o, rays.seg_d, tc.T_MIN, tc.T_MAX)
            assert e.value.status == api.RT_E_UNSUPPORTED and "mesh BVH too deep for the occlusion kernel's LDS traversal stack" in str(e.value)
    finally:
        scene.close()


@pytest.mark.parametrize("pipe", sorted(PIPELINES))
def test_device_builder_frame(pipe):
    a = tc.host_scene("base")
    scene = tc.flagged_scene(a)
    got = frame(scene, a, "f64", pipe)
    scene.close()
    print(f"device-built {pipe}: {int((got.view(np.uint64) != fresh('base', 'frame', 'f64', pipe).view(np.uint64)).any(axis=2).sum())} pixels differ from the host-built tree's frame")
    assert_f64_parity(got, tc.oracle_frame("base"))


# ---- B2: a device-built tree, then refitted ----
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_device_built_then_refitted(f32):
    a, b, rays = tc.host_scene("base"), tc.host_scene("smooth"), tc.ray_sets("smooth")
    prec = "f32" if f32 else "f64"
    scene = tc.flagged_scene(a)
    scene.debug_mesh_digest(f32)
    info = scene.update(b.desc)
    print(f"device-built, then smooth, {prec}: {info}")
    try:
        assert info["n_meshes_refit"] == 1 and info["n_triangles_refit"] == tc.N_TRIS and info["refit_kernel_ms"] > 0
        assert_same_digests(digests(scene, f32), host_derived("smooth", f32, flagged=True), f"device-built, refitted by kernels vs on the host, {prec}")
        checked(scene.debug_mesh(0, f32), f"device-built, refitted, {prec}")
        got = scene.trace_rays(rays.o, rays.d, PRECISIONS[prec])
        compare_with_host_built(got, fresh("smooth", "rays")[prec][0], f"trace_rays {prec}")
        if not f32:
            tc.assert_answers_equal_oracle(got, rays.hits)
            assert_f64_parity(frame(scene, b, "f64", "wavefront"), tc.oracle_frame("smooth"))
    finally:
        scene.close()
