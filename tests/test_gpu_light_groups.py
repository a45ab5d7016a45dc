"""Light groups on the GPU (rt_render_light_groups, rt_light_mix; include/rt_mi355.h).

The yardstick is exact: group frame g must equal, bit for bit, rt_render's frame of the scene in which every emitter outside
g emits zero (light_groups_ref.Zeroed edits hs.desc in place) - paths, random draws and light sampling do not depend on
emission values.  That scene is also rendered by the CPU oracle (1e-12 relative, floor 1e-15, NaN masks equal: the bar of
tests/test_gpu_parity.py).  The ordinary frame of the same call must be rt_render's bits, and the group frames must add up
to it within (S^2 + T + G + 2) 2^-52 relative.  The seeds below give finite zeroed frames on the oracle for sun_sky, smoke
and cornell; the f64 tests assert that first (a non-finite frame needs another seed, not a skip).  nested_lights has no such
seed: its one-sided lamps inside nested lists give 0/0 weights in 13-16 % of the pixels at every seed tried (74 .. 99, on the
oracle), so there the equality is held where the zeroed frame is finite - which is what the property says - and at least
80 % of the values must be."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import light_groups_ref as lgr
from oracle import pyoracle
from rust_raytracer_amd import api

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTRACE = os.path.join(REPO, "rust_raytracer_amd", "rtrace")

# -s=16 -t=4: 4 replicas of 2 x 2 strata
FRAME_SCENES = {
    "cornell": ["scenes/cornell", "-w=40", "-s=16", "-t=4", "--seed=71"],
    "light_test": ["scenes/light_test", "-w=48", "-s=16", "-t=4", "--seed=72"],          # a mesh, depth of field
    "smoke": ["tests/scenes/smoke", "-w=40", "-s=16", "-t=4", "--seed=73"],              # volumes: the combined intersect kernel
    "nested_lights": ["tests/scenes/nested_lights", "-w=40", "-s=16", "-t=4", "--seed=74"],
    "sun_sky": ["tests/scenes/sun_sky", "-w=40", "-s=16", "-t=4", "--seed=75"],
    "two_meshes": ["tests/scenes/two_meshes", "-w=40", "-s=16", "-t=4", "--seed=76"],
}
BACKGROUND = (0.25, 0.5, 0.75)
FINITE_SCENES = ("sun_sky", "smoke", "cornell_bg")  # every zeroed frame is finite at these seeds (checked on the oracle)
# property 2: (args, background colour or None = the scene's own setting)
GROUP_SCENES = {
    "nested_lights": (FRAME_SCENES["nested_lights"], None),
    "sun_sky": (FRAME_SCENES["sun_sky"], None),
    "smoke": (FRAME_SCENES["smoke"], None),
    "cornell_bg": (FRAME_SCENES["cornell"], BACKGROUND),
}


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def load(name, precision="f64", extra=()):
    args, bg = GROUP_SCENES[name] if name in GROUP_SCENES else (FRAME_SCENES[name], None)
    hs = api.HostScene(list(args) + list(extra))
    if bg is not None:
        hs.params.has_background = 1
        for k in range(3):
            hs.params.background[k] = bg[k]
    hs.params.pipeline = api.RT_PIPELINE_WAVEFRONT
    if precision == "f32":
        hs.params.precision = api.RT_PRECISION_F32
    return hs


def auto(hs):
    return api.light_groups_auto(hs.desc, 16, bool(hs.params.has_background))


def zeroed_frames(hs, groups, ids, oracle=False):
    """rt_render's (and optionally the oracle's) frame of the zeroed scene of every group in `ids`."""
    out = {}
    for g in ids:
        z = lgr.Zeroed(hs, groups, g)
        try:
            scene = api.DeviceScene(hs.desc, 0)
            frame = scene.render(hs.camera, z.params)
            scene.close()
            ref = pyoracle.render(hs.desc, hs.camera, z.params)[0] if oracle else None
        finally:
            z.restore()
        out[g] = (frame, ref)
    return out


def assert_equal_where_finite(group_frame, zeroed, what):
    fin = np.isfinite(zeroed)
    assert fin.mean() >= 0.8, what
    assert np.isfinite(group_frame[fin]).all(), what  # a group frame is non-finite only where its zeroed scene is
    same = bits(group_frame)[fin] == bits(zeroed)[fin]
    assert same.all(), f"{what}: {int((~same).sum())} of {int(fin.sum())} finite values differ"


def assert_f64_parity(gpu, ref):
    a, b = gpu[..., :3], ref[..., :3]
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    fin = ~np.isnan(b)
    err = np.abs(a[fin] - b[fin])
    bad = err > np.maximum(1e-12 * np.abs(b[fin]), 1e-15)
    assert not bad.any(), f"{bad.mean():.4%} of values differ by more than 1e-12 relative (max abs err {err.max():.3e})"
    assert np.all(gpu[..., 3] == 0.0)


# ---------------------------------------------------------------------------------------------------------------- property 1
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(FRAME_SCENES))
def test_frame_of_the_same_call_is_rt_renders(dev, name, precision):
    hs = load(name, precision)
    scene = api.DeviceScene(hs.desc, 0)
    want = scene.render(hs.camera, hs.params)
    groups = auto(hs)
    frames, frame = scene.render_light_groups(hs.camera, hs.params, groups)
    assert frames.shape == (groups.n_groups,) + want.shape
    assert bits(frame).tobytes() == bits(want).tobytes()
    assert not bits(frames[..., 3]).any()  # w = +0.0
    st = scene.stats()
    assert st.pipeline_used == api.RT_PIPELINE_WAVEFRONT and st.samples == hs.width * hs.height * 16
    # and a render after it is still the same frame (the shared per-sample buffer is not left in a state that matters)
    assert bits(scene.render(hs.camera, hs.params)).tobytes() == bits(want).tobytes()


# ---------------------------------------------------------------------------------------------------------------- property 2, 3, 4
@pytest.mark.parametrize("name", sorted(GROUP_SCENES))
def test_every_group_is_the_zeroed_scene_f64_and_the_oracle_agrees(dev, name):
    hs = load(name)
    groups = auto(hs)
    lamp_groups = sorted(set(int(x) for x in groups.table if x))
    lit = lamp_groups + ([groups.background_group] if hs.params.has_background and any(hs.params.background) else [])
    assert groups.n_groups == len(lamp_groups) + 1 + int(bool(hs.params.has_background)) and groups.n_groups >= 3
    scene = api.DeviceScene(hs.desc, 0)
    frames, frame = scene.render_light_groups(hs.camera, hs.params, groups)
    with_oracle = name in ("cornell_bg", "sun_sky")  # property 3 on two scenes (equal NaN masks: scenes with finite frames)
    zs = zeroed_frames(hs, groups, range(groups.n_groups), oracle=with_oracle)
    for g in range(groups.n_groups):
        z, ref = zs[g]
        if name in FINITE_SCENES:
            assert np.isfinite(z).all(), f"group {g}: the zeroed frame is not finite - choose another seed"
            assert bits(frames[g]).tobytes() == bits(z).tobytes(), f"{name} group {g}"
        else:
            assert_equal_where_finite(frames[g], z, f"{name} group {g}")
        if with_oracle:
            assert np.isfinite(ref).all(), f"group {g}: the oracle's zeroed frame is not finite - choose another seed"
            assert_f64_parity(frames[g], ref)
    for g in lit:
        assert np.nanmax(frames[g][..., :3]) > 0.0, f"group {g} is black: the test would show nothing"
    lgr.assert_sum_property(frames, frame, hs.params.sqrt_spt, hs.params.thread_count)


@pytest.mark.parametrize("name", sorted(GROUP_SCENES))
def test_every_group_is_the_zeroed_scene_f32(dev, name):
    hs = load(name, "f32")
    groups = auto(hs)
    scene = api.DeviceScene(hs.desc, 0)
    frames, frame = scene.render_light_groups(hs.camera, hs.params, groups)
    zs = zeroed_frames(hs, groups, range(groups.n_groups))
    for g in range(groups.n_groups):
        assert_equal_where_finite(frames[g], zs[g][0], f"{name} f32 group {g}")
    lgr.assert_sum_property(frames, frame, hs.params.sqrt_spt, hs.params.thread_count)


@pytest.mark.parametrize("mode", ["three_replica_groups", "small_pool", "no_tail_compaction"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", ["nested_lights", "smoke"])
def test_groups_do_not_depend_on_the_schedule(dev, monkeypatch, name, precision, mode):
    """Replica groups (RT_WF_SAMPLE_GB=0 with -t=3: one replica per group), a pool far smaller than the sample count, tail
    compaction off: the group frames stay the zeroed scene's bits, and the frame rt_render's."""
    hs = load(name, precision, extra=["-s=12", "-t=3"] if mode == "three_replica_groups" else [])
    groups = auto(hs)
    zs = zeroed_frames(hs, groups, range(groups.n_groups))  # rendered with the default schedule
    scene = api.DeviceScene(hs.desc, 0)
    want = scene.render(hs.camera, hs.params)
    if mode == "three_replica_groups":
        monkeypatch.setenv("RT_WF_SAMPLE_GB", "0")
    elif mode == "small_pool":
        monkeypatch.setenv("RT_WF_POOL", "1000")
    else:
        monkeypatch.setenv("RT_WF_COMPACT", "0")
    frames, frame = scene.render_light_groups(hs.camera, hs.params, groups)
    if mode == "three_replica_groups":
        assert scene.stats().n_replica_groups == 3
    assert bits(frame).tobytes() == bits(want).tobytes()
    for g in range(groups.n_groups):
        assert_equal_where_finite(frames[g], zs[g][0], f"{name} {precision} {mode} group {g}")
    lgr.assert_sum_property(frames, frame, hs.params.sqrt_spt, hs.params.thread_count)


def lerp_sky(hs):
    """Gives the sky of sun_sky an interpolated emission map (lerp of its colour and a second one): the scene then needs the
    texture-interpreter kernels, while a zeroed scene that switches the sky off does not.  Returns what must stay alive."""
    d = hs.desc.contents
    n = d.n_textures
    tex = (api.RtTexture * (n + 3))()
    C.memmove(tex, d.textures, n * C.sizeof(api.RtTexture))
    sky = [d.nodes[i].material for i in range(d.n_nodes) if d.nodes[i].type == 7][0]  # RT_NODE_SKY
    for t in (tex[n], tex[n + 1]):
        t.a = t.b = t.c = -1
    tex[n].type = api.RT_TEX_CONST_COLOR
    for k, v in enumerate((0.9, 0.5, 0.2)):
        tex[n].v[k] = v
    tex[n + 1].type = api.RT_TEX_CONST_FLOAT
    tex[n + 1].v[0] = 0.25
    tex[n + 2].type = api.RT_TEX_LERP
    tex[n + 2].a, tex[n + 2].b, tex[n + 2].c = d.materials[sky].tex_a, n, n + 1
    d.textures = C.cast(tex, type(d.textures))
    d.n_textures = n + 3
    d.materials[sky].tex_a = n + 2
    return tex


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_zeroing_may_change_the_kernel_variant(dev, precision):
    """The scene compiler reads texture TYPES, never emission values, but a zeroed scene can lose its last interpreted texture
    and with it the texture-interpreter variants of the kernels.  The group frames (interpreter variants) must still be the
    bits of the zeroed scenes (lean variants)."""
    hs = load("sun_sky", precision)
    keep = lerp_sky(hs)
    assert api.scene_info(hs.desc) & api.RT_SCENE_INFO_TEX_INTERPRETER
    groups = auto(hs)
    lean = 0
    for g in range(groups.n_groups):
        z = lgr.Zeroed(hs, groups, g)
        lean += not api.scene_info(hs.desc) & api.RT_SCENE_INFO_TEX_INTERPRETER
        z.restore()
    assert lean == groups.n_groups - 1  # every zeroed scene but the sky's own
    scene = api.DeviceScene(hs.desc, 0)
    frames, frame = scene.render_light_groups(hs.camera, hs.params, groups)
    assert bits(frame).tobytes() == bits(scene.render(hs.camera, hs.params)).tobytes()
    zs = zeroed_frames(hs, groups, range(groups.n_groups))
    for g in range(groups.n_groups):
        assert np.isfinite(zs[g][0]).all()
        assert bits(frames[g]).tobytes() == bits(zs[g][0]).tobytes(), f"group {g}"
    assert all(np.nanmax(frames[g][..., :3]) > 0 for g in (1, 2))
    del keep


def test_hand_made_assignment(dev):
    """Two lamps share a group, the unlit group is not 0, and a group nothing uses is +0.0 everywhere."""
    hs = load("nested_lights")
    d = hs.desc.contents
    lamps = [i for i in range(d.n_materials) if d.materials[i].type == api.RT_MAT_EMISSIVE]
    assert len(lamps) == 4
    table = np.full(d.n_materials, 3, dtype=np.uint8)  # scattering materials: never read (their paths end in the unlit group)
    table[lamps[0]] = table[lamps[1]] = 1
    table[lamps[2]] = 2
    table[lamps[3]] = 3
    groups = api.RtLightGroups.make(6, table, background_group=4, unlit_group=5)
    scene = api.DeviceScene(hs.desc, 0)
    frames, frame = scene.render_light_groups(hs.camera, hs.params, groups)
    assert not bits(frames[0]).any()  # unused: +0.0, not -0.0
    # the zeroed scenes: Zeroed looks at the Emissive materials' entries and the background only
    zs = zeroed_frames(hs, groups, range(1, 6))
    for g in range(1, 6):
        assert_equal_where_finite(frames[g], zs[g][0], f"group {g}")
    assert np.nanmax(frames[1][..., :3]) > 0 and np.nanmax(frames[3][..., :3]) > 0
    assert not frames[5][np.isfinite(frames[5])].any()  # black terminals are black (or not finite: 0/0 weights end there)
    lgr.assert_sum_property(frames, frame, hs.params.sqrt_spt, hs.params.thread_count)
    # the shared group is the sum of what the two lamps give on their own (same paths, disjoint samples), to rounding
    auto_frames, _ = scene.render_light_groups(hs.camera, hs.params, auto(hs))
    both = auto_frames[1] + auto_frames[2]
    np.testing.assert_array_equal(np.isfinite(frames[1]), np.isfinite(both))
    both, shared = np.nan_to_num(both, nan=0.0, posinf=0.0), np.nan_to_num(frames[1], nan=0.0, posinf=0.0)
    # each side carries at most S^2 + T roundings of 2^-53 (ordered sums, one division, one more addition on the right)
    np.testing.assert_allclose(shared, both, rtol=(4 + 4) * lgr.EPS, atol=0)


def test_row_partition(dev):
    hs = load("nested_lights")
    groups = auto(hs)
    scene = api.DeviceScene(hs.desc, 0)
    whole, whole_frame = scene.render_light_groups(hs.camera, hs.params, groups)
    seen = 0
    for part in range(3):
        p = hs.params.copy()
        p.band_rows, p.n_parts, p.part = 4, 3, part
        rows = api.owned_rows(hs.height, p)
        frames, frame = scene.render_light_groups(hs.camera, p, groups)
        assert frames.shape == (groups.n_groups, len(rows), hs.width, 4)
        assert bits(frames).tobytes() == bits(whole[:, rows]).tobytes()
        assert bits(frame).tobytes() == bits(whole_frame[rows]).tobytes()
        seen += len(rows)
    assert seen == hs.height


# ---------------------------------------------------------------------------------------------------------------- mix
def test_mix_is_the_numpy_restatement(dev):
    hs = load("sun_sky")
    groups = auto(hs)
    scene = api.DeviceScene(hs.desc, 0)
    frames, frame = scene.render_light_groups(hs.camera, hs.params, groups)
    rng = np.random.default_rng(9)
    tints = rng.random((groups.n_groups, 3)) * 3.0
    tints[1] = 0.0
    tints[2, 1] = -0.5
    assert bits(api.light_mix(frames, tints)).tobytes() == bits(lgr.mix(frames, tints)).tobytes()
    ones = api.light_mix(frames, np.ones(groups.n_groups))
    assert bits(ones).tobytes() == bits(lgr.mix(frames, np.ones(groups.n_groups))).tobytes()
    # every tint 1: the sum in group order (1 * x is x), so property 4 holds for the mixed frame
    assert bits(ones[..., :3]).tobytes() == bits(lgr.sum_in_group_order(frames[..., :3])).tobytes()
    fin = np.isfinite(frame[..., :3])
    assert (np.abs(ones[..., :3][fin] - frame[..., :3][fin]) <= lgr.sum_bound(hs.params.sqrt_spt, hs.params.thread_count, groups.n_groups) * frame[..., :3][fin]).all()
    # a synthetic non-finite pixel that one group alone holds leaves with that group's tint of 0
    broken = frames.copy()
    broken[2, 3, 4, 0] = np.nan
    broken[2, 5, 6, 1] = np.inf
    t = np.ones(groups.n_groups)
    assert not np.isfinite(api.light_mix(broken, t)[3, 4, 0])
    t[2] = 0.0
    out = api.light_mix(broken, t)
    assert np.isfinite(out).all() and bits(out).tobytes() == bits(lgr.mix(broken, t)).tobytes()
    with pytest.raises(api.RtError):
        api.light_mix(np.zeros((17, 2, 2, 4)), np.ones(17))


def test_tint_zero_removes_a_non_finite_pixel_of_one_group(dev):
    """zero_weight_nan renders NaN pixels (0/0 weights behind a one-sided light).  Where exactly one group holds a pixel's
    non-finite values, switching that group off leaves a finite pixel.  Skipped (stated here) only if no scene pixel is of
    that kind; the synthetic case in test_mix_is_the_numpy_restatement is unconditional."""
    hs = api.HostScene(["tests/scenes/zero_weight_nan", "-w=48", "-s=16", "-t=4", "--seed=18"])
    hs.params.pipeline = api.RT_PIPELINE_WAVEFRONT
    groups = auto(hs)
    scene = api.DeviceScene(hs.desc, 0)
    frames, frame = scene.render_light_groups(hs.camera, hs.params, groups)
    assert bits(frame).tobytes() == bits(scene.render(hs.camera, hs.params)).tobytes()
    bad = ~np.isfinite(frames[..., :3]).all(axis=-1)  # [G, H, W]
    np.testing.assert_array_equal(bad.any(axis=0), ~np.isfinite(frame[..., :3]).all(axis=-1))
    only_one = bad.sum(axis=0) == 1
    if not only_one.any():
        pytest.skip("no pixel of zero_weight_nan is non-finite in exactly one light group")
    g = int(np.argmax(bad[:, only_one].sum(axis=1)))
    t = np.ones(groups.n_groups)
    t[g] = 0.0
    out = api.light_mix(frames, t)
    mine = only_one & bad[g]
    assert mine.any() and np.isfinite(out[mine]).all()
    assert not np.isfinite(api.light_mix(frames, np.ones(groups.n_groups))[mine][:, :3]).all(axis=-1).any()


# ---------------------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_output_untouched_and_name_the_field(dev):
    hs = load("nested_lights")
    scene = api.DeviceScene(hs.desc, 0)
    good = auto(hs)
    n_mat = hs.desc.contents.n_materials
    shape = (good.n_groups, hs.height, hs.width, 4)

    def call(groups, params=hs.params):
        out_g = np.full(shape, 7.5)
        out = np.full(shape[1:], 7.5)
        st = dev.rt_render_light_groups(scene._h, C.byref(hs.camera), C.byref(params), C.byref(groups), out_g.ctypes.data, out.ctypes.data)
        assert (out_g == 7.5).all() and (out == 7.5).all(), "output written on an error"
        return st, dev.rt_last_error().decode()

    mega = hs.params.copy()
    mega.pipeline = api.RT_PIPELINE_MEGAKERNEL
    st, msg = call(good, mega)
    assert st == api.RT_E_UNSUPPORTED and "MEGAKERNEL" in msg
    stats = hs.params.copy()
    stats.collect_stats = 1
    assert call(good, stats)[0] == api.RT_E_UNSUPPORTED
    bad_table = good.table.copy()
    bad_table[n_mat - 1] = good.n_groups
    st, msg = call(api.RtLightGroups.make(good.n_groups, bad_table, good.background_group, 0))
    assert st == api.RT_E_INVALID and f"material_group[{n_mat - 1}]" in msg
    st, msg = call(api.RtLightGroups.make(good.n_groups, good.table, good.n_groups, 0))
    assert st == api.RT_E_INVALID and "background_group" in msg
    st, msg = call(api.RtLightGroups.make(good.n_groups, good.table, 0, good.n_groups))
    assert st == api.RT_E_INVALID and "unlit_group" in msg
    st, msg = call(api.RtLightGroups.make(good.n_groups, good.table[:-1], good.background_group, 0))
    assert st == api.RT_E_INVALID and "n_materials" in msg
    null = api.RtLightGroups.make(good.n_groups, good.table, good.background_group, 0)
    null.material_group = None
    st, msg = call(null)
    assert st == api.RT_E_INVALID and "material_group" in msg
    for n in (0, 17):
        st, msg = call(api.RtLightGroups.make(n, np.zeros(n_mat, dtype=np.uint8), 0, 0))
        assert st == api.RT_E_INVALID and "n_groups" in msg
    # and the scene still renders
    frames, frame = scene.render_light_groups(hs.camera, hs.params, good)
    assert bits(frame).tobytes() == bits(scene.render(hs.camera, hs.params)).tobytes()


# ---------------------------------------------------------------------------------------------------------------- rtrace
def run_rtrace(args, cwd):
    return subprocess.run([RTRACE] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def png_rgb8(path):
    return np.rint(api.load_image(str(path)).astype(np.float64) * 255.0).astype(np.uint8)


def test_rtrace_light_groups(dev, tmp_path):
    args = [os.path.join(REPO, "tests", "scenes", "nested_lights"), "-w=40", "-s=16", "-t=4", "--seed=74"]
    for sub in ("plain", "groups"):
        (tmp_path / sub).mkdir()
    r0 = run_rtrace(args, str(tmp_path / "plain"))
    assert r0.returncode == 0, r0.stderr
    plain = (tmp_path / "plain" / "out.png").read_bytes()
    assert not list((tmp_path / "plain").glob("out_light_*.png"))
    r = run_rtrace(args + ["--light-groups", "--light-mix=1,1"], str(tmp_path / "groups"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "groups" / "out.png").read_bytes() == plain
    hs = api.HostScene(args)
    hs.params.pipeline = api.RT_PIPELINE_WAVEFRONT
    groups = auto(hs)
    frames, frame = api.DeviceScene(hs.desc, 0).render_light_groups(hs.camera, hs.params, groups)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Light group ")]
    assert len(lines) == groups.n_groups and lines[0].startswith("Light group 0: unlit, mean luminance ")
    assert "material" in lines[1] and "mean luminance" in lines[1]
    others = [ln for ln in r.stdout.splitlines() if not ln.startswith("Light group ")]
    assert len(others) == len(r0.stdout.splitlines())
    for g in range(groups.n_groups):
        np.testing.assert_array_equal(png_rgb8(tmp_path / "groups" / f"out_light_{g}.png"), api.tonemap_rgb8(frames[g]))
    assert not (tmp_path / "groups" / f"out_light_{groups.n_groups}.png").exists()
    mixed = png_rgb8(tmp_path / "groups" / "out_mixed.png").astype(np.int32)
    assert np.abs(mixed - png_rgb8(tmp_path / "groups" / "out.png").astype(np.int32)).max() <= 1
