"""Light groups without a GPU (include/rt_mi355.h): the automatic assignment rt_light_groups_auto, the
numpy restatement of the re-mix and of the ordered per-group sums with the bound of property 4, and rtrace's flags."""
import ctypes as C

import numpy as np
import pytest

import light_groups_ref as lgr
from rust_raytracer_amd import api

E = api.RT_MAT_EMISSIVE


def scene(args):
    return api.HostScene(list(args) + ["-w=16", "-s=4"])


def material_types(hs):
    d = hs.desc.contents
    return [d.materials[i].type for i in range(d.n_materials)]


def test_struct_layout_and_symbols():
    lib = api.load_device_lib()
    for name in ("rt_light_groups_auto", "rt_render_light_groups", "rt_render_light_groups_device", "rt_light_mix", "rt_light_mix_device"):
        assert hasattr(lib, name), name
    assert C.sizeof(api.RtLightGroups) == 8 + 8 + 8 + 16
    assert api.RT_LIGHT_GROUPS_MAX == 16


def test_auto_nested_lights_one_group_per_emissive_material():
    hs = scene(["tests/scenes/nested_lights"])
    types = material_types(hs)
    emissive = [i for i, t in enumerate(types) if t == E]
    assert len(emissive) == 4
    g = api.light_groups_auto(hs.desc, 16, has_background=False)
    assert g.n_groups == 5 and g.unlit_group == 0 and g.background_group == 0
    assert [int(g.table[i]) for i in emissive] == [1, 2, 3, 4]  # ascending material index
    assert all(int(g.table[i]) == 0 for i in range(len(types)) if i not in emissive)
    gb = api.light_groups_auto(hs.desc, 16, has_background=True)
    assert gb.n_groups == 6 and gb.background_group == 5 and list(gb.table) == list(g.table)


def test_auto_sun_sky_embedded_materials():
    hs = scene(["tests/scenes/sun_sky"])
    d = hs.desc.contents
    embedded = sorted(d.nodes[i].material for i in range(d.n_nodes) if d.nodes[i].type in (7, 8))  # RT_NODE_SKY, RT_NODE_SUN
    assert len(embedded) == 2 and all(d.materials[m].type == E for m in embedded)
    g = api.light_groups_auto(hs.desc)
    assert g.n_groups == 3
    assert [int(g.table[m]) for m in embedded] == [1, 2]


def test_auto_cornell_with_background_and_a_scene_without_emitters():
    hs = scene(["scenes/cornell"])
    types = material_types(hs)
    n_e = sum(t == E for t in types)
    assert n_e >= 1
    g = api.light_groups_auto(hs.desc, 16, has_background=True)
    assert g.n_groups == n_e + 2 and g.background_group == n_e + 1
    # no emitter at all: the materials of cornell turned into Lambertian
    d = hs.desc.contents
    for i in range(d.n_materials):
        if d.materials[i].type == E:
            d.materials[i].type = api.RT_MAT_LAMBERTIAN
    g = api.light_groups_auto(hs.desc, 16, has_background=False)
    assert g.n_groups == 1 and not g.table.any() and g.background_group == 0
    g = api.light_groups_auto(hs.desc, 16, has_background=True)
    assert g.n_groups == 2 and not g.table.any() and g.background_group == 1


def test_auto_ignores_materials_no_node_of_world_references_and_normal_debug():
    hs = scene(["tests/scenes/nested_lights"])
    d = hs.desc.contents
    emissive = [i for i, t in enumerate(material_types(hs)) if t == E]
    victim = emissive[1]
    for i in range(d.n_nodes):  # detach one lamp's material from every node
        if d.nodes[i].material == victim:
            d.nodes[i].material = emissive[0]
    g = api.light_groups_auto(hs.desc)
    assert int(g.table[victim]) == 0 and g.n_groups == 4
    d.materials[emissive[2]].type = api.RT_MAT_NORMAL_DEBUG
    g = api.light_groups_auto(hs.desc)
    assert int(g.table[emissive[2]]) == 0 and g.n_groups == 3


def test_auto_overflow_determinism_and_range():
    hs = scene(["tests/scenes/nested_lights"])
    emissive = [i for i, t in enumerate(material_types(hs)) if t == E]
    g = api.light_groups_auto(hs.desc, 2, has_background=True)
    assert g.n_groups == 2 and g.background_group == 1
    assert [int(g.table[i]) for i in emissive] == [1, 1, 1, 1]
    g3 = api.light_groups_auto(hs.desc, 3, has_background=True)
    assert [int(g3.table[i]) for i in emissive] == [1, 2, 2, 2] and g3.background_group == 2 and g3.n_groups == 3
    g1 = api.light_groups_auto(hs.desc, 1, has_background=True)
    assert g1.n_groups == 1 and not g1.table.any() and g1.background_group == 0
    again = api.light_groups_auto(hs.desc, 3, has_background=True)
    assert again.table.tobytes() == g3.table.tobytes() and again.background_group == g3.background_group
    lib = api.load_device_lib()
    for bad in (0, 17, 1000):
        with pytest.raises(api.RtError) as e:
            api.light_groups_auto(hs.desc, bad)
        assert e.value.status == api.RT_E_INVALID and "max_groups" in str(e.value)
    table = np.full(hs.desc.contents.n_materials, 99, dtype=np.uint8)
    bg, n = C.c_uint32(77), C.c_uint32(77)
    assert lib.rt_light_groups_auto(hs.desc, 0, 0, table.ctypes.data, C.byref(bg), C.byref(n)) == api.RT_E_INVALID
    assert (table == 99).all() and bg.value == 77 and n.value == 77  # outputs untouched on an error


def test_mix_restatement():
    rng = np.random.default_rng(5)
    groups = rng.random((3, 4, 5, 4))
    groups[..., 3] = 0.0
    tints = np.array([[1.0, 0.5, 2.0], [0.0, 0.0, 0.0], [3.0, 1.0, 0.25]])
    out = lgr.mix(groups, tints)
    want = (tints[0] * groups[0, ..., :3] + 0.0) + tints[2] * groups[2, ..., :3]
    assert out[..., :3].tobytes() == want.tobytes() and not out[..., 3].any()
    # a tint of exactly 0 switches the group off, infinities and NaNs included
    groups[1, 0, 0, 0] = np.nan
    groups[1, 1, 1, 1] = np.inf
    assert np.isfinite(lgr.mix(groups, tints)).all()
    assert np.isnan(lgr.mix(groups, np.ones(3))[0, 0, 0])
    # scalars per group = the same tint in every channel
    assert lgr.mix(groups, np.array([1.0, 0.0, 2.0])).tobytes() == lgr.mix(groups, np.array([[1.0] * 3, [0.0] * 3, [2.0] * 3])).tobytes()


@pytest.mark.parametrize("S,T,G", [(1, 1, 1), (2, 4, 6), (4, 3, 16), (3, 10, 8)])
def test_sum_of_group_frames_obeys_the_bound(S, T, G):
    """Property 4 on synthetic non-negative samples spread over many magnitudes: the ordered per-group sums, added in
    group order, stay within (S^2 + T + G + 2) 2^-52 of the ordered sum of all samples."""
    rng = np.random.default_rng(S * 100 + T * 10 + G)
    npix = 4096
    samples = rng.random((T, S * S, npix, 3)) * 10.0 ** rng.integers(-8, 8, (T, S * S, npix, 1))
    samples[rng.random(samples.shape) < 0.3] = 0.0
    gid = rng.integers(0, G, (T, S * S, npix))
    frame = lgr.resolve(samples)
    groups = lgr.resolve_groups(samples, gid, G)
    f4 = np.concatenate([frame, np.zeros((npix, 1))], axis=1)[None]
    g4 = np.concatenate([groups, np.zeros((G, npix, 1))], axis=2)[:, None]
    worst = lgr.assert_sum_property(g4, f4, S, T)
    assert worst <= lgr.sum_bound(S, T, G)
    # one group holding everything is the frame itself, bit for bit; an unused group is +0.0
    solo = lgr.resolve_groups(samples, np.zeros_like(gid), 2)
    assert solo[0].tobytes() == frame.tobytes() and not solo[1].view(np.uint64).any()


def test_mask_rule_of_the_restatement():
    samples = np.ones((2, 4, 8, 3))
    gid = np.zeros((2, 4, 8), dtype=np.int64)
    gid[1, 2, 5] = 1
    samples[1, 2, 5, 0] = np.nan
    samples[0, 1, 3, 2] = np.inf
    groups = lgr.resolve_groups(samples, gid, 3)
    frame = lgr.resolve(samples)
    assert np.isnan(groups[1, 5, 0]) and np.isfinite(groups[0, 5]).all() and np.isinf(groups[0, 3, 2])
    np.testing.assert_array_equal(~np.isfinite(groups).all(axis=0), ~np.isfinite(frame))
    assert not groups[2].view(np.uint64).any()


def test_rtrace_flags():
    lib = api.load_host_lib()
    lib.rth_light_groups.argtypes = [C.c_void_p]
    lib.rth_light_groups.restype = C.c_uint32
    lib.rth_light_mix.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint32]
    lib.rth_light_mix.restype = C.c_int32
    w = (C.c_double * 16)()
    hs = api.HostScene(["scenes/cornell", "-w=16", "-s=4"])
    assert lib.rth_light_groups(hs._h) == 0 and lib.rth_light_mix(hs._h, w, 16) == -1
    hs = api.HostScene(["scenes/cornell", "-w=16", "-s=4", "--light-groups"])
    assert lib.rth_light_groups(hs._h) == 16 and lib.rth_light_mix(hs._h, w, 16) == -1
    hs = api.HostScene(["scenes/cornell", "-w=16", "-s=4", "--light-groups=3", "--light-mix=0.5,0,2"])
    assert lib.rth_light_groups(hs._h) == 3 and lib.rth_light_mix(hs._h, w, 16) == 3 and list(w[:3]) == [0.5, 0.0, 2.0]
    assert lib.rth_light_mix(hs._h, w, 1) == 3  # the count given, whatever the capacity
    for bad, word in ((["--light-groups=0"], "Light group count"), (["--light-groups=17"], "Light group count"),
                      (["--light-mix=1,2"], "requires --light-groups"), (["--light-groups", "--light-mix=1,x"], "Light mix"),
                      (["--light-groups", "--gpus=2"], "--light-groups"), (["--light-groups", "--progressive=2"], "--light-groups"),
                      (["--light-groups", "--pipeline=mega"], "wavefront")):
        with pytest.raises(api.RtError) as e:
            api.HostScene(["scenes/cornell", "-w=16", "-s=4"] + bad)
        assert word in str(e.value), (bad, str(e.value))
