"""One whole path vertex on the GPU - search, hit resolution, textures, material, light sampling and weight - against the CPU
oracle, vertex by vertex (rt_debug_shade_rays against pyoracle.shade_rays; tests/f32_shade_bounds.py has the f32 rule and its
derivation, tests/shade_vertex_cases.py the vertex sets, tests/test_f32_shade_bounds_host.py shows that the rule fails what it
must fail).

f64: the probe's answers equal the oracle's (53-bit draws) on every set, nothing excused: discrete fields, the number of draws
     and the generator state exactly, reals at the project's 1e-12 bar, NaN and infinity of the same kind.
f32: the rule on every set, for the kernel variant the render picks and for the full variant.
Every test prints its figures before it asserts."""
import numpy as np
import pytest

from rust_raytracer_amd import api
from ray_query_cases import close
import f32_shade_bounds as sb
import shade_vertex_cases as vc

pytestmark = pytest.mark.gpu

F32 = api.RT_PRECISION_F32


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


_scenes = {}


def device_scene(s):
    """One DeviceScene per set for the whole module (the probe leaves a scene as it was)."""
    if s.label not in _scenes:
        _scenes[s.label] = api.DeviceScene(s.hs.desc, 0)
    return _scenes[s.label]


def needs_full(s):
    """The render picks the full kernel variant: the simple one is refused."""
    try:
        device_scene(s).shade_rays(s.params, s.o[:1], s.d[:1], s.states[:1], variant=2)
        return False
    except api.RtError as e:
        assert e.status == api.RT_E_INVALID
        return True


def f64_mismatches(s, got, st):
    """{field: vertices that differ from the oracle's R64}"""
    want, wst = s.r64, s.s64
    hit = want[:, sb.MATERIAL] >= 0
    klass = sb.classes_of(s.hs.desc, s.params, got, s.states, st, False)
    wk = want[:, sb.OP].astype(np.int64)
    # the kernels end a path whose weight is zero or NaN in every channel; the radiance is then that weight
    w = got[:, sb.WEIGHT]
    ended = np.isin(wk, sb.CONTINUING) & (got[:, sb.CONT] == 0) & ((w == 0).all(axis=1) | np.isnan(w).all(axis=1))
    bad = {
        "material": got[:, sb.MATERIAL] != want[:, sb.MATERIAL],
        "front": hit & (got[:, sb.FRONT] != want[:, sb.FRONT]),
        "state": st != wst,
        "search draws": got[:, sb.SEARCH_DRAWS] != want[:, sb.SEARCH_DRAWS],
        "class": klass != wk,
        "continues": ~ended & (got[:, sb.CONT] != want[:, sb.CONT]),
        "ended radiance": ended & ~((got[:, sb.RADIANCE] == w) | np.isnan(w)).all(axis=1),
    }
    both = (got[:, sb.CONT] != 0) & (want[:, sb.CONT] != 0)
    uv = hit & ((got[:, sb.UU] != 0) | (got[:, sb.VV] != 0))   # (u, v) stay 0 where no texture of the material reads them
    for name, sl, rows in (("t", slice(0, 1), hit), ("pos", sb.POS, hit), ("normal", sb.NORMAL, hit), ("uv", slice(7, 9), uv),
                           ("tex_a", sb.TEX_A, hit), ("tex_b", slice(15, 16), hit), ("direction", sb.DIR, both),
                           ("weight", sb.WEIGHT, np.ones(len(got), bool)), ("radiance", sb.RADIANCE, ~ended)):
        bad[name] = rows & ~close(got[:, sl], want[:, sl]).all(axis=1)
    return {k: np.nonzero(v)[0] for k, v in bad.items() if v.any()}


@pytest.mark.parametrize("name", vc.ALL_SETS)
def test_f64_vertices_equal_the_oracle(dev, name):
    s = vc.vertex_set(name)
    s.assert_not_vacuous()
    scene = device_scene(s)
    full = needs_full(s)
    p = s.params.copy()
    results = {v: scene.shade_rays(p, s.o, s.d, s.states, variant=v) for v in ((0, 1) if full else (0, 1, 2))}
    same = 1 if full else 2                                             # variant 0 IS the full / the simple variant here
    assert results[0][0].tobytes() == results[same][0].tobytes() and results[0][1].tobytes() == results[same][1].tobytes()
    report = {v: f64_mismatches(s, *results[v]) for v in (0, 1)}
    for v, bad in report.items():
        print(f"{name} f64 variant {v}: {len(s.o)} vertices, mismatches " +
              (", ".join(f"{k}: {len(i)} (first {i[:3].tolist()})" for k, i in bad.items()) or "none"))
    assert not report[0] and not report[1]


@pytest.mark.parametrize("name", vc.ALL_SETS)
def test_f32_vertices_within_the_rule(dev, name):
    s = vc.vertex_set(name)
    s.assert_not_vacuous()
    scene = device_scene(s)
    p = s.params.copy()
    p.precision = F32
    reports = []
    for v in (0, 1):
        got, st = scene.shade_rays(p, s.o, s.d, s.states, variant=v)
        klass = sb.classes_of(s.hs.desc, p, got, s.states, st, True)
        reports.append(sb.check(s.answers, got, st, klass, f"{name} f32 variant {v}"))
        print(reports[-1].line())     # both lines before any assertion
    for rep in reports:
        rep.check(show=False)
