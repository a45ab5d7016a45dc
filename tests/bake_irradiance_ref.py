"""Reference for the irradiance bake (rt_bake_irradiance): plain numpy plus the oracle, per point and
sample (tests/test_bake_irradiance_host.py, tests/test_gpu_bake_irradiance.py).

For point i (position p, normal n), replica t and stratum st = sy * S + sx of a call with `seed`:
    r1, r2   = pyoracle.rng_uniforms(seed, t, i, st, 2)              (the two draws a camera spends on its jitter)
    u1, u2   = (sx + r1) * (1 / S), (sy + r2) * (1 / S)
    sin, cos = pyoracle.detmath(u1 * 2 * pi)[:2]                      (the deterministic functions of include/rt_detmath.h)
    (x, y, z) = (cos * sqrt(u2), sin * sqrt(u2), sqrt(1 - u2))        (vec4.rs:50-61)
    w = n / |n|,  u, v = pyoracle.onb_from_vec(w)                     (utils.rs:17-28)
    d = u x + v y + w z + 0 * 0, summed left to right per component   (basis_apply, mat4.rs:342-353)
    camera = render_rays_ref.ray_camera(p, p + d, 1, n_points): position = p, first_pixel = fl(p + d), pixel deltas 0, no
             aperture, so get_ray returns (p, fl(fl(p + d) - p)) = the first ray of the device
    L = pyoracle.trace_sample(desc, camera, params, t, 0, i, sx, sy): keyed (seed, t, i, st); the camera's own two jitter draws
        are the r1, r2 above, so the path's first draw is the third of the stream on both sides
out[i] = sum over t, in order, of ((sum over st, in order, of L) / (S^2 T)), in f64: the ordered sum k_wf_resolve forms for a
pixel of a frame (camera.rs:229,247-253: every replica's strata are divided by the samples per pixel, S^2 T).

Points: the oracle's surface hits of the camera rays of tests/ray_query_cases.py (24 pixels wide, seed 31), walked with a fixed
stride per scene (WALK: the stretches of render_rays_ref.WALK, which say where two_meshes and sun_sky see light), position =
hit + 0.01 * normal, no grid rounding.  Everything is computed once per (scene, n, S, T, seed) and shared; the oracle rebuilds
its world for every sample."""
import functools
import math

import numpy as np

import ray_query_cases as rq
import render_rays_ref as rr
from oracle import pyoracle

N, S, T, SEED, SEED_B = 37, 2, 3, 31, 77
SCENES = ("cornell", "two_meshes", "sphere_field", "nested_transform", "smoke", "texture_mix", "sun_sky")
WALK = dict(rr.WALK)


def uniforms(seed, t, i, sx, sy, s):
    """(u1, u2) of sample (t, i, sy * s + sx): the stratified pair the direction is formed from."""
    r1, r2 = pyoracle.rng_uniforms(seed, t, i, sy * s + sx, 2)
    inv_s = 1.0 / float(s)
    return (float(sx) + r1) * inv_s, (float(sy) + r2) * inv_s


def direction(u1, u2, normal):
    """The unit direction of (u1, u2) about `normal`, in f64 and in the device's order of operations (before the round trip)."""
    sn, cs = pyoracle.detmath(u1 * 2.0 * math.pi)[:2]
    sqrt_u2 = np.sqrt(u2)
    x, y, z = cs * sqrt_u2, sn * sqrt_u2, np.sqrt(1.0 - u2)
    n = np.asarray(normal, dtype=np.float64)
    w = n / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    u, v, w = pyoracle.onb_from_vec(w)
    zero = 0.0
    return np.array([u[k] * x + v[k] * y + w[k] * z + zero * zero for k in range(3)])


def first_ray(seed, t, i, sx, sy, s, pos, normal):
    """(o, d') of the sample: d' = (o + d) - o, two roundings per component."""
    o = np.asarray(pos, dtype=np.float64)
    d = direction(*uniforms(seed, t, i, sx, sy, s), normal)
    return o, (o + d) - o


def first_rays(pos, nrm, s, t, seed, first=0):
    """(n * t * s * s, 6): every sample's (o, d'), point-major, then replica, then stratum; point k has index first + k."""
    return np.array([np.concatenate(first_ray(seed, tt, first + k, st % s, st // s, s, pos[k], nrm[k]))
                     for k in range(len(pos)) for tt in range(t) for st in range(s * s)])


def point_set(name, n):
    """(positions, normals), (n, 3) each: hit + 0.01 * normal along the scene's walk through the camera's surface hits."""
    c = rq.cases(name)
    surf = c.cam_hits[c.cam_hits["klass"] == rq.SURFACE]
    assert len(surf) > 0
    first, stride = WALK[name]
    sel = [surf[(first + k * stride) % len(surf)] for k in range(n)]
    pos = np.array([h["pos"] + 0.01 * h["normal"] for h in sel])
    nrm = np.array([h["normal"] for h in sel])
    return np.ascontiguousarray(pos), np.ascontiguousarray(nrm)


def oracle_bake(desc, params, pos, nrm, first=0):
    """(n, 4) f64 reference of rt_bake_irradiance for points whose indices in the call are first, first + 1, ..."""
    s, t, n = params.sqrt_spt, params.thread_count, len(pos)
    out = np.zeros((n, 4))
    for k in range(n):
        i = first + k
        acc = np.zeros(3)
        for tt in range(t):
            rep = np.zeros(3)
            for st in range(s * s):
                sx, sy = st % s, st // s
                d = direction(*uniforms(params.seed, tt, i, sx, sy, s), nrm[k])
                cam = rr.ray_camera(pos[k], d, 1, first + n)
                rgb, _ = pyoracle.trace_sample(desc, cam, params, tt, 0, i, sx, sy)
                rep = rep + rgb
            acc = acc + rep / (float(s) * float(s) * float(t))
        out[k, :3] = acc
    return out


class Case:
    def __init__(self, name, n, s, t, seed):
        self.name, self.n, self.s, self.t, self.seed = name, n, s, t, seed
        self.hs = rq.cases(name).hs
        self.pos, self.nrm = point_set(name, n)
        self.params = rr.params_for(self.hs, s, t, seed)
        self.ref = oracle_bake(self.hs.desc, self.params, self.pos, self.nrm)   # (n, 4) f64


@functools.lru_cache(maxsize=None)
def case(name, n=N, s=S, t=T, seed=SEED):
    return Case(name, n, s, t, seed)


def assert_not_vacuous(c):
    """The point set tests something: conditions on the oracle's answers alone."""
    for i in range(c.n):
        for tt in range(c.t):
            for st in range(c.s * c.s):
                sx, sy = st % c.s, st // c.s
                o, d1 = first_ray(c.seed, tt, i, sx, sy, c.s, c.pos[i], c.nrm[i])
                d = direction(*uniforms(c.seed, tt, i, sx, sy, c.s), c.nrm[i])
                got = pyoracle.get_ray(rr.ray_camera(o, d, 1, c.n), c.params, tt, 0, i, sx, sy)
                assert got.tobytes() == np.concatenate([o, d1]).tobytes(), f"point {i}, sample ({tt}, {st}): the reference camera does not return (o, (o + d) - o)"
    assert np.isfinite(c.ref).all()
    assert (c.ref[:, 3] == 0).all()
    nonzero = (c.ref[:, :3] != 0).any(axis=1)
    assert nonzero.sum() * 4 >= c.n, f"{c.name}: only {int(nonzero.sum())} of {c.n} points carry radiance"
    other = case(c.name, c.n, c.s, c.t, SEED_B if c.seed != SEED_B else SEED)
    differ = (other.ref[:, :3] != c.ref[:, :3]).any(axis=1)
    assert differ.sum() * 4 >= c.n, f"{c.name}: only {int(differ.sum())} of {c.n} points change with the seed"
