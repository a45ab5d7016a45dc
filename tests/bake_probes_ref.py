"""Reference for the SH probe bake (rt_bake_probes): plain numpy plus the oracle, per probe and sample
(tests/test_bake_probes_host.py, tests/test_gpu_bake_probes.py).

For probe i (position p), replica t and stratum st = sy * S + sx of a call with `seed`:
    r1, r2   = pyoracle.rng_uniforms(seed, t, i, st, 2)              (the two draws a camera spends on its jitter)
    u1, u2   = (sx + r1) * (1 / S), (sy + r2) * (1 / S)              (bake_irradiance_ref.uniforms: formed exactly as that bake's)
    z = 1 - 2 u2,  r = sqrt(1 - z z),  sin, cos = pyoracle.detmath(u1 * 2 * pi)[:2],  d = (cos r, sin r, z)
    camera = render_rays_ref.ray_camera(p, d, 1, n_probes): position = p, first_pixel = fl(p + d), pixel deltas 0, no aperture,
             so get_ray returns (p, fl(fl(p + d) - p)) = the first ray of the device
    L = pyoracle.trace_sample(desc, camera, params, t, 0, i, sx, sy): keyed (seed, t, i, st); the camera's own two jitter draws
        are the r1, r2 above, so the path's first draw is the third of the stream on both sides
    Y_0 .. Y_8 = the real L2 basis on d (not on the round-tripped direction), positive signs
out[i][k] = sum over t, in order, of ((sum over st, in order, of fl(Y_k * L)) / (S^2 T)), in f64.

Probes: the midpoints between the camera position and the oracle's surface hits of the camera rays of tests/ray_query_cases.py
(24 pixels wide, seed 31), walked with render_rays_ref.WALK's (first hit, stride) per scene: positions in free space in front of
what the camera sees.  Everything is computed once per (scene, n, S, T, seed) and shared; the oracle rebuilds its world for every
sample."""
import functools
import math

import numpy as np

import bake_irradiance_ref as br
import ray_query_cases as rq
import render_rays_ref as rr
from oracle import pyoracle

N, S, T, SEED, SEED_B = 37, 2, 3, 31, 77
SCENES = rr.SCENES
WALK = dict(rr.WALK)

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2A = 1.0925484305920792
C2B = 0.31539156525252005
C2C = 0.5462742152960396
# max |Y_k| over the unit sphere, k = 0 .. 8
Y_MAX = np.array([C0, C1, C1, C1, C2C, C2C, 0.6307831305050401, C2C, C2C])

uniforms = br.uniforms


def direction(u1, u2):
    """The uniform-sphere direction of (u1, u2), in f64 and in the device's order of operations (before the round trip)."""
    z = 1.0 - 2.0 * u2
    r = np.sqrt(1.0 - z * z)
    sn, cs = pyoracle.detmath(u1 * 2.0 * math.pi)[:2]
    return np.array([cs * r, sn * r, z])


def basis(d):
    """(9,): Y_0 .. Y_8 on d, every product and difference rounded as written."""
    x, y, z = (np.float64(v) for v in d)
    return np.array([C0, C1 * y, C1 * z, C1 * x, C2A * (x * y), C2A * (y * z), C2B * (3.0 * (z * z) - 1.0), C2A * (x * z),
                     C2C * (x * x - y * y)])


def sample_dirs(n, s, t, seed, first=0):
    """(n, t, s * s, 3): d of every sample; probe k has index first + k."""
    return np.array([[[direction(*uniforms(seed, tt, first + k, st % s, st // s, s)) for st in range(s * s)] for tt in range(t)]
                     for k in range(n)])


def first_rays(pos, s, t, seed, first=0):
    """(n * t * s * s, 6): every sample's (o, d'), probe-major, then replica, then stratum; d' = (o + d) - o."""
    dirs = sample_dirs(len(pos), s, t, seed, first)
    rows = []
    for k in range(len(pos)):
        o = np.asarray(pos[k], dtype=np.float64)
        for d in dirs[k].reshape(-1, 3):
            rows.append(np.concatenate([o, (o + d) - o]))
    return np.array(rows).reshape(-1, 6)


def ordered_sums(dirs, radiance, s, t):
    """(n, 9, 4): the device's ordered sums for dirs (n, t, s * s, 3) and radiance (n, t, s * s, 3)."""
    n = len(dirs)
    out = np.zeros((n, 9, 4))
    spp = float(s) * float(s) * float(t)
    for k in range(n):
        acc = np.zeros((9, 3))
        for tt in range(t):
            rep = np.zeros((9, 3))
            for st in range(s * s):
                rep = rep + basis(dirs[k, tt, st])[:, None] * radiance[k, tt, st][None, :]
            acc = acc + rep / spp
        out[k, :, :3] = acc
    return out


def probe_set(name, n):
    """(n, 3): midpoints between the camera and the scene's walk through the camera's surface hits."""
    c = rq.cases(name)
    surf = c.cam_hits[c.cam_hits["klass"] == rq.SURFACE]
    assert len(surf) > 0
    first, stride = WALK[name]
    eye = np.array(list(c.hs.camera.position))
    pos = np.array([(eye + surf[(first + k * stride) % len(surf)]["pos"]) * 0.5 for k in range(n)])
    return np.ascontiguousarray(pos)


def oracle_radiance(desc, params, pos, first=0):
    """(dirs, L), (n, t, s * s, 3) each: every sample's direction and the oracle's radiance along its first ray."""
    s, t, n = params.sqrt_spt, params.thread_count, len(pos)
    dirs = sample_dirs(n, s, t, params.seed, first)
    L = np.zeros_like(dirs)
    for k in range(n):
        for tt in range(t):
            for st in range(s * s):
                cam = rr.ray_camera(pos[k], dirs[k, tt, st], 1, first + n)
                L[k, tt, st], _ = pyoracle.trace_sample(desc, cam, params, tt, 0, first + k, st % s, st // s)
    return dirs, L


def oracle_probes(desc, params, pos, first=0):
    """(n, 9, 4) f64 reference of rt_bake_probes for probes whose indices in the call are first, first + 1, ..."""
    dirs, L = oracle_radiance(desc, params, pos, first)
    return ordered_sums(dirs, L, params.sqrt_spt, params.thread_count)


class Case:
    def __init__(self, name, n, s, t, seed):
        self.name, self.n, self.s, self.t, self.seed = name, n, s, t, seed
        self.hs = rq.cases(name).hs
        self.pos = probe_set(name, n)
        self.params = rr.params_for(self.hs, s, t, seed)
        self.dirs, self.L = oracle_radiance(self.hs.desc, self.params, self.pos)
        self.ref = ordered_sums(self.dirs, self.L, s, t)   # (n, 9, 4) f64


@functools.lru_cache(maxsize=None)
def case(name, n=N, s=S, t=T, seed=SEED):
    return Case(name, n, s, t, seed)


def assert_band_bound(sh, slack):
    """|out_k| <= (max |Y_k| / Y0) * out_0 per probe and channel, which holds because L >= 0; `slack` relative."""
    a0 = sh[:, 0, :3]
    assert (a0 >= 0).all()
    for k in range(1, 9):
        bound = (Y_MAX[k] / C0) * a0 * (1.0 + slack)
        over = np.abs(sh[:, k, :3]) > bound
        assert not over.any(), f"coefficient {k}: {int(over.sum())} values above (max |Y_k| / Y0) * out_0"


def assert_not_vacuous(c):
    """The probe set tests something: conditions on the oracle's answers alone."""
    for i in range(c.n):
        for tt in range(c.t):
            for st in range(c.s * c.s):
                sx, sy = st % c.s, st // c.s
                o, d = c.pos[i], c.dirs[i, tt, st]
                got = pyoracle.get_ray(rr.ray_camera(o, d, 1, c.n), c.params, tt, 0, i, sx, sy)
                assert got.tobytes() == np.concatenate([o, (o + d) - o]).tobytes(), f"probe {i}, sample ({tt}, {st}): the reference camera does not return (o, (o + d) - o)"
    assert np.isfinite(c.ref).all()
    assert (c.ref[:, :, 3] == 0).all()
    lit = (c.ref[:, 0, :3] != 0).any(axis=1)
    assert lit.sum() * 4 >= c.n, f"{c.name}: only {int(lit.sum())} of {c.n} probes carry radiance"
    assert (c.ref[lit][:, 1:, :3] != 0).any(axis=2).all(), f"{c.name}: a lit probe has a zero coefficient in bands 1-2"
    assert (c.ref[~lit] == 0).all()
    other = case(c.name, c.n, c.s, c.t, SEED_B if c.seed != SEED_B else SEED)
    differ = (other.ref[:, :, :3] != c.ref[:, :, :3]).any(axis=(1, 2))
    assert differ.sum() * 4 >= c.n, f"{c.name}: only {int(differ.sum())} of {c.n} probes change with the seed"
    assert_band_bound(c.ref, 1e-12)
