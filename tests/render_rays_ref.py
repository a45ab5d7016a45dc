"""Ray sets and oracle answers for the rt_render_rays tests (tests/test_render_rays_host.py, tests/test_gpu_render_rays.py).

Ray set of a scene, from ray_query_cases.cases(name) (-w=24 -s=1 --seed=31; texture_mix: -w=12): the oracle's surface hits of
the camera rays, walked with a fixed stride (wrapping round); origin k = (hit position + 0.01 * normal) rounded to the 2^-10
grid, skipped if a coordinate reaches 2^10; direction k = a normalised numpy.random.default_rng(7).normal(3), flipped into the
normal's hemisphere and rounded to the 2^-10 grid.  On that grid o + d and (o + d) - o are exact, so the reference's camera

    image 1 x n, position = o_i, first_pixel = o_i + d_i, pixel deltas 0, no aperture;  band_rows = 1, n_parts = n, part = i

sends every sample of its only owned pixel - row i, pixel index i - along (o_i, d_i): pyoracle.render of it is out[i] of
rt_render_rays, keyed (seed, replica, i, stratum).  The n_parts form costs one pixel per ray; the plain form (image n x 1,
every pixel rendered, pixel i kept) is the same thing n times as dear, and test_render_rays_host.py holds the two together.
Everything is computed once per (scene, n, S, T, seed) and shared."""
import functools

import numpy as np

import ray_query_cases as rq
from oracle import pyoracle
from rust_raytracer_amd import api

GRID = 1024.0   # 2^10: coordinates are multiples of 2^-10 and below 2^10 in magnitude
N, S, T, SEED, SEED_B = 37, 2, 3, 31, 77
# scenes of the f64 comparison; per scene (first hit, stride) through the surface hits
SCENES = ("cornell", "two_meshes", "sphere_field", "nested_transform", "smoke", "texture_mix", "sun_sky")
# (sun_sky: the hits on and under the two balls - from the open floor every ray ends in the sky, whatever the seed; two_meshes: an
# open scene without a background, most rays leave it black: the densest stretch of hits that see the light)
WALK = {"cornell": (0, 7), "two_meshes": (50, 1), "sphere_field": (0, 7), "nested_transform": (0, 7), "smoke": (0, 7),
        "texture_mix": (0, 3), "sun_sky": (120, 1)}


def to_grid(v):
    return np.round(np.asarray(v, dtype=np.float64) * GRID) / GRID


def ray_set(name, n):
    """(origins, dirs), (n, 3) each, on the 2^-10 grid."""
    c = rq.cases(name)
    surf = c.cam_hits[c.cam_hits["klass"] == rq.SURFACE]
    assert len(surf) > 0
    first, stride = WALK[name]
    rng = np.random.default_rng(7)
    o, d = [], []
    k = first
    while len(o) < n:
        h = surf[k % len(surf)]
        k += stride
        assert k < first + stride * (n + len(surf)), "too few usable hits"
        pos = to_grid(h["pos"] + 0.01 * h["normal"])
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v)
        if np.dot(v, h["normal"]) < 0:
            v = -v
        v = to_grid(v)
        if (np.abs(pos) >= GRID).any() or not v.any():
            continue
        o.append(pos)
        d.append(v)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def params_for(hs, s, t, seed, precision=api.RT_PRECISION_F64):
    """The scene's own depth, background and bias with S, T, seed and precision of the test."""
    p = hs.params.copy()
    p.sqrt_spt, p.thread_count, p.seed, p.precision = s, t, seed, precision
    p.band_rows, p.n_parts, p.part = 0, 1, 0
    p.pipeline, p.collect_stats = api.RT_PIPELINE_AUTO, 0
    return p


def ray_camera(o, d, width, height):
    """The zero-delta camera of ray (o, d): get_ray returns (o, d) for every pixel and stratum."""
    cam = api.RtCameraDesc()
    cam.image_width, cam.image_height = width, height
    for a in range(3):
        cam.position[a] = o[a]
        cam.first_pixel[a] = o[a] + d[a]
    cam.has_aperture = 0
    return cam


def oracle_ray(desc, params, o, d, i, n):
    """Pixel i of the reference's frame with the camera of ray (o, d), by the one-pixel form; (4,)."""
    p = params.copy()
    p.band_rows, p.n_parts, p.part = 1, n, i
    out, _ = pyoracle.render(desc, ray_camera(o, d, 1, n), p)
    assert out.shape == (1, 1, 4)
    return out[0, 0]


def oracle_ray_plain(desc, params, o, d, i, n):
    """The same through an n-wide frame rendered whole (n times the work)."""
    out, _ = pyoracle.render(desc, ray_camera(o, d, n, 1), params)
    assert out.shape == (1, n, 4)
    return out[0, i]


def oracle_rays(desc, params, origins, dirs):
    n = len(origins)
    return np.array([oracle_ray(desc, params, origins[i], dirs[i], i, n) for i in range(n)])


class Case:
    def __init__(self, name, n, s, t, seed):
        self.name, self.n, self.s, self.t, self.seed = name, n, s, t, seed
        self.hs = rq.cases(name).hs
        self.o, self.d = ray_set(name, n)
        self.params = params_for(self.hs, s, t, seed)
        self.ref = oracle_rays(self.hs.desc, self.params, self.o, self.d)   # (n, 4) f64


@functools.lru_cache(maxsize=None)
def case(name, n=N, s=S, t=T, seed=SEED):
    return Case(name, n, s, t, seed)


def assert_not_vacuous(c):
    """The ray set tests something: conditions on the oracle's answers alone."""
    for i in range(c.n):
        p = c.params.copy()
        p.band_rows, p.n_parts, p.part = 1, c.n, i
        got = pyoracle.get_ray(ray_camera(c.o[i], c.d[i], 1, c.n), p, c.t - 1, 0, i, c.s - 1, c.s - 1)
        assert got.tobytes() == np.concatenate([c.o[i], c.d[i]]).tobytes(), f"ray {i}: the reference camera does not return it"
    assert np.isfinite(c.ref).all()
    assert (c.ref[:, 3] == 0).all()
    nonzero = (c.ref[:, :3] != 0).any(axis=1)
    assert nonzero.sum() * 4 >= c.n, f"{c.name}: only {int(nonzero.sum())} of {c.n} rays carry radiance"
    other = case(c.name, c.n, c.s, c.t, SEED_B if c.seed != SEED_B else SEED)
    differ = (other.ref[:, :3] != c.ref[:, :3]).any(axis=1)
    assert differ.sum() * 4 >= c.n, f"{c.name}: only {int(differ.sum())} of {c.n} rays change with the seed"


def probe_rays_numpy(position, width, height):
    """rth_probe_rays restated: the same f64 operations in the same order, sines and cosines from the oracle's detmath."""
    pi = np.float64(3.14159265358979323846)
    o = np.empty((width * height, 3))
    d = np.empty((width * height, 3))
    for y in range(height):
        theta = (pi * (np.float64(y) + 0.5)) / np.float64(height)
        st, ct, _ = pyoracle.detmath(theta)
        for x in range(width):
            phi = ((2.0 * pi) * (np.float64(x) + 0.5)) / np.float64(width) - pi
            sp, cp, _ = pyoracle.detmath(phi)
            o[y * width + x] = position
            d[y * width + x] = (st * sp, ct, -(st * cp))
    return o, d
