"""Reference for the ambient-occlusion bake (rt_bake_visibility): plain numpy plus the oracle, per
point and sample (tests/test_bake_host.py, tests/test_gpu_bake.py).

For point i (position p, normal n) and sample s of a call with `seed`:
    r1, r2   = pyoracle.rng_uniforms(seed, 0, i, s, 2)
    sin, cos = pyoracle.detmath(r1 * 2 * pi)[:2]                      (the deterministic functions of include/rt_detmath.h)
    (x, y, z) = (cos * sqrt(r2), sin * sqrt(r2), sqrt(1 - r2))        (vec4.rs:50-61)
    w = n / |n|,  u, v = pyoracle.onb_from_vec(w)                     (utils.rs:17-28)
    d = u x + v y + w z + 0 * 0, summed left to right per component   (basis_apply, mat4.rs:342-353)
    visible = pyoracle.world_hit(desc, p, d, bias, max_distance) is None, or the hit is a Sky / Sun (they never occlude)
count = number of visible samples, visibility = count / S, bent = mean over ALL S samples of (visible ? d : 0).

Scenes and points: the oracle's camera hits of tests/ray_query_cases.py (24 pixels wide, seed 31), a fixed stride through the
surface hits, three shapes per scene: 16 points x 64 samples (one full pass of a wave), 4 x 100 (a second, partial pass) and
8 x 5 (a nearly empty wave): 1 464 oracle rays per scene (the oracle rebuilds its world for every ray), computed once per
process.  MAX_DISTANCE is fixed per scene so that the reference's answers are a test: mean visibility in [0.1, 0.9] and at
least a quarter of the 64-sample points partly occluded (assert_not_vacuous; checked on the CPU before the values were fixed)."""
import functools
import math
import sys

import numpy as np

from oracle import pyoracle
from ray_query_cases import SURFACE, cases

SEED = 2024
BIAS = 1e-3
SCENES = ["cornell", "two_meshes", "sphere_field", "nested_transform"]
MAX_DISTANCE = {"cornell": 300.0, "two_meshes": 4.0, "sphere_field": 8.0, "nested_transform": 4.0}
SHAPES = [(16, 64), (4, 100), (8, 5)]   # (points, samples)
DBL_MAX = sys.float_info.max


def direction(seed, i, s, normal):
    """Sample s of point i: the unit direction the kernel draws, in f64 and in its order of operations."""
    r1, r2 = pyoracle.rng_uniforms(seed, 0, i, s, 2)
    sn, cs = pyoracle.detmath(r1 * 2.0 * math.pi)[:2]
    sqrt_r2 = np.sqrt(r2)
    x, y, z = cs * sqrt_r2, sn * sqrt_r2, np.sqrt(1.0 - r2)
    n = np.asarray(normal, dtype=np.float64)
    w = n / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    u, v, w = pyoracle.onb_from_vec(w)
    zero = 0.0
    return np.array([u[k] * x + v[k] * y + w[k] * z + zero * zero for k in range(3)])


def occluded(desc, pos, d, bias, max_distance):
    h = pyoracle.world_hit(desc, pos, d, bias, max_distance)
    return h is not None and h["t"] != np.inf and h["t"] != DBL_MAX


def bake(desc, positions, normals, samples, seed=SEED, bias=BIAS, max_distance=float("inf")):
    """(count[n] int, visibility[n], bent[n, 3]) of the reference."""
    positions, normals = np.atleast_2d(positions), np.atleast_2d(normals)
    n = len(positions)
    count, bent = np.zeros(n, dtype=np.int64), np.zeros((n, 3))
    for i in range(n):
        for s in range(samples):
            d = direction(seed, i, s, normals[i])
            if not occluded(desc, positions[i], d, bias, max_distance):
                count[i] += 1
                bent[i] += d
    return count, count / float(samples), bent / float(samples)


def points(c, n, shape_index):
    """n surface points of a scene's camera hits: a fixed stride through them, another phase for every shape."""
    surf = c.cam_hits[c.cam_hits["klass"] == SURFACE]
    stride = len(surf) // n
    assert stride >= 1
    first = (shape_index * stride) // 3
    sel = surf[first::stride][:n]
    assert len(sel) == n
    return np.ascontiguousarray(sel["pos"]), np.ascontiguousarray(sel["normal"])


class BakeCase:
    def __init__(self, name):
        self.name = name
        self.cases = cases(name)
        self.desc = self.cases.hs.desc
        self.max_distance = MAX_DISTANCE[name]
        self.shapes = []   # (positions, normals, samples, count, visibility, bent)
        for k, (n, samples) in enumerate(SHAPES):
            p, nr = points(self.cases, n, k)
            self.shapes.append((p, nr, samples) + bake(self.desc, p, nr, samples, max_distance=self.max_distance))

    def assert_not_vacuous(self):
        """Conditions on the reference's answers (not tolerances): the bake has something to get wrong."""
        rays = sum(len(p) * s for p, _, s, *_ in self.shapes)
        vis = sum(int(c.sum()) for *_, c, _, _ in self.shapes) / rays
        assert 0.1 <= vis <= 0.9, f"{self.name}: mean visibility {vis:.3f}"
        _, _, s64, c64, _, _ = self.shapes[0]
        partly = ((c64 > 0) & (c64 < s64)).mean()
        assert partly >= 0.25, f"{self.name}: only {partly:.2%} of the 64-sample points are partly occluded"


@functools.lru_cache(maxsize=None)
def bake_case(name):
    return BakeCase(name)
