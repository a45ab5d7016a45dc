"""numpy restatement of the light-group arithmetic (include/rt_mi355.h) and the scene edits the tests
share: the re-mix of rt_light_mix, the ordered sums of k_wf_resolve / k_wf_resolve_groups, the bound of property 4, and the
"zeroed" scene in which every emitter outside one group emits nothing."""
import ctypes as C

import numpy as np

from rust_raytracer_amd import api

EPS = 2.0 ** -52


def mix(groups: np.ndarray, tints: np.ndarray) -> np.ndarray:
    """out = ((term_0 + term_1) + ...) per channel, term_g = tint_g * f_g, or +0.0 where tint_g == 0; w = 0."""
    groups = np.asarray(groups, dtype=np.float64)
    tints = np.asarray(tints, dtype=np.float64)
    if tints.ndim == 1:
        tints = np.repeat(tints[:, None], 3, axis=1)
    out = np.zeros(groups.shape[1:], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(groups.shape[0]):
            for k in range(3):
                t = tints[g, k]
                term = np.zeros(groups.shape[1:3]) if t == 0.0 else t * groups[g, ..., k]
                out[..., k] = term if g == 0 else out[..., k] + term
    return out


def resolve(samples: np.ndarray) -> np.ndarray:
    """samples[T, S2, npix, 3] -> frame[npix, 3]: per replica the strata in order, / spp, then the replicas in order."""
    T, S2 = samples.shape[:2]
    spp = float(T * S2)
    acc = np.zeros(samples.shape[2:], dtype=np.float64)
    for t in range(T):
        col = np.zeros(samples.shape[2:], dtype=np.float64)
        for st in range(S2):
            col = col + samples[t, st]
        acc = acc + col / spp
    return acc


def resolve_groups(samples: np.ndarray, gid: np.ndarray, n_groups: int) -> np.ndarray:
    """Group frames [G, npix, 3]: the same sums with every sample of another group replaced by +0.0."""
    return np.stack([resolve(np.where((gid == g)[..., None], samples, 0.0)) for g in range(n_groups)])


def sum_bound(sqrt_spt: int, thread_count: int, n_groups: int) -> float:
    """Property 4: |sum_g frame_g - frame| <= this * |frame| per channel (samples >= 0, finite pixels)."""
    return (sqrt_spt * sqrt_spt + thread_count + n_groups + 2) * EPS


def sum_in_group_order(groups: np.ndarray) -> np.ndarray:
    out = groups[0].copy()
    for g in range(1, groups.shape[0]):
        out = out + groups[g]
    return out


def assert_sum_property(groups: np.ndarray, frame: np.ndarray, sqrt_spt: int, thread_count: int) -> float:
    """Property 4 and the mask rule; returns the largest relative difference met."""
    G = groups.shape[0]
    total = sum_in_group_order(groups[..., :3])
    f = frame[..., :3]
    np.testing.assert_array_equal(~np.isfinite(groups[..., :3]).all(axis=0), ~np.isfinite(f))
    fin = np.isfinite(f)
    assert (f[fin] >= 0).all()
    diff = np.abs(total[fin] - f[fin])
    bound = sum_bound(sqrt_spt, thread_count, G) * np.abs(f[fin])
    worst = float((diff / np.maximum(np.abs(f[fin]), 1e-300)).max()) if fin.any() else 0.0
    print(f"sum of {G} groups vs frame: max relative difference {worst:.3e}, bound {sum_bound(sqrt_spt, thread_count, G):.3e}")
    assert (diff <= bound).all()
    return worst


class Zeroed:
    """Edits hs.desc in place: every Emissive material whose group is not `g` gets tex_a pointed at a constant-zero colour
    texture appended to the texture table; `params` loses its background when that is not in `g`.  restore() undoes it."""

    def __init__(self, hs, groups: api.RtLightGroups, g: int):
        d = hs.desc.contents
        self._d = d
        self._old = (d.textures, d.n_textures, [d.materials[i].tex_a for i in range(d.n_materials)])
        n = d.n_textures
        self._tex = (api.RtTexture * (n + 1))()
        if n:
            C.memmove(self._tex, d.textures, n * C.sizeof(api.RtTexture))
        zero = self._tex[n]
        zero.type = api.RT_TEX_CONST_COLOR
        zero.a = zero.b = zero.c = -1
        for k in range(3):
            zero.v[k] = 0.0
        d.textures = C.cast(self._tex, type(d.textures))
        d.n_textures = n + 1
        table = groups.table
        for i in range(d.n_materials):
            if d.materials[i].type == api.RT_MAT_EMISSIVE and int(table[i]) != g:
                d.materials[i].tex_a = n
        self.params = hs.params.copy()
        if self.params.has_background and groups.background_group != g:
            for k in range(3):
                self.params.background[k] = 0.0

    def restore(self):
        d = self._d
        d.textures, d.n_textures = self._old[0], self._old[1]
        for i, t in enumerate(self._old[2]):
            d.materials[i].tex_a = t
