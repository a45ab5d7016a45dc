"""A per-vertex yardstick for what the f32 kernels do at ONE path vertex - search, hit resolution, textures, material, light
sampling and weight (tests/test_f32_shade_bounds_host.py, tests/test_gpu_f32_shade.py).  The device side is
rt_debug_shade_rays, the oracle side pyoracle.shade_rays: one level of ray_color from a ray and a generator state.

Like tests/f32_ray_bounds.py an f32 answer is modelled as the EXACT answer to a slightly moved problem, with its u = 2^-24, its
L per ray, delta = 8 u L and its eight moved copies of a ray.  Every vertex has nine oracle answers, all from the same
generator state and with 24-bit draws (the oracle's uniform() keeps the top 24 bits of a draw exactly as rng_uniform<float>
does, so the draws are the device's and only arithmetic differs): R0 for the ray itself, R1..R8 for its copies.

  fit        the discrete outcome of a vertex is (material, front face, outcome class, generator state after - that is the number
             of draws - and which channels of the weight and the radiance are finite, NaN, +inf or -inf: a light sampled from
             a point on its own surface gives 0/0 for the ray and a finite weight for a copy).  If the f32 outcome equals
             R0's, closeness is checked; else if it equals some Rk's the vertex is EXCUSED (edges of geometry, texels, checker
             cells, the sphere seam, Schlick coins, the TIR test, the absorbed test and the free flight against the boundary
             all depend on the ray, so the copies flip them); else the vertex fails.
  closeness  for the unit continuation direction (as an angle) and each channel of tex_a, weight and radiance:
             |q32 - q0| <= K_q (S_q + u |q0|), S_q = the largest |q_k - q0| over the copies whose discrete outcome equals
             R0's: the oracle's own sensitivity to a perturbation of f32 size, a finite-difference condition number (large near
             TIR, at grazing cosines, next to a light, on steep noise; zero for a constant albedo).  Where q0 is NaN or
             infinite (a zero pdf, the reference's 0/0) the f32 value must be of the same kind.
  self-lit   a diffuse vertex ON a member of the light list (the glossy ball of tests/scenes/nested_lights) whose direction is
             sampled from the lights, or on the member's inside, meets that member from its own surface: sphere.rs:106-145
             takes sqrt(1 - r^2 / d^2) with d = r up to the rounding of the hit position, so NaN or not is decided by the last bit of the position - in f64 too, and no moved RAY reproduces the
             other answer, because every copy's hit lies on the surface as exactly.  There the kinds of the weight are no part
             of the outcome; a vertex whose weight is of another kind than R0's is excused, and every self-lit vertex counts
             towards the share that can be excused.  Its weight, where finite, is the quotient by a pdf taken a few ulps from
             that singularity: it is not held to the closeness bound and stays out of the measurement of K (its direction,
             tex_a and radiance are held like any other vertex's).  Self-lit goes by MATERIAL: a primitive that shares its
             material with a member of the light list counts as one.
  CAP        at most 10 % of a set may be excused: a condition, not a measurement.

The outcome class of a DEVICE answer is not a field of the probe (shade() does not report it); classes_of() derives it from
what the probe does report: the material's type, whether the path continues, the side of the surface the direction lies on,
the number of draws, and - for the light / material coin of MixPDF - the draw itself, replayed from the generator state.

K[quantity][class] is the smallest power of two that is at least 4 times the largest ratio measured on the MI355X against the
oracle over all sets of tests/test_gpu_f32_shade.py (DESIGN.md section 14 has the table; the kernels are deterministic, the
factor covers a later compiler that reorders f32 arithmetic)."""
import numpy as np

from oracle import pyoracle
from rust_raytracer_amd import api
import f32_ray_bounds as fb
from f32_ray_bounds import CAP, DELTA, U

GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
CLASSES = pyoracle.SHADE_CLASSES
BACKGROUND, EMITTED, ABSORBED, REFLECT, REFRACT, PDF_LIGHT, PDF_MATERIAL, VOLUME = range(8)
CONTINUING = (REFLECT, REFRACT, PDF_LIGHT, PDF_MATERIAL, VOLUME)
QUANTITIES = ("direction", "tex_a", "weight", "radiance")
# record slots (include/rt_mi355.h, rt_debug_shade_rays)
T, POS, NORMAL, UU, VV, FRONT, MATERIAL, OP, TEX_A, TEX_B, CONT, DIR, WEIGHT, RADIANCE, SEARCH_DRAWS = (
    0, slice(1, 4), slice(4, 7), 7, 8, 9, 10, 11, slice(12, 15), 15, 16, slice(17, 20), slice(20, 23), slice(23, 26), 26)

# MEASURED_RATIOS[quantity][class]: the largest ratio over all sets of tests/test_gpu_f32_shade.py on the MI355X (both variants)
# (set and vertex of each in DESIGN.md section 14).  A class that is absent was exact on every vertex: ratio 0.
MEASURED_RATIOS = {
    "direction": {"pdf_light": 12.4, "pdf_material": 6.66, "reflect": 16.5, "refract": 5.12, "volume": 11.9},
    "tex_a": {"absorbed": 1.71, "emitted": 0.667, "pdf_light": 15, "pdf_material": 16, "reflect": 3.29, "volume": 0.667},
    # pdf_light, the one class above 2^10: vertex 973 of cornell lies on the ceiling (y = 555) and samples the lamp 0.1 below it
    # (y = 554.9).  plane.rs:120-126 forms pt - origin; its y is -0.1 with the rounding of 554.9 (f32 ulp 6.1e-5) in it, 3e-4
    # relative, the direction makes cos = 6.7e-4 with both normals, and the weight goes with cos^2.  No moved ray changes the 0.1.
    # Self-lit vertices are not in these figures (see above).
    "weight": {"pdf_light": 257, "pdf_material": 111, "reflect": 0.667, "volume": 2.46},
    "radiance": {"emitted": 1.16},
}


def _k_of(ratio):
    """The smallest power of two that is at least 4 x ratio (1 for a ratio of 0: any bound holds an exact value)."""
    return 1.0 if ratio <= 0.25 else 2.0 ** int(np.ceil(np.log2(4.0 * ratio)))


K = {q: {c: _k_of(MEASURED_RATIOS[q].get(c, 0.0)) for c in CLASSES} for q in QUANTITIES}


# ---- the generator on the host (rt_device.h Rng; oracle.cpp Rng) ----
def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draws_between(s0, s1):
    """Number of draws that take state s0 to s1, or None if s1 is not on s0's sequence within 2^20 draws."""
    d = (int(s1) - int(s0)) & M64
    k = (d * pow(GOLDEN, -1, 1 << 64)) & M64
    return k if k < (1 << 20) else None


def uniform_at(state, k, draws24):
    """The k-th (1-based) uniform draw after `state`."""
    x = _mix((int(state) + k * GOLDEN) & M64)
    return (x >> 40) / 16777216.0 if draws24 else (x >> 11) / 9007199254740992.0


def classes_of(desc, params, rec, st_in, st_out, draws24):
    """The outcome class of each answer (n, 28) in the probe's layout, derived from the probe's own fields.  Reflect / refract
    of a Dielectric is the side of the surface the direction lies on (the oracle's class is formed the same way, not from the
    branch taken).  Known blind spot: a diffuse Glossy vertex that makes exactly seven draws (a light list nested three deep)
    AND whose weight is exactly (1, 1, 1) would be taken for a specular one.  tests/test_f32_shade_bounds_host.py holds this
    derivation to the oracle's classes on every set."""
    mats = desc.contents.materials
    bias = float(np.float32(params.light_bias)) if draws24 else float(params.light_bias)
    out = np.zeros(len(rec), dtype=np.int64)
    for i, r in enumerate(rec):
        m = int(r[MATERIAL])
        if m < 0:
            out[i] = BACKGROUND
            continue
        ty, cont = mats[m].type, r[CONT] != 0
        if ty in (api.RT_MAT_EMISSIVE, api.RT_MAT_NORMAL_DEBUG):
            out[i] = EMITTED
        elif ty == api.RT_MAT_ISOTROPIC:
            out[i] = VOLUME
        elif ty == api.RT_MAT_METAL:
            out[i] = REFLECT if cont else ABSORBED
        elif ty == api.RT_MAT_DIELECTRIC:
            out[i] = REFRACT if float(np.dot(r[DIR], r[NORMAL])) < 0.0 else REFLECT
        else:
            first = int(r[SEARCH_DRAWS]) + 1   # the first draw of shade()
            if ty == api.RT_MAT_GLOSSY:
                # specular: the Schlick coin and the six draws of the fuzz, and the weight stays (1, 1, 1) whether the direction is
                # kept or absorbed; else coin, mix coin, ... and a weight that is (1, 1, 1) by accident only
                n = draws_between(st_in[i], st_out[i])
                if n == first + 6 and (r[WEIGHT] == 1.0).all():
                    out[i] = REFLECT if cont else ABSORBED
                    continue
                first += 1
            out[i] = PDF_LIGHT if uniform_at(st_in[i], first, draws24) < bias else PDF_MATERIAL
    return out


# ---- the nine oracle answers ----
class Answers:
    """R0 and R1..R8 of a set of vertices: rec[k] (n, 28), state[k] (n,), klass[k] (n,), k = 0..8."""

    def __init__(self, rec, state, lit_materials=()):
        self.rec, self.state = rec, state
        self.klass = rec[:, :, OP].astype(np.int64)
        # self-lit: R0 is a vertex on a member of the light list whose direction can meet that member again - sampled from the
        # lights, or sampled on the member's inside (a cosine-sampled direction on the outside of a sphere or quad leaves it)
        k0 = self.klass[0]
        self.self_lit = np.isin(rec[0, :, MATERIAL].astype(np.int64), list(lit_materials)) & \
            ((k0 == PDF_LIGHT) | ((k0 == PDF_MATERIAL) & (rec[0, :, FRONT] == 0)))

    def key(self, k, i):
        return outcome(self.rec[k, i], self.klass[k, i], self.state[k, i], not self.self_lit[i])

    def fragile(self):
        """Per vertex: its nine answers do not all agree discretely - the most that can ever be excused."""
        n = self.rec.shape[1]
        return np.array([any(self.key(k, i) != self.key(0, i) for k in range(1, 9)) for i in range(n)]) | self.self_lit


def light_member_materials(desc):
    """Materials of the primitives reachable from the light list."""
    d = desc.contents
    out, todo = set(), [d.lights_root]
    while todo:
        node = d.nodes[todo.pop()]
        if node.n_children:
            todo += [d.child_indices[node.first_child + k] for k in range(node.n_children)]
        elif node.material >= 0:
            out.add(int(node.material))
    return out


def _kinds(v):
    return tuple(1 if np.isnan(x) else (2 if x == np.inf else (3 if x == -np.inf else 0)) for x in v)


def outcome(r, klass, state, weight_kinds=True):
    """The discrete outcome of an answer.  A continuing class that does not continue is the kernels' early end of a path whose
    weight is zero or NaN in every channel (path_goes_on): its radiance is that weight, the oracle's is zero."""
    ended = int(klass) in CONTINUING and r[CONT] == 0
    return (int(r[MATERIAL]), bool(r[FRONT]), int(klass), int(state), _kinds(r[WEIGHT]) if weight_kinds else None,
            (0, 0, 0) if ended else _kinds(r[RADIANCE]))


def scales(geom, o, r0, extent):
    """(L, t_point) per ray, after f32_ray_bounds.ray_scale: L from the origin, the oracle's hit position and the numbers of
    the primitive nearest to it (a volume's vertex lies inside its boundary: the nearest primitive of any material)."""
    L, tp = np.zeros(len(o)), np.zeros(len(o))
    for i in range(len(o)):
        t = r0[i, T]
        if r0[i, MATERIAL] < 0 or not t < fb.FLT_MAX:
            L[i], tp[i] = max(float(np.abs(o[i]).max()), extent), -1.0
            continue
        pos = r0[i, POS]
        e, prim, _ = geom.locate(pos, int(r0[i, MATERIAL]))
        if e is None:
            e, prim, _ = geom.locate(pos)
        L[i] = max(float(np.abs(o[i]).max()), float(np.abs(pos).max()), float(np.abs(geom.numbers(e, prim)).max()))
        tp[i] = t
    return L, tp


def oracle_answers(desc, params, geom, o, d, states, extent):
    """The nine answers with 24-bit draws: two batched oracle calls (the world is built once per call)."""
    n = len(o)
    r0, s0 = pyoracle.shade_rays(desc, params, o, d, states, draws24=True)
    L, tp = scales(geom, o, r0, extent)
    co, cd = np.zeros((n, 8, 3)), np.zeros((n, 8, 3))
    for i in range(n):
        t_point = tp[i] if tp[i] > 0 else extent / np.linalg.norm(d[i])
        co[i], cd[i] = fb.copies(o[i], d[i], t_point, DELTA * U * L[i])
    rk, sk = pyoracle.shade_rays(desc, params, co.reshape(-1, 3), cd.reshape(-1, 3), np.repeat(states, 8), draws24=True)
    rec = np.concatenate([r0[None], rk.reshape(n, 8, -1).transpose(1, 0, 2)])
    state = np.concatenate([s0[None], sk.reshape(n, 8).T])
    return Answers(rec, state, light_member_materials(desc))


# ---- the rule ----
def _unit_rows(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _angle(a, b):
    """Angle between unit vectors, accurate for small angles."""
    return 2.0 * np.arctan2(np.linalg.norm(a - b, axis=-1), np.linalg.norm(a + b, axis=-1))


def _same_kind(x, y):
    return (np.isnan(x) and np.isnan(y)) or (np.isinf(x) and x == y)


class Report:
    def __init__(self, label, n):
        self.label, self.n = label, n
        self.excused, self.failures = [], []
        self.ratio = {q: {} for q in QUANTITIES}   # [quantity][class name] = (largest ratio, vertex)
        self.checked = 0

    @property
    def share(self):
        return len(self.excused) / max(self.n, 1)

    def _note(self, q, klass, ratio, i):
        name = CLASSES[klass]
        if ratio > self.ratio[q].get(name, (-1.0, -1))[0]:
            self.ratio[q][name] = (float(ratio), i)

    def line(self):
        parts = []
        for q in QUANTITIES:
            cells = ", ".join(f"{c} {r:.3g}@{i}" for c, (r, i) in sorted(self.ratio[q].items()) if r > 0)
            parts.append(f"{q}: {cells or '0'}")
        return (f"{self.label}: {self.n} vertices, {len(self.excused)} excused ({self.share:.2%}), {len(self.failures)} failures; "
                "largest ratios " + "; ".join(parts))

    def check(self, k=None, show=True):
        """Prints the figures, then asserts: nothing failed, the excused share is at most CAP, the ratios are within K (k: one
        number for every quantity and class, in place of K)."""
        if show:
            print(self.line())
        assert not self.failures, f"{self.label}: {len(self.failures)} vertices fail, first: {self.failures[:5]}"
        assert self.share <= CAP, f"{self.label}: {self.share:.2%} of the vertices excused, cap {CAP:.0%}"
        for q in QUANTITIES:
            for name, (r, i) in self.ratio[q].items():
                bound = K[q][name] if k is None else k
                assert r <= bound, f"{self.label}: {q} of a {name} vertex ({i}): ratio {r:.4g} > {bound}"
        return self


def check(answers, got, got_state, got_klass, label):
    """The rule on the f32 answers `got` (n, 28; the probe's layout), their generator states and classes (classes_of)."""
    n = answers.rec.shape[1]
    assert got.shape == (n, answers.rec.shape[2]) and len(got_state) == n and len(got_klass) == n
    rep = Report(label, n)
    for i in range(n):
        g = got[i]
        key = outcome(g, got_klass[i], got_state[i], not answers.self_lit[i])
        key0 = answers.key(0, i)
        if key == key0 and answers.self_lit[i] and _kinds(g[WEIGHT]) != _kinds(answers.rec[0, i, WEIGHT]):
            rep.excused.append(i)
            continue
        same = [k for k in range(1, 9) if answers.key(k, i) == key0]
        if key != key0:
            if any(answers.key(k, i) == key for k in range(1, 9)):
                rep.excused.append(i)
            else:
                rep.failures.append((i, f"outcome {key} fits neither the oracle's {key0} nor a copy's"))
            continue
        rep.checked += 1
        klass = key0[2]
        r0, rk = answers.rec[0, i], answers.rec[same, i]
        cont = g[CONT] != 0
        if klass in CONTINUING and not cont:
            # the kernels end a path whose weight is zero or NaN in every channel (path_goes_on): the radiance is that weight
            w = g[WEIGHT]
            if not ((w == 0).all() or np.isnan(w).all()) or not all(_same_kind(a, b) or a == b for a, b in zip(g[RADIANCE], w)):
                rep.failures.append((i, f"a {CLASSES[klass]} vertex ends with weight {w} and radiance {g[RADIANCE]}"))
                continue
        elif cont != (klass in CONTINUING):
            rep.failures.append((i, f"a {CLASSES[klass]} vertex with continues = {cont}"))
            continue
        columns = []   # (quantity, the f32 value, R0's, the copies')
        if klass in CONTINUING and cont:
            d0, dk, dg = _unit_rows(r0[DIR]), _unit_rows(rk[:, DIR]), _unit_rows(g[DIR])
            if not np.isfinite(d0).all() or not np.isfinite(dg).all():
                if _kinds(d0) != _kinds(dg):
                    rep.failures.append((i, f"direction {g[DIR]} against the oracle's {r0[DIR]}"))
                    continue
            else:
                dk = dk[np.isfinite(dk).all(axis=-1)]
                s = float(_angle(dk, d0).max()) if len(dk) else 0.0
                rep._note("direction", klass, float(_angle(dg, d0)) / (s + U), i)
        for q, sl in (("tex_a", TEX_A), ("weight", WEIGHT), ("radiance", RADIANCE)):
            if q == "radiance" and klass in CONTINUING and not cont:
                continue
            if q == "weight" and answers.self_lit[i] and np.isfinite(r0[sl]).all() and np.isfinite(g[sl]).all():
                continue
            for c in range(3):
                columns.append((q, g[sl][c], r0[sl][c], rk[:, sl][:, c]))
        for q, x, x0, xk in columns:
            if not np.isfinite(x0) or not np.isfinite(x):
                if not _same_kind(x, x0):
                    rep.failures.append((i, f"{q} {x} against the oracle's {x0}"))
                continue
            xk = xk[np.isfinite(xk)]   # tex_a is no part of the outcome
            s = float(np.abs(xk - x0).max()) if len(xk) else 0.0
            den = s + U * abs(x0)
            diff = abs(x - x0)
            ratio = 0.0 if diff == 0 else (np.inf if den == 0 else diff / den)
            rep._note(q, klass, ratio, i)
    return rep
