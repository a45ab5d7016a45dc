"""The yardstick and the ray sets of tests/special_ray_cases.py, without a GPU.

1. pyoracle.world_hits(unculled=True) changes culling and nothing else: on every ray set of ray_query_cases.cases(name), none of
   which is in special position, it gives the bytes of pyoracle.world_hit, ray by ray.
2. On the dyadic mesh families an exact reference (Moeller-Trumbore over all triangles in rational arithmetic,
   special_ray_cases.exact_mesh_hits) agrees with the unculled oracle with `==` in t and position, and the oracle's `near` is
   the exact number of ties.  That checks the oracle and proves that these inputs are free of rounding.
3. The sets are not vacuous, as conditions on the oracles alone."""
import numpy as np
import pytest

from oracle import pyoracle
from ray_query_cases import MISS, SURFACE, T_MAX, T_MIN, cases, oracle_hits
import special_ray_cases as sc

ORACLE_SCENES = ["cornell", "two_meshes", "nested_transform", "sun_sky", "sphere_field", "hollow_glass", "light_test", "texture_mix"]


@pytest.mark.parametrize("name", ORACLE_SCENES)
def test_unculled_changes_nothing_in_general_position(name):
    c = cases(name)
    desc = c.hs.desc
    for o, d, want, lo, hi in ((c.ab_o, c.ab_d, c.ab_hits, T_MIN, np.inf),
                               (c.seg_o, c.seg_d, oracle_hits(desc, c.seg_o, c.seg_d, T_MIN, T_MAX), T_MIN, T_MAX)):
        for unculled in (False, True):   # False: the batch entry itself against the single-ray one
            got = sc.expected(*pyoracle.world_hits(desc, o, d, lo, hi, unculled=unculled))
            assert got.tobytes() == want.tobytes(), f"unculled={unculled}"
        _, near = pyoracle.world_hits(desc, o, d, lo, hi, unculled=True)
        np.testing.assert_array_equal(near > 0, want["klass"] != MISS)


@pytest.mark.parametrize("name", sc.MESH_SCENES)
def test_exact_reference_agrees_with_unculled_oracle(name):
    c = sc.case(name)
    for f in sc.MESH_FAMILIES:
        r = c.families[f]
        want, near = c.want(f)
        sel = np.flatnonzero(r.dyadic)
        sel = sel[sc._thin(len(sel), 1500)]
        exact = sc.exact_mesh_hits(c.desc, r.o[sel], r.d[sel])
        for i, (t, pos, n_ties, _, _) in zip(sel, exact):
            w = want[i]
            if t is None:
                assert w["klass"] != SURFACE and near[i] == (1 if w["klass"] != MISS else 0), f"{name} {f} ray {i}"
                continue
            assert w["klass"] == SURFACE, f"{name} {f} ray {i}: the oracle misses an exact hit at t = {float(t)}"
            # the oracle's doubles ARE the rationals: nothing was rounded
            assert sc.Fraction(float(w["t"])) == t, f"{name} {f} ray {i}: t"
            assert all(sc.Fraction(float(w["pos"][a])) == pos[a] for a in range(3)), f"{name} {f} ray {i}: pos"
            assert near[i] == n_ties, f"{name} {f} ray {i}: near = {near[i]}, exact ties {n_ties}"


@pytest.mark.parametrize("kind", sc.MESHES)
def test_mesh_families_not_vacuous(kind):
    ties = {f: 0 for f in sc.MESH_FAMILIES}
    for name in (kind, kind + "_moved", kind + "_twice"):
        c = sc.case(name)
        for f in sc.MESH_FAMILIES:
            r = c.families[f]
            want, near = c.want(f)
            plain, _ = c.plain(f)
            dropped = int(((plain["klass"] != SURFACE) & (want["klass"] == SURFACE)).sum())
            differ = int(sum(a.tobytes() != b.tobytes() for a, b in zip(plain, want)))
            print(f"{name} ({f}): {len(r)} rays, {int((want['klass'] == SURFACE).sum())} surface hits, the plain oracle answers "
                  f"{differ} differently and drops {dropped}, {int((near > 1).sum())} ties, {int(((near == 1) & (want['klass'] == SURFACE)).sum())} surface hits without a tie")
            assert len(r) <= 5000
            ties[f] += int((near > 1).sum())
            # culling can only lose hits: the unculled hit is never farther (with two instances the plain one may be the second mesh)
            assert (want["t"] <= plain["t"]).all()
            if f in ("a", "b", "c"):
                assert (want["klass"] == SURFACE).mean() >= 0.5
                assert (near > 1).any() and ((near == 1) & (want["klass"] == SURFACE)).any()
            if f in ("a", "b") and kind in ("G", "C"):
                assert dropped > 0, "the axis family holds no ray that the reference's octree drops"
    # (d) and (e) hit nothing on a bare open mesh (in its plane: det = 0; from its surface: t = 0), so their ties are asked of
    # the three scenes of a mesh together
    assert all(n > 0 for n in ties.values()), ties


def test_octree_drops_the_centre_column_of_the_grid():
    """The measurement that set this work off: straight down through the 289 vertices of G, the reference's octree answers the
    17 of the column x = 0 with the sky."""
    c = sc.case("G")
    i, j = np.meshgrid(np.arange(17), np.arange(17), indexing="ij")
    p = np.stack([-1 + i.ravel() / 8, np.zeros(289), -1 + j.ravel() / 8], axis=1)
    for d in ([0.0, -1.0, 0.0], [-0.0, -1.0, -0.0], [0.0, -2.0 ** -40, 0.0]):
        o = p + np.array([0.0, 1.0, 0.0])
        plain = sc.expected(*pyoracle.world_hits(c.desc, o, np.tile(d, (289, 1))))
        want = sc.expected(*pyoracle.world_hits(c.desc, o, np.tile(d, (289, 1)), unculled=True))
        assert (want["klass"] == SURFACE).all() and (want["t"] * -d[1] == 1.0).all()
        lost = plain["klass"] != SURFACE
        assert lost.sum() == 17 and (p[lost, 0] == 0).all()


def test_sphere_scene_not_vacuous():
    c = sc.case("S")
    for f in ("s", "f"):
        want, near = c.want(f)
        plain, _ = c.plain(f)
        assert want.tobytes() == plain.tobytes()      # no mesh: nothing to drop
        assert (near <= 1).all()
    want, _ = c.want("s")
    r = c.families["s"]
    assert len(r) <= 6000 and (want["klass"] == SURFACE).mean() >= 0.5
    assert len({int(m) for m in want["material"][want["klass"] == SURFACE]}) == 4
    # exact distances on the big sphere: offsets 3 and 4 from 16 away along an axis, tangent rays at 5 and (3, 4)
    big = np.array(sc.BIG[0])
    base = len(r) // 3
    off2 = (np.cross(r.o[:base] - big, r.d[:base]) ** 2).sum(axis=1)
    first = want[:base]
    for dist, t in ((0.0, 11.0), (3.0, 12.0), (4.0, 13.0), (5.0, 16.0)):
        sel = (off2 == dist * dist) & (np.abs(r.d[:base]).sum(axis=1) == 1) & (((r.o[:base] - big) ** 2).sum(axis=1) == 256 + dist * dist)
        assert sel.sum() >= 6 and (first["t"][sel] <= t).all() and (first["t"][sel] == t).sum() >= 2, (dist, first["t"][sel])
    # quads hit exactly on their rims and corners
    surf = want["klass"] == SURFACE
    assert ((want["u"][surf] == 0) | (want["u"][surf] == 1)).sum() >= 50 and ((want["v"][surf] == 0) | (want["v"][surf] == 1)).sum() >= 50
    # (f): rays on a guard plane that the reference drops and that hit once the origin moves by one ulp
    r = c.families["f"]
    want, _ = c.want("f")
    assert len(r) <= 5000
    lost = np.flatnonzero(want["klass"] != SURFACE)
    found = 0
    for sign in (-np.inf, np.inf):
        o = r.o[lost].copy()
        # the axis whose direction component is a signed zero and whose origin coordinate is the plane: move along each zero axis
        for a in range(3):
            z = r.d[lost][:, a] == 0
            o2 = o.copy()
            o2[z, a] = np.nextafter(o[z, a], sign)
            moved = sc.unculled_hits(c.desc, o2, r.d[lost])
            found += int(((moved["klass"] == SURFACE) & z).sum())
    print(f"S (f): {len(r)} rays, {len(lost)} without a surface hit, {found} (ray, one-ulp move) pairs that hit")
    assert found >= 10
    assert (want["klass"] == SURFACE).any()


@pytest.mark.parametrize("name", sc.MESH_SCENES + ("S",))
def test_f32_sets_stay_under_the_cap_on_the_oracle_alone(name):
    """The share of rays (segments) of the f32 sets with a copy that the unculled oracle answers differently bounds what the f32
    rule can excuse; it must stay under the cap whatever the kernels do.  The rule also passes the oracle's own answers."""
    import f32_ray_bounds as fb
    c = sc.case(name)
    geom, o, d, want, so, sd, hi, occ = sc.f32_set(name)
    closest = fb.fragile_share_closest(geom, o, d, want, c.extent(), oracle=lambda dsc, oo, dd, lo: sc.unculled_hits(dsc, oo, dd, lo))
    segments = fb.fragile_share_segments(geom, so, sd, occ, T_MIN, hi, hi, oracle=sc.unculled_hits)
    print(f"{name}: {len(o)} rays, {closest:.2%} with a copy that differs; {len(so)} segments, {segments:.2%}")
    assert closest <= fb.CAP / 2 and segments <= fb.CAP / 2
    assert (want["klass"] == SURFACE).mean() >= 0.3 and occ.mean() >= 0.2 and (~occ).mean() >= 0.2
    if name != "D_twice":   # locate() cannot tell D's coincident copies apart
        fb.check_closest(geom, o, d, fb.as_ray_hits(geom, want), want, c.extent(), name + " (the oracle's own answers)",
                         oracle=lambda oo, dd: sc.unculled_hits(c.desc, oo, dd)).check(k_pos=0.0, k_dir=0.0)
