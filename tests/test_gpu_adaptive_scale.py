"""The decision step of adaptive sampling (k_ad_quiet, k_ad_window, k_ad_scan, k_ad_scatter, k_ad_flags_from_counts in
rt_accum.hip) beyond one workgroup, with exact assertions: 515 x 257 pixels are 65 chunks of 2 048 list entries - a second
scan round, non-zero chunk offsets, a last chunk of 5 * 256 + 3 entries.

rt_accum_load_state takes the crafted states of tests/adaptive_state_cases.py (any keep pattern, no render needed); the
rule (tests/adaptive_ref.py) says which pixels have to be active afterwards, and one more replica shows the list itself:
exactly those pixels move on to the plain accumulator's next sum, bit for bit, and nothing else changes.  Then one state
is continued to the end, also through a pool smaller than the list, and a real render at this size is held to the prefix
property and the rule."""
import numpy as np
import pytest

import adaptive_ref as ar
import adaptive_state_cases as sc
from rust_raytracer_amd import api

pytestmark = pytest.mark.gpu

T = sc.T
REAL_ARGS = ["scenes/light_test", "-w=515", "-r=2", "-s=8", "-t=8", "--seed=82"]
REAL_THRESHOLD, REAL_RADIUS = 0.5, 1  # chosen from the reference alone: profiles/adaptive_scale/README.md


@pytest.fixture(scope="module")
def dev():
    lib = api.load_device_lib()
    assert lib.rt_device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return lib


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_same_bits(a, b, what=""):
    assert a.shape == b.shape
    diff = bits(a) != bits(b)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} doubles differ"


def params(threshold, radius):
    return api.RtAdaptiveParams.defaults(threshold=threshold, radius=radius, **sc.PARAMS)


def plain_snapshots(scene, hs):
    """sum_k (k = 0 .. T) of the plain accumulator, one replica per call."""
    pr = api.ProgressiveRender(scene, hs.camera, hs.params)
    snaps = [np.zeros((hs.height, hs.width, 4))]
    for _ in range(T):
        pr.render(1)
        blob = pr.save_state()
        assert len(blob) == 48 + hs.height * hs.width * 32
        snaps.append(np.frombuffer(blob, dtype=np.float64, offset=48).reshape(hs.height, hs.width, 4).copy())
    pr.close()
    snaps = np.stack(snaps)
    snaps.setflags(write=False)
    return snaps


def prefix_sums(snaps, n):
    return np.take_along_axis(snaps, n.astype(np.int64)[None, ..., None].repeat(4, axis=-1), axis=0)[0]


@pytest.fixture(scope="module")
def frame(dev):
    hs = api.HostScene(sc.ARGS)
    sc.check_frame(hs)
    return hs, api.DeviceScene(hs.desc, 0)


@pytest.fixture(scope="module")
def snaps(frame):
    hs, scene = frame
    return plain_snapshots(scene, hs)


@pytest.fixture(scope="module")
def templates(frame):
    """Per radius (it is part of the parameter block): the blob of a real adaptive accumulator after one replica - no
    decision has happened, and it carries the digests."""
    hs, scene = frame
    out = {}
    for radius in (0,) + sc.WINDOW_RADII:
        pr = api.ProgressiveRender(scene, hs.camera, hs.params, adaptive=params(sc.THRESHOLD, radius))
        pr.render(1)
        out[radius] = pr.save_state()
        assert sc.parse(out[radius])["k"] == 1
        pr.close()
    return out


def load_and_check(pr, scene, snaps, templates, name):
    """Loads the crafted state `name` into pr and holds it, and the replica after it, to the rule."""
    c, want = sc.case(name), sc.expected(name)
    k, n_want = c["k"], int(want.sum())
    blob = sc.craft(templates[c["radius"]], k, snaps[k], c["s1"], c["s2"], c["n"])
    pr.load_state(blob)
    assert pr.replicas_done == k
    assert pr.active_pixels == n_want
    np.testing.assert_array_equal(pr.sample_counts(), c["n"])
    assert pr.save_state() == blob
    assert pr.finished == (n_want == 0)
    pr.render(1)
    assert scene.stats().samples == n_want  # S^2 = 1
    after_blob = pr.save_state()
    if n_want == 0:
        assert pr.replicas_done == k and after_blob == blob, "nothing to render, yet the state changed"
        return
    st = sc.parse(after_blob)
    assert st["k"] == k + 1 == pr.replicas_done
    np.testing.assert_array_equal(st["n"], c["n"] + want.astype(np.uint32))
    assert_same_bits(st["sum"][want], snaps[k + 1][want], "sum on the active set")
    assert_same_bits(st["sum"][~want], snaps[k][~want], "sum off the active set")
    for key in ("s1", "s2"):
        assert_same_bits(st[key][~want], c[key][~want], key + " off the active set")
    y = ar.luminance(snaps[k + 1][want] - snaps[k][want], T)
    moments = {}
    for key, add in (("s1", y), ("s2", y * y)):
        got, ref = st[key][want], c[key][want] + add
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        np.testing.assert_allclose(got[~np.isnan(ref)], ref[~np.isnan(ref)], rtol=1e-9, atol=0)
        moments[key] = c[key].copy()
        moments[key][want] = ref
    # the replica may have ended at a decision point (route b: k + 1 = 4): the count of the decision taken there, up to
    # the pixels the reference moments put in the 1e-9 band (radius 0 on route b: nobody else depends on them)
    then = sc.expected_active(k + 1, moments["s1"], moments["s2"], st["n"], c["radius"])
    unsure = int(sc.band(k + 1, moments["s1"], moments["s2"], st["n"]).sum())
    assert unsure == 0 or c["radius"] == 0
    assert abs(pr.active_pixels - int(then.sum())) <= unsure


# ---- 1. every crafted state ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.NAMES)
def test_crafted_state_leaves_exactly_the_rules_pixels_active(frame, snaps, templates, name):
    hs, scene = frame
    pr = api.ProgressiveRender(scene, hs.camera, hs.params, adaptive=params(sc.THRESHOLD, sc.case(name)["radius"]))
    try:
        load_and_check(pr, scene, snaps, templates, name)
    finally:
        pr.close()


# ---- 2. reload: the second answer does not depend on the first ---------------------------------------------------------

@pytest.mark.parametrize("radius, names", [
    (0, ["a/all", "c/first-of-chunk", "a/none", "b/cycle", "c/half", "b/last-of-chunk", "a/one-before-round-border"]),
    (1, ["window/nan/r1", "window/row-end/r1", "window/stopped-noisy/r1", "window/corner-br/r1"]),
])
def test_one_accumulator_loads_one_state_after_another(frame, snaps, templates, radius, names):
    """state, keep and the list buffer that is not current still hold the previous state's data at every load."""
    hs, scene = frame
    pr = api.ProgressiveRender(scene, hs.camera, hs.params, adaptive=params(sc.THRESHOLD, radius))
    try:
        for name in names:
            load_and_check(pr, scene, snaps, templates, name)
    finally:
        pr.close()


# ---- 3. continuation --------------------------------------------------------------------------------------------------

def test_a_sparse_state_continues_to_the_end_as_the_rule_says_through_any_pool(frame, snaps, templates, monkeypatch):
    hs, _ = frame
    c = sc.case(sc.CONTINUATION)
    k, a0 = c["k"], c["n"] == c["k"]
    blob = sc.craft(templates[0], k, snaps[k], c["s1"], c["s2"], c["n"])
    ap = params(sc.THRESHOLD, 0)

    def run():
        scene = api.DeviceScene(hs.desc, 0)
        pr = api.ProgressiveRender(scene, hs.camera, hs.params, adaptive=ap)
        pr.load_state(blob)
        assert pr.active_pixels == int(sc.expected(sc.CONTINUATION).sum())
        pr.render(T)
        assert pr.finished and pr.replicas_done == T
        out = pr.save_state()
        pr.close()
        return out

    final = run()
    st = sc.parse(final)
    sim = ar.simulate(ar.contributions_from_snapshots(snaps), start=dict(k=k, n=c["n"], s1=c["s1"], s2=c["s2"], sum=snaps[k], active=a0),
                      **ar.params_of(ap))
    exempt = sim["exempt"]
    hist = dict(zip(*np.unique(sim["n"][a0], return_counts=True)))
    print(f"continuation of {sc.CONTINUATION}: n of the pixels active at the load {hist}, exempt {int(exempt.sum())} of {exempt.size}")
    assert set(hist) == {4, 6, 8}, "the reference must see pixels stop at the load, at k = 6 and never"
    assert exempt.mean() <= 0.005
    np.testing.assert_array_equal(st["n"][~exempt], sim["n"][~exempt])
    np.testing.assert_array_equal(st["n"][~a0], c["n"][~a0])
    assert_same_bits(st["sum"][a0], prefix_sums(snaps, st["n"])[a0], "sum of the pixels active at the load")
    assert_same_bits(st["sum"][~a0], snaps[k][~a0], "sum of the others")
    same = st["n"] == sim["n"]
    for key in ("s1", "s2"):
        assert_same_bits(st[key][~a0], c[key][~a0], key + " of the others")
        np.testing.assert_allclose(st[key][same & a0], sim[key][same & a0], rtol=1e-9, atol=0)
    # a pool of about one segment's samples (two replicas of ~24 000 listed pixels), and one an eighth of the list: the
    # sparse pass refills its pool many times over
    for pool in ("50000", "3000"):
        monkeypatch.setenv("RT_WF_POOL", pool)
        assert run() == final, "RT_WF_POOL=" + pool
    monkeypatch.delenv("RT_WF_POOL")


# ---- 4. a real render at this size ---------------------------------------------------------------------------------------

def test_real_render_keeps_the_prefix_property_and_the_rule_at_65_chunks(dev):
    hs = api.HostScene(REAL_ARGS)
    assert (hs.width, hs.height, hs.params.thread_count) == (sc.W, sc.H, T)
    scene = api.DeviceScene(hs.desc, 0)
    real_snaps = plain_snapshots(scene, hs)
    ap = params(REAL_THRESHOLD, REAL_RADIUS)
    # the case is judged by the reference, not by the code under test
    sim = ar.simulate(ar.contributions_from_snapshots(real_snaps), **ar.params_of(ap))
    shares = {int(v): round(float((sim["n"] == v).mean()), 4) for v in np.unique(sim["n"])}
    exempt = sim["exempt"]
    print(f"light_test at threshold {REAL_THRESHOLD}, radius {REAL_RADIUS}: reference n shares {shares}, exempt {int(exempt.sum())} of {exempt.size}")
    assert 0.10 <= (sim["n"] < T).mean() <= 0.95 and set(shares) == {2, 4, 6, 8}
    assert exempt.mean() <= 0.005

    def run(split):
        pr = api.ProgressiveRender(scene, hs.camera, hs.params, adaptive=ap)
        for m in split:
            pr.render(m)
        out = pr.save_state()
        assert pr.finished
        pr.close()
        return out

    blob = run([T])
    st = sc.parse(blob)
    n = st["n"]
    assert set(np.unique(n)) <= set(sc.D) | {T}
    assert_same_bits(st["sum"], prefix_sums(real_snaps, n), "prefix property")
    nan = np.isnan(st["sum"][..., :3]).any(axis=-1)
    assert (n[nan] == T).all(), "a pixel whose sum holds a NaN never stops"
    np.testing.assert_array_equal(n[~exempt], sim["n"][~exempt])
    same = n == sim["n"]
    for key in ("s1", "s2"):
        a, b = st[key][same], sim[key][same]
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        fin = ~np.isnan(b)
        np.testing.assert_allclose(a[fin], b[fin], rtol=1e-9, atol=0)
    assert run([1] * T) == blob
