"""The crafted states of tests/adaptive_state_cases.py without a GPU: the blobs are well formed and loadable, the catalogue
reaches the sizes and per-chunk counts it claims with nothing near the 1e-9 band, and it can tell a wrong decision step
from a right one: a numpy model of the step (quiet, window, per-chunk counts, scan, scatter as rt_accum.hip lays them out)
agrees with the rule on every case, and with any one of a list of faults switched on it disagrees on a named case."""
import os
import re
import struct

import numpy as np

import adaptive_ref as ar
import adaptive_state_cases as sc
from rust_raytracer_amd import api

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCUM_HIP = os.path.join(REPO, "rust_raytracer_amd", "csrc", "rt_accum.hip")
CHUNK, ROUND = sc.AD_CHUNK, sc.SCAN_ROUND


def test_frame_is_what_the_catalogue_assumes():
    sc.check_frame(api.HostScene(sc.ARGS))
    assert sc.D == [2, 4, 6]


def test_kernels_still_use_the_chunk_and_round_the_catalogue_is_sized_for():
    text = open(ACCUM_HIP).read()
    assert "constexpr uint32_t AD_CHUNK = %d" % CHUNK in text
    assert re.search(r"for \(uint32_t b0 = 0; b0 < n_blocks; b0 \+= %d\)" % ROUND, text), "k_ad_scan: counts per round"


def fake_template():
    head = b"RTACCUM\0" + struct.pack("<IIIIII", 2, 0, sc.W, sc.H, sc.T, 1) + struct.pack("<QQ", 0x1122334455667788, 0x99AABBCCDDEEFF00)
    par = struct.pack("<ddIIII", sc.THRESHOLD, sc.PARAMS["floor"], sc.PARAMS["min_replicas"], sc.PARAMS["check_interval"], 1, 0)
    assert len(head) == sc.HEADER and len(par) == sc.PARAM_BYTES
    return head + par + bytes(sc.NPIX * 52)


def local_parse(blob):
    """The layout once more, independent of sc.parse: header, parameters, sum, s1, s2, n."""
    np_ = sc.NPIX
    body = memoryview(blob)[80:]
    return (struct.unpack_from("<I", blob, 28)[0], np.frombuffer(body[:np_ * 32], dtype="<f8"), np.frombuffer(body[np_ * 32:np_ * 40], dtype="<f8"),
            np.frombuffer(body[np_ * 40:np_ * 48], dtype="<f8"), np.frombuffer(body[np_ * 48:], dtype="<u4"))


def test_craft_round_trips_and_every_count_is_loadable():
    template = fake_template()
    total = np.random.default_rng(5).uniform(0, 1, (sc.H, sc.W, 4))
    for name in sc.NAMES:
        c = sc.case(name)
        blob = sc.craft(template, c["k"], total, c["s1"], c["s2"], c["n"])
        assert len(blob) == len(template) and blob[:28] == template[:28] and blob[32:80] == template[32:80], name
        k, total_, s1, s2, n = local_parse(blob)
        assert k == c["k"]
        for got, want in ((total_, total), (s1, c["s1"]), (s2, c["s2"])):
            assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).reshape(-1).view(np.uint64)), name
        assert np.array_equal(n, c["n"].reshape(-1))
        p = sc.parse(blob)
        assert p["k"] == k and np.array_equal(p["n"], c["n"]) and np.array_equal(p["s1"].view(np.uint64), c["s1"].view(np.uint64))
        # accum_check_state: a count is replicas_done, or smaller and a decision point
        dp = np.isin(n, [2, 4, 6]) & (n < sc.T)
        ok = (n == k) | ((n < k) & dp)
        assert ok.all() and sc.counts_are_loadable(k, n), name


def test_catalogue_hits_what_it_claims():
    assert len(set(sc.NAMES)) == len(sc.NAMES)
    assert sc.NPIX > ROUND * CHUNK and sc.NPIX - ROUND * CHUNK == 1283
    seen = set()
    for name in sc.NAMES:
        c = sc.case(name)
        want = sc.expected(name)
        assert np.array_equal(want, c["want"]), name + ": the rule does not give the set the case was built for"
        assert not sc.band(c["k"], c["s1"], c["s2"], c["n"]).any(), name + ": a pixel in the 1e-9 band"
        counts = sc.chunk_counts(c["stay"])
        if name.split("/")[0] in ("a", "b") or name.startswith("window/"):
            assert counts.size == ROUND + 1, name            # a second scan round
        if name.startswith("c/"):
            m = int((c["n"] == 4).sum())
            assert c["stay"].size == m and abs(m / sc.NPIX - 0.37) < 0.01 and m % CHUNK % 256 != 0
        pattern = name.split("/")[1]
        if pattern == "cycle":
            seen |= set(counts.tolist())
            assert name.startswith("c/") or counts[ROUND] == 65
        elif pattern == "all":
            assert want.sum() == c["stay"].size and counts[-1] == c["stay"].size % CHUNK
        elif pattern == "none":
            assert not want.any()
        elif pattern == "first-of-chunk":
            assert (counts == 1).all() and c["stay"][::CHUNK].all()
        elif pattern == "last-of-chunk":
            assert (counts == 1).all() and c["stay"][-1] and c["stay"][CHUNK - 1::CHUNK].all()
        elif pattern == "one-at-round-border":
            assert want.sum() == 1 and c["stay"][sc.single_entry_index(c["stay"].size)]
            if not name.startswith("c/"):
                assert np.flatnonzero(c["stay"])[0] == ROUND * CHUNK and counts[ROUND] == 1
        elif pattern == "one-before-round-border":
            assert want.sum() == 1
            if not name.startswith("c/"):
                assert np.flatnonzero(c["stay"])[0] == ROUND * CHUNK - 1 and counts[ROUND - 1] == 1 and counts[ROUND] == 0
        elif pattern == "half" or name == sc.CONTINUATION:
            assert 0.49 < c["stay"].mean() < 0.51
    assert set(sc.CYCLE) <= seen, "a named per-chunk count does not occur"
    for what, (y, x) in sc.WINDOW_POINTS.items():
        for r in sc.WINDOW_RADII:
            want = sc.expected("window/%s/r%d" % (what, r))
            hy, hx = min(sc.H - 1, y + r) - max(0, y - r) + 1, min(sc.W - 1, x + r) - max(0, x - r) + 1
            assert want.sum() == hy * hx and want[y, x]
    for r in sc.WINDOW_RADII:
        assert not sc.expected("window/row-end/r%d" % r)[101, 0] and not sc.expected("window/row-start/r%d" % r)[100, sc.W - 1]
        c, want = sc.case("window/stopped-noisy/r%d" % r), sc.expected("window/stopped-noisy/r%d" % r)
        assert (c["n"] == 2).sum() == 4 and want.sum() == (2 * r + 1) ** 2 and not want[55:66, 55:66].any()
        c, want = sc.case("window/nan/r%d" % r), sc.expected("window/nan/r%d" % r)
        assert np.isnan(c["s1"]).sum() == 3 and want[np.isnan(c["s1"])].all() and want.sum() == (2 * r + 1) ** 2 + (r + 1) ** 2 + (2 * r + 1) * (r + 1)


def test_simulate_resumes_from_a_given_state():
    T = 8
    rng = np.random.default_rng(11)
    c = rng.uniform(0, 1, (T, 6, 7, 3)) * rng.uniform(0, 1, (1, 6, 7, 1)) ** 4
    kw = dict(threshold=0.25, floor=0.01, min_replicas=4, check_interval=2, radius=1)
    full = ar.simulate(c, **kw)
    assert 0 < (full["n"] < T).sum() < 42 and len(np.unique(full["n"])) >= 3
    y = [ar.luminance(c[t], T) for t in range(4)]
    start = dict(k=4, n=np.full((6, 7), 4, dtype=np.uint32), s1=((y[0] + y[1]) + y[2]) + y[3],
                 s2=((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]) + y[3] * y[3], sum=((c[0] + c[1]) + c[2]) + c[3], active=np.ones((6, 7), dtype=bool))
    again = ar.simulate(c, start=start, **kw)
    for key in full:
        assert np.array_equal(full[key], again[key], equal_nan=full[key].dtype.kind == "f"), key
    none = ar.simulate(c, start=dict(k=0, n=np.zeros((6, 7)), s1=np.zeros((6, 7)), s2=np.zeros((6, 7)), sum=np.zeros((6, 7, 3)),
                                     active=np.ones((6, 7), dtype=bool)), **kw)
    assert all(np.array_equal(full[key], none[key]) for key in full)
    # a stopped pixel of the start state stays where it is, whatever its moments say
    start["n"] = start["n"].copy()
    start["n"][2, 3] = 2
    start["active"] = start["n"] == 4
    part = ar.simulate(c, start=start, **kw)
    assert part["n"][2, 3] == 2 and np.array_equal(part["sum"][2, 3], start["sum"][2, 3]) and part["s1"][2, 3] == start["s1"][2, 3]


# ---- a numpy model of the decision step, with switchable faults ------------------------------------------------------

NOISY, QUIET, STOPPED = 0, 1, 2
SENTINEL = np.uint32(0xFFFFFFFF)
FAULTS = ("scan-base-reset-each-round", "chunk-offset-off-by-one", "tail-chunk-dropped", "tail-lanes-past-end-stay",
          "window-without-row-end-check", "stopped-read-as-noisy", "nan-read-as-quiet", "quiet-over-every-pixel")


def model_compact(src, keep, state, fault):
    """Per-chunk counts, k_ad_scan, k_ad_scatter: the kept entries of src in order; the others' pixels become STOPPED."""
    n_src = src.size
    n_blocks = n_src // CHUNK if fault == "tail-chunk-dropped" else (n_src + CHUNK - 1) // CHUNK
    if fault == "tail-lanes-past-end-stay" and n_src % 256:  # lanes of the last 256-step beyond `end`: pixel 0, staying
        pad = 256 - n_src % 256
        src = np.concatenate([src, np.zeros(pad, dtype=src.dtype)])
        keep = np.concatenate([keep, np.ones(pad, dtype=bool)])
    seen = min(src.size, n_blocks * CHUNK)
    src, keep = src[:seen], keep[:seen]
    if seen == 0:
        return src[:0]
    starts = np.arange(0, seen, CHUNK)
    counts = np.add.reduceat(keep.astype(np.int64), starts)
    offset = np.zeros(n_blocks, dtype=np.int64)
    base = 0
    for b0 in range(0, n_blocks, ROUND):  # one wave, 64 counts a round, `base` carried
        v = counts[b0:b0 + ROUND]
        incl = np.cumsum(v)
        if fault == "scan-base-reset-each-round":
            base = 0
        offset[b0:b0 + ROUND] = base + incl - v
        base += int(incl[-1])
    n_out = base
    excl = np.cumsum(keep) - keep
    chunk = np.arange(seen) // CHUNK
    pos = offset[chunk] + (excl - excl[starts][chunk])
    if fault == "chunk-offset-off-by-one":
        pos = pos + (chunk > 0)
    out = np.full(seen + CHUNK, SENTINEL, dtype=np.uint32)
    out[pos[keep]] = src[keep]
    gone = src[~keep]
    state[gone[gone != SENTINEL]] = STOPPED  # SENTINEL: a list slot a faulty scatter never wrote
    return out[:n_out]


def model(c, fault=None):
    """The list after rt_accum_load_state of the case's state: adaptive_rebuild, then adaptive_decide at a decision point."""
    k, radius, h, w = c["k"], c["radius"], sc.H, sc.W
    n, s1, s2 = c["n"].reshape(-1), c["s1"].reshape(-1), c["s2"].reshape(-1)
    state = np.full(n.size, NOISY, dtype=np.uint8)
    lst = model_compact(np.arange(n.size, dtype=np.uint32), n == k, state, fault)  # k_ad_flags_from_counts feeds it
    if k not in sc.D or lst.size == 0:
        return lst
    who = np.arange(n.size) if fault == "quiet-over-every-pixel" else lst[lst != SENTINEL]
    with np.errstate(all="ignore"):
        mean = s1[who] / float(k)
        num = s2[who] - s1[who] * mean
        num = np.where(num < 0.0, 0.0, num)
        se2 = num / (float(k) * float(k - 1))
        lim = sc.THRESHOLD * (mean + sc.PARAMS["floor"])
        q = ~(se2 > lim * lim) if fault == "nan-read-as-quiet" else se2 <= lim * lim
    state[who] = np.where(q, QUIET, NOISY)
    p = lst.astype(np.int64)
    p[lst == SENTINEL] = 0
    y, x = p // w, p % w
    stop = state[p] == QUIET
    holds = state != QUIET if fault == "stopped-read-as-noisy" else state == NOISY
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ok = (y + dy >= 0) & (y + dy < h)
            if fault != "window-without-row-end-check":
                ok &= (x + dx >= 0) & (x + dx < w)
            flat = (y + dy) * w + (x + dx)
            ok &= (flat >= 0) & (flat < n.size)
            stop &= ~(ok & holds[np.clip(flat, 0, n.size - 1)])
    return model_compact(lst, ~stop, state, fault)


def test_the_catalogue_tells_a_wrong_decision_step_from_a_right_one():
    caught = {f: [] for f in FAULTS}
    for name in sc.NAMES:
        c = sc.case(name)
        want = np.flatnonzero(sc.expected(name)).astype(np.uint32)
        assert np.array_equal(model(c), want), name + ": the fault-free model and the rule disagree"
        for f in FAULTS:
            if not np.array_equal(model(c, f), want):
                caught[f].append(name)
    for f in FAULTS:
        print("%-30s caught by %2d cases: %s" % (f, len(caught[f]), ", ".join(caught[f][:6]) + (" ..." if len(caught[f]) > 6 else "")))
    for f in FAULTS:
        assert caught[f], f + ": no case of the catalogue notices this fault"
    # the cases built for a fault do catch it
    # (an entry at the border itself has nothing before it in its round: the one before it is what a lost `base` moves)
    assert {"a/one-before-round-border", "b/one-before-round-border", "b/last-of-chunk", "a/cycle"} <= set(caught["scan-base-reset-each-round"])
    assert {"a/one-at-round-border", "b/one-at-round-border"} <= set(caught["chunk-offset-off-by-one"])
    assert "b/first-of-chunk" in caught["chunk-offset-off-by-one"] and "c/cycle" in caught["chunk-offset-off-by-one"]
    assert {"a/last-of-chunk", "b/last-of-chunk", "c/last-of-chunk"} <= set(caught["tail-chunk-dropped"])
    assert {"b/none", "b/all", "a/all", "b/last-of-chunk"} <= set(caught["tail-lanes-past-end-stay"])
    assert {"window/row-end/r1", "window/row-start/r4"} <= set(caught["window-without-row-end-check"])
    assert {"window/stopped-noisy/r1", "window/stopped-noisy/r4"} <= set(caught["stopped-read-as-noisy"]) & set(caught["quiet-over-every-pixel"])
    assert {"window/nan/r1", "a/half"} <= set(caught["nan-read-as-quiet"])
