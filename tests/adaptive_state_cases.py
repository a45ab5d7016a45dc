"""Crafted states of an adaptive accumulator and what the rule says about them.

rt_accum_load_state copies sum, s1, s2 and n from a version-2 blob and checks only the header, the parameter block and
that every count is replicas_done or an earlier decision point (accum_check_state, rt_accum_state.h); adaptive_rebuild
then rebuilds the active list from the counts and, at a decision point, decides on the loaded moments.  So a blob with
made-up moments hands the decision step (k_ad_quiet, k_ad_window, k_ad_scan, k_ad_scatter, k_ad_flags_from_counts in
rt_accum.hip) any keep pattern, at a size where the list spans more workgroups than one scan round holds, and
expected_active() says, from tests/adaptive_ref.py alone, which pixels have to be on the list afterwards.

Frame: 515 x 257 = 132 355 pixels, one sample per replica, 8 replicas: 65 chunks of AD_CHUNK entries (one more than a
scan round of 64), the last of 1 283 = 5 * 256 + 3 entries.  Index i runs over A0 = (n == k) in ascending pixel order;
chunk = i // AD_CHUNK.

Cases are named "<route>/<pattern>" and "window/<what>/r<radius>":
  a/  k = 4, every pixel active, the pattern in quiet and noisy moments: rebuild, then decide
  b/  k = 3 (no decision point), staying entries n = 3, the rest n = 2: flags from counts, scan and scatter alone
  c/  k = 4, A0 a seeded 37 % of the pixels (the others n = 2, with noisy moments nobody may read), the pattern over the
      entries of that list: decide reads a sparse source list.  That list has 24 chunks, so the two single-entry patterns,
      which sit at the first scan-round border (i = 64 * AD_CHUNK) where the list is long enough, sit at the start of its
      last chunk and the entry before it."""
import functools
import struct

import numpy as np

import adaptive_ref as ar

AD_CHUNK = 2048      # constexpr uint32_t AD_CHUNK in rust_raytracer_amd/csrc/rt_accum.hip (test_adaptive_state_cases_host.py checks)
SCAN_ROUND = 64      # workgroup counts per round of k_ad_scan: one wave
SEED = 81
ARGS = ["scenes/cornell", "-w=515", "-r=2", "-s=8", "-t=8", "--seed=%d" % SEED]
W, H, T = 515, 257, 8
NPIX = W * H
PARAMS = dict(min_replicas=2, check_interval=2, floor=0.01)
THRESHOLD = 0.3
D = ar.decision_points(T, PARAMS["min_replicas"], PARAMS["check_interval"])
assert D == [2, 4, 6]
HEADER, PARAM_BYTES = 48, 32
CYCLE = (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048)  # per-chunk stay counts of the "cycle" pattern
PATTERNS = ("all", "none", "first-of-chunk", "last-of-chunk", "one-at-round-border", "one-before-round-border", "cycle", "half")
ROUTES = ("a", "b", "c")
WINDOW_POINTS = {"corner-tl": (0, 0), "corner-tr": (0, W - 1), "corner-bl": (H - 1, 0), "corner-br": (H - 1, W - 1),
                 "row-end": (100, W - 1), "row-start": (101, 0), "interior": (137, 260)}
WINDOW_RADII = (1, 4)


def check_frame(hs):
    """The figures this catalogue is built on, from the parsed scene (api.HostScene(ARGS))."""
    assert (hs.width, hs.height) == (W, H) and hs.params.thread_count == T and hs.params.sqrt_spt == 1
    assert NPIX == 132355 and NPIX > SCAN_ROUND * AD_CHUNK
    assert (NPIX + AD_CHUNK - 1) // AD_CHUNK == SCAN_ROUND + 1
    assert NPIX - SCAN_ROUND * AD_CHUNK == 1283 == 5 * 256 + 3


def parse(blob, h=H, w=W):
    """The version-2 layout, as parse_v2 of tests/test_gpu_adaptive.py reads it (arrays are views of the blob)."""
    np_ = h * w
    assert blob[:8] == b"RTACCUM\0" and struct.unpack_from("<I", blob, 8)[0] == 2
    assert len(blob) == HEADER + PARAM_BYTES + np_ * (32 + 8 + 8 + 4)
    off = HEADER + PARAM_BYTES
    return dict(k=struct.unpack_from("<I", blob, 28)[0],
                sum=np.frombuffer(blob, dtype=np.float64, count=np_ * 4, offset=off).reshape(h, w, 4),
                s1=np.frombuffer(blob, dtype=np.float64, count=np_, offset=off + np_ * 32).reshape(h, w),
                s2=np.frombuffer(blob, dtype=np.float64, count=np_, offset=off + np_ * 40).reshape(h, w),
                n=np.frombuffer(blob, dtype=np.uint32, count=np_, offset=off + np_ * 48).reshape(h, w))


def craft(template, k, sum_k, s1, s2, n):
    """`template` (the blob of a real adaptive accumulator of this frame: its header and parameter block) with
    replicas_done = k and the four arrays replaced."""
    np_ = n.size
    assert len(template) == HEADER + PARAM_BYTES + np_ * 52 and sum_k.size == np_ * 4 and s1.size == np_ and s2.size == np_
    out = bytearray(template[:HEADER + PARAM_BYTES])
    struct.pack_into("<I", out, 28, int(k))
    out += np.ascontiguousarray(sum_k, dtype=np.float64).tobytes()
    out += np.ascontiguousarray(s1, dtype=np.float64).tobytes()
    out += np.ascontiguousarray(s2, dtype=np.float64).tobytes()
    out += np.ascontiguousarray(n, dtype=np.uint32).tobytes()
    return bytes(out)


def counts_are_loadable(k, n):
    """The count rule of accum_check_state: every count is k, or a decision point before k."""
    n = np.asarray(n)
    return bool(((n == k) | ((n < k) & np.isin(n, D))).all())


def expected_active(k, s1, s2, n, radius):
    """The active set after rt_accum_load_state: n == k, less (at a decision point) what the rule stops."""
    a0 = n == k
    if k in D:
        return a0 & ~ar.stops(ar.quiet(s1, s2, k, THRESHOLD, PARAMS["floor"]), a0, radius)
    return a0


def band(k, s1, s2, n):
    """Pixels whose decision at k may fall either way: |se2 - lim^2| <= 1e-9 lim^2 (empty for every crafted case)."""
    if k not in D:
        return np.zeros(n.shape, dtype=bool)
    se2, lim2, _ = ar.se2_and_limit(s1, s2, k, THRESHOLD, PARAMS["floor"])
    with np.errstate(all="ignore"):
        return (n == k) & (np.abs(se2 - lim2) <= ar.BAND * lim2)


# ---- moments -----------------------------------------------------------------------------------------------------

def quiet_moments(k):        # se2 = 0
    return float(k), float(k)


def clamped_moments(k):      # num = s2 - s1 * mean < 0: clamped to se2 = 0
    return float(k), float(k) * (1.0 - 2.0 ** -40)


def noisy_moments(k):        # se2 = 99 k / (k (k - 1)) against lim^2 = 0.0918
    return float(k), 100.0 * float(k)


def nan_moments(k):          # noisy for ever
    return float("nan"), 100.0 * float(k)


def mild_moments(k):         # se2 = 0.1, 9 % above lim^2: noisy at k, but bright replicas can make it quiet later (continuation only)
    return float(k), float(k) + 0.1 * float(k) * float(k - 1)


def _fill(s1, s2, where, moments):
    s1[where], s2[where] = moments


def moments_of_pattern(k, a0, stay, noisy=noisy_moments):
    """s1, s2 over the frame: staying entries noisy (every 7th of them NaN), leaving ones quiet (every 3rd through the
    clamp), pixels outside A0 noisy: they are stopped and must not be read."""
    s1 = np.empty(a0.size)
    s2 = np.empty(a0.size)
    _fill(s1, s2, slice(None), noisy_moments(k))
    idx = np.flatnonzero(a0)
    st, go = idx[stay], idx[~stay]
    _fill(s1, s2, st, noisy(k))
    if noisy is noisy_moments:
        _fill(s1, s2, st[3::7], nan_moments(k))
    _fill(s1, s2, go, quiet_moments(k))
    _fill(s1, s2, go[1::3], clamped_moments(k))
    return s1, s2


# ---- keep patterns over a list of m entries ------------------------------------------------------------------------

def single_entry_index(m):
    """Where the single-entry patterns put their entry: the first scan-round border, or the last chunk's start."""
    return min(SCAN_ROUND * AD_CHUNK, (m - 1) // AD_CHUNK * AD_CHUNK)


def keep_pattern(pattern, m, rng):
    i = np.arange(m)
    if pattern == "all":
        return np.ones(m, dtype=bool)
    if pattern == "none":
        return np.zeros(m, dtype=bool)
    if pattern == "first-of-chunk":
        return i % AD_CHUNK == 0
    if pattern == "last-of-chunk":
        return (i % AD_CHUNK == AD_CHUNK - 1) | (i == m - 1)
    if pattern == "one-at-round-border":
        return i == single_entry_index(m)
    if pattern == "one-before-round-border":
        return i == single_entry_index(m) - 1
    if pattern == "cycle":
        stay = np.zeros(m, dtype=bool)
        for c, b in enumerate(range(0, m, AD_CHUNK)):
            size = min(AD_CHUNK, m - b)
            stay[b + rng.permutation(size)[:min(CYCLE[c % len(CYCLE)], size)]] = True
        return stay
    if pattern == "half":
        return rng.random(m) < 0.5
    raise KeyError(pattern)


def chunk_counts(stay):
    """Entries that stay per chunk of AD_CHUNK list entries."""
    return np.add.reduceat(stay.astype(np.int64), np.arange(0, stay.size, AD_CHUNK))


# ---- the catalogue ---------------------------------------------------------------------------------------------------

def _rng(name):
    return np.random.default_rng([SEED] + list(name.encode()))


def _pattern_case(name, route, pattern, noisy=noisy_moments):
    rng = _rng(name)
    if route == "c":
        a0 = rng.random(NPIX) < 0.37
        assert abs(a0.mean() - 0.37) < 0.01
    else:
        a0 = np.ones(NPIX, dtype=bool)
    stay = keep_pattern(pattern, int(a0.sum()), rng)
    if route == "b":
        k = 3
        listed = stay  # what k_ad_scatter compacts here: the identity list of every pixel
        n = np.full(NPIX, 2, dtype=np.uint32)
        n[np.flatnonzero(a0)[stay]] = 3
        s1, s2 = (np.full(NPIX, v) for v in quiet_moments(k))  # not read: 3 is no decision point
        a0 = n == 3
        stay = np.ones(int(a0.sum()), dtype=bool)
    else:
        k = 4
        n = np.where(a0, 4, 2).astype(np.uint32)
        s1, s2 = moments_of_pattern(k, a0, stay, noisy)
        listed = stay
    want = np.zeros(NPIX, dtype=bool)
    want[np.flatnonzero(a0)[stay]] = True
    return dict(name=name, k=k, radius=0, s1=s1.reshape(H, W), s2=s2.reshape(H, W), n=n.reshape(H, W),
                stay=listed, want=want.reshape(H, W))


def _window_case(name, what, radius):
    k = 4
    n = np.full((H, W), k, dtype=np.uint32)
    s1 = np.full((H, W), quiet_moments(k)[0])
    s2 = np.full((H, W), quiet_moments(k)[1])
    s2[::2, 1::3] = clamped_moments(k)[1]
    want = np.zeros((H, W), dtype=bool)

    def hold(y, x):
        want[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1] = True

    if what in WINDOW_POINTS:
        y, x = WINDOW_POINTS[what]
        s1[y, x], s2[y, x] = noisy_moments(k)
        hold(y, x)
        if what == "row-end":
            assert not want[101, 0] and not want[100, 0]   # (101, 0) is the next flat index, not a neighbour
        if what == "row-start":
            assert not want[100, W - 1] and not want[101, W - 1]
    elif what == "stopped-noisy":
        # noisy moments at n = 2 (stopped at the decision before): they hold nobody; one active noisy pixel far away
        for y, x in ((60, 60), (100, W - 1), (0, 0), (H - 1, 300)):
            s1[y, x], s2[y, x] = noisy_moments(k)
            n[y, x] = 2
        s1[200, 400], s2[200, 400] = noisy_moments(k)
        hold(200, 400)
    elif what == "nan":
        for y, x in ((150, 33), (H - 1, W - 1), (77, 0)):
            s1[y, x], s2[y, x] = nan_moments(k)
            hold(y, x)
            assert want[y, x]
    else:
        raise KeyError(what)
    return dict(name=name, k=k, radius=radius, s1=s1, s2=s2, n=n, stay=want[n == k], want=want)


CONTINUATION = "c/half-mild"  # route c, the staying half mildly noisy: later decisions stop some of it
NAMES = (["%s/%s" % (r, p) for r in ROUTES for p in PATTERNS]
         + ["window/%s/r%d" % (w, r) for w in list(WINDOW_POINTS) + ["stopped-noisy", "nan"] for r in WINDOW_RADII]
         + [CONTINUATION])


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, k, radius, s1, s2, n (H x W), stay (the keep flags the scatter step sees, over its source list), want
    (the set the case was built to leave active: expected_active() has to agree))."""
    parts = name.split("/")
    if parts[0] == "window":
        c = _window_case(name, parts[1], int(parts[2][1:]))
    elif name == CONTINUATION:
        c = _pattern_case(name, "c", "half", mild_moments)
    else:
        c = _pattern_case(name, parts[0], parts[1])
    for key in ("s1", "s2", "n", "stay", "want"):
        c[key].setflags(write=False)
    return c


def expected(name):
    c = case(name)
    return expected_active(c["k"], c["s1"], c["s2"], c["n"], c["radius"])
