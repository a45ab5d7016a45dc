"""The hand-out policy of the persistent search kernels (csrc/rt_handout.h), replayed on the host without a GPU:
rt_debug_handout_replay runs the very functions the kernels call (handout_first / handout_static / handout_next), with a plain
counter in place of the atomic, for a queue of n entries, W waves and an order in which the waves ask.

For every case: the ranges partition [0, n) exactly; every size is a multiple of 64 in 64..256 except the range that ends
at n; the kernel makes at most n/256 + 4 W atomics; a wave that has been told "exhausted" is handed nothing when it asks again."""
import numpy as np
import pytest

from rust_raytracer_amd import api

WAVES = (1, 4, 8, 12, 1024, 4096)
ORDERS = ("forward", "reverse", "random")
EXHAUSTED = 0xFFFFFFFF


def asking_order(kind: str, waves: int) -> np.ndarray:
    if kind == "forward":
        return np.arange(waves, dtype=np.uint32)
    if kind == "reverse":
        return np.arange(waves, dtype=np.uint32)[::-1].copy()
    # seeded: some waves ask far more often than others, every wave at least once
    rng = np.random.default_rng(1234 + waves)
    often = rng.integers(0, waves, size=3 * waves, dtype=np.uint32)
    return rng.permutation(np.concatenate([often, np.arange(waves, dtype=np.uint32)]))


_orders = {(k, w): asking_order(k, w) for k in ORDERS for w in WAVES}
_buf = np.empty((1 << 16, 3), dtype=np.uint32)


def check(n: int, waves: int, kind: str, policy=None):
    asks, atomics, atomics_after = api.handout_replay(n, waves, _orders[(kind, waves)], policy, _buf)
    where = f"n = {n}, W = {waves}, {kind} order"
    done = asks[:, 1] == EXHAUSTED
    assert np.array_equal(done, asks[:, 2] == EXHAUSTED), where
    got = asks[~done]
    # partition of [0, n): sorted by first entry, every range starts where the one before ends
    got = got[np.argsort(got[:, 1], kind="stable")]
    first, end = got[:, 1].astype(np.int64), got[:, 2].astype(np.int64)
    assert np.all(end > first), where
    if n == 0:
        assert got.shape[0] == 0, where
    else:
        assert first[0] == 0 and end[-1] == n and np.array_equal(first[1:], end[:-1]), where
    size = end - first
    inner = size[end != n]
    assert np.all((inner % 64 == 0) & (inner >= 64) & (inner <= 256)), where
    assert np.all(size <= 256), where
    assert atomics <= n // 256 + 4 * waves, f"{where}: {atomics} atomics"
    # per wave: nothing after "exhausted" (the replay asks every wave once more after it), and exactly two such answers
    last_range = np.full(waves, -1, dtype=np.int64)
    first_done = np.full(waves, asks.shape[0], dtype=np.int64)
    idx = np.arange(asks.shape[0])
    np.maximum.at(last_range, asks[~done, 0], idx[~done])
    np.minimum.at(first_done, asks[done, 0], idx[done])
    assert np.all(last_range < first_done), where
    assert np.array_equal(np.bincount(asks[done, 0], minlength=waves), np.full(waves, 2)), where
    return got, atomics


@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("waves", WAVES)
def test_small_queues(waves, kind):
    for n in range(0, 2001):
        check(n, waves, kind)


@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("n", (65535, 65536, 65537, 1048577))
def test_large_queues(n, waves, kind):
    check(n, waves, kind)


def test_static_ranges_need_no_atomic():
    """W * s0 >= n: nobody touches the cursor; s0 is ceil(n / W) rounded up to a multiple of 64 inside 64..256."""
    for n, waves, s0 in ((1, 4, 64), (256, 4, 64), (257, 4, 128), (1000, 4, 256), (1024, 4, 256), (4096 * 256, 4096, 256), (5000, 4096, 64)):
        got, atomics = check(n, waves, "forward")
        assert atomics == 0
        assert np.all(got[:-1, 2] - got[:-1, 1] == s0) and got[-1, 2] - got[-1, 1] <= s0


def test_ranges_shrink_towards_the_end():
    """256 while much is left, then 128, then 64: sizes never grow along the queue behind the static ranges (forward order: the
    waves' knowledge of the cursor is equally fresh), and all three sizes occur."""
    n, waves = 1048577, 1024
    got, _ = check(n, waves, "forward")
    size = (got[:, 2] - got[:, 1])[:-1].astype(np.int64)
    dyn = size[waves:]
    assert np.all(size[:waves] == 256)
    assert np.all(np.diff(dyn) <= 0) and set(np.unique(dyn)) == {64, 128, 256}


def test_mode_0_is_the_fixed_hand_out():
    """RT_WF_HANDOUT=0, the A/B control: no static range, 256 entries per atomic, one failing atomic per wave."""
    for n, waves in ((0, 4), (1000, 4), (65537, 12)):
        asks, atomics, _ = api.handout_replay(n, waves, _orders[("forward", waves)], (0, 0, 0), _buf)
        got = asks[asks[:, 1] != EXHAUSTED]
        assert np.array_equal(np.sort(got[:, 1]), np.arange(0, n, 256))
        assert np.array_equal(np.minimum(got[:, 1] + 256, n), got[:, 2])
        assert atomics == (n + 255) // 256 + waves
