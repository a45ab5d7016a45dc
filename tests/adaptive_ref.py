"""numpy restatement of the adaptive-sampling rule of rt_accum_set_adaptive (include/rt_mi355.h),
operation for operation: luminance moments of the per-replica contributions in replica order, the decision points, the
quiet test, the window rule, the estimate and the noise image.  numpy never fuses a*b+c, like the uncontracted kernels.

`contrib[t, y, x, :3]` is what replica t adds to pixel (y, x) of the sum; snapshots of a plain accumulator give it as
differences of consecutive sums (contributions_from_snapshots), exact up to the rounding of that subtraction."""
import numpy as np

DEFAULTS = dict(floor=0.01, min_replicas=4, check_interval=2, radius=1)  # rt_adaptive_default_params; threshold has none
BAND = 1e-9  # relative distance of se2 from lim^2 inside which a decision may legitimately fall either way


def params_of(ap):
    """The keyword arguments of simulate() for an api.RtAdaptiveParams."""
    return dict(threshold=ap.threshold, floor=ap.floor, min_replicas=ap.min_replicas, check_interval=ap.check_interval,
                radius=ap.radius)


def decision_points(T, min_replicas, check_interval):
    """D = { k : min_replicas <= k < T, (k - min_replicas) mod check_interval = 0 }, ascending."""
    return [k for k in range(min_replicas, T) if (k - min_replicas) % check_interval == 0]


def luminance(c, T):
    """y = double(T) * ((0.2126 c_r + 0.7152 c_g) + 0.0722 c_b)"""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.float64(T) * ((0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2])


def se2_and_limit(s1, s2, k, threshold, floor):
    """(se2, lim^2, mean) of pixels with k >= 2 replicas (k: scalar or array)."""
    k = np.asarray(k, dtype=np.float64)
    with np.errstate(all="ignore"):
        mean = s1 / k
        num = s2 - s1 * mean
        num = np.where(num < 0.0, 0.0, num)  # a NaN stays a NaN
        se2 = num / (k * (k - 1.0))
        lim = threshold * (mean + floor)
        return se2, lim * lim, mean


def quiet(s1, s2, k, threshold, floor):
    """se2 <= lim^2; false where anything is NaN."""
    se2, lim2, _ = se2_and_limit(s1, s2, k, threshold, floor)
    with np.errstate(all="ignore"):
        return se2 <= lim2


def _any_in_window(mask, radius):
    """out[y, x] = any(mask[y + dy, x + dx]) over |dy|, |dx| <= radius inside the image."""
    h, w = mask.shape
    out = np.zeros_like(mask)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            y0, y1 = max(0, -dy), min(h, h - dy)
            x0, x1 = max(0, -dx), min(w, w - dx)
            if y0 < y1 and x0 < x1:
                out[y0:y1, x0:x1] |= mask[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def stops(quiet_mask, active, radius):
    """A pixel stops iff it is active and quiet and every ACTIVE pixel of its window is quiet too: stopped pixels do
    not hold their neighbours."""
    noisy = active & ~quiet_mask
    return active & quiet_mask & ~_any_in_window(noisy, radius)


def contributions_from_snapshots(snapshots):
    """snapshots[k] = sum_k of a plain accumulator (k = 0 .. T, snapshots[0] = 0): contrib[t] = sum_{t+1} - sum_t."""
    s = np.asarray(snapshots, dtype=np.float64)
    with np.errstate(all="ignore"):
        return s[1:] - s[:-1]


def simulate(contrib, threshold, floor=0.01, min_replicas=4, check_interval=2, radius=1, start=None):
    """Runs the rule over contrib (T, H, W, >= 3).  Returns a dict: n (uint32), s1, s2, sum (H, W, 3), active (bool: still
    active at the end), band (bool: se2 within BAND of lim^2 at one of the pixel's decision points), exempt (band dilated
    by the window: pixels whose decision may depend on one in the band).

    `start` = dict(k, n, s1, s2, sum, active) resumes at replica k from that state, as a loaded accumulator does
    (rt_accum_load_state): `active` is the set before any decision at k, and if k is a decision point the decision at k is
    taken on the given moments first; contrib[:k] is not read."""
    contrib = np.asarray(contrib, dtype=np.float64)
    T, h, w = contrib.shape[:3]
    D = set(decision_points(T, min_replicas, check_interval))
    n = np.zeros((h, w), dtype=np.uint32)
    s1 = np.zeros((h, w))
    s2 = np.zeros((h, w))
    total = np.zeros((h, w, 3))
    active = np.ones((h, w), dtype=bool)
    band = np.zeros((h, w), dtype=bool)
    first = 0
    if start is not None:
        first = int(start["k"])
        n = np.array(start["n"], dtype=np.uint32).reshape(h, w)
        s1 = np.array(start["s1"], dtype=np.float64).reshape(h, w)
        s2 = np.array(start["s2"], dtype=np.float64).reshape(h, w)
        total = np.array(start["sum"], dtype=np.float64).reshape(h, w, -1)[..., :3]
        active = np.array(start["active"], dtype=bool).reshape(h, w)
        if first in D:
            with np.errstate(all="ignore"):
                se2, lim2, _ = se2_and_limit(s1, s2, first, threshold, floor)
                band |= active & (np.abs(se2 - lim2) <= BAND * lim2)
                active = active & ~stops(se2 <= lim2, active, radius)
    with np.errstate(all="ignore"):
        for t in range(first, T):
            if not active.any():
                break
            c = contrib[t, ..., :3]
            y = luminance(c, T)
            s1 = np.where(active, s1 + y, s1)
            s2 = np.where(active, s2 + y * y, s2)
            total = np.where(active[..., None], total + c, total)
            n = n + active.astype(np.uint32)
            k = t + 1
            if k in D:
                se2, lim2, _ = se2_and_limit(s1, s2, k, threshold, floor)
                band |= active & (np.abs(se2 - lim2) <= BAND * lim2)
                active = active & ~stops(se2 <= lim2, active, radius)
    return dict(n=n, s1=s1, s2=s2, sum=total, active=active, band=band, exempt=_any_in_window(band, radius))


def estimate(total, n, T):
    """sum[p] * (double(T) / double(n[p]))"""
    with np.errstate(all="ignore"):
        return np.asarray(total, dtype=np.float64) * (np.float64(T) / n.astype(np.float64))[..., None]


def noise(s1, s2, n, floor):
    """sqrt(se2) / (mean + floor) at each pixel's n; 0 while n < 2."""
    k = np.maximum(n, 2).astype(np.float64)
    se2, _, mean = se2_and_limit(s1, s2, k, 1.0, floor)
    with np.errstate(all="ignore"):
        return np.where(n < 2, 0.0, np.sqrt(se2) / (mean + floor))


def quality(est, full, n, T, threshold):
    """The figures of the quality check: share of pixels stopped, share of the samples rendered, share of the stopped
    pixels with dev = |Y_est - Y_full| / (Y_full + 0.01) > threshold and > 3 threshold."""
    stopped = n < T
    y_a, y_f = luminance(est, 1), luminance(full, 1)
    with np.errstate(all="ignore"):
        dev = np.abs(y_a - y_f) / (y_f + 0.01)
    d = dev[stopped]
    return dict(stopped=float(stopped.mean()), rendered=float(n.astype(np.float64).sum() / (T * n.size)),
                over=float((d > threshold).mean()) if d.size else 0.0, over3=float((d > 3 * threshold).mean()) if d.size else 0.0)
