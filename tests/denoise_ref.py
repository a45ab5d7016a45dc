"""numpy restatement of the edge-avoiding a-trous denoiser of rt_denoise (include/rt_mi355.h, csrc/rt_aov.hip), operation for
operation: tap weights in float32, the weighted colour and weight sums in float64, taps in the kernel's order (dy, then
dx, from -2 to 2).  Only exp may differ from the device's in its last bits."""
import numpy as np

F32 = np.float32
KH = (np.array([1, 4, 6, 4, 1], dtype=F32) / F32(16)).astype(F32)
DEFAULTS = dict(iterations=4, sigma_color=8.0, sigma_normal=0.3, sigma_albedo=0.3, sigma_depth=0.1, demodulate=True)  # rt_denoise_default_params


def params_of(dp):
    """The keyword arguments of denoise() for an api.RtDenoiseParams."""
    return dict(iterations=dp.iterations, sigma_color=dp.sigma_color, sigma_normal=dp.sigma_normal,
                sigma_albedo=dp.sigma_albedo, sigma_depth=dp.sigma_depth, demodulate=bool(dp.flags & 1))


def _shifted(a, oy, ox, fill):
    """b[y, x] = a[y + oy, x + ox], `fill` where that lies outside the image."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def denoise(rgba, aov, iterations=4, sigma_color=8.0, sigma_normal=0.3, sigma_albedo=0.3, sigma_depth=0.1, demodulate=True):
    rgba = np.asarray(rgba, dtype=np.float64)
    aov = np.asarray(aov, dtype=np.float64)
    if iterations == 0:
        return rgba.copy()
    albedo = aov[..., 0:3].astype(F32)
    normal = aov[..., 3:6].astype(F32)
    depth = aov[..., 6].astype(F32)
    amask = albedo > F32(1e-3)
    a64 = albedo.astype(np.float64)
    col = rgba[..., :3].copy()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        if demodulate:
            col = np.where(amask, col / a64, col)
        sc, sn, sa, sz = F32(sigma_color), F32(sigma_normal), F32(sigma_albedo), F32(sigma_depth)
        den_n, den_a = sn * sn, sa * sa
        for i in range(iterations):
            step = 1 << i
            den_c = sc * sc * F32(2.0 ** -i)
            centre_finite = np.isfinite(col).all(-1)
            fp = col.astype(F32)
            s = np.zeros_like(col)
            ws = np.zeros(col.shape[:2])
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cq = _shifted(col, dy * step, dx * step, np.nan)  # outside = not finite: skipped either way
                    aq = _shifted(albedo, dy * step, dx * step, F32(0))
                    nq = _shifted(normal, dy * step, dx * step, F32(0))
                    zq = _shifted(depth, dy * step, dx * step, F32(0))
                    d = cq.astype(F32) - fp
                    wc = np.where(centre_finite, np.exp(-(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) / den_c),
                                  F32(1))
                    e = nq - normal
                    wn = np.exp(-(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]) / den_n)
                    e = aq - albedo
                    wa = np.exp(-(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]) / den_a)
                    wz = np.exp(-np.abs(zq - depth) / (sz * np.fmax(depth, zq) + F32(1e-30)))
                    wt = KH[dy + 2] * KH[dx + 2] * wc.astype(F32) * wn * wa * wz
                    use = np.isfinite(cq).all(-1) & (wt > F32(0))
                    wd = np.where(use, wt.astype(np.float64), 0.0)
                    s += wd[..., None] * np.where(use[..., None], cq, 0.0)
                    ws += wd
            out = np.where((ws > 0)[..., None], s / np.where(ws > 0, ws, 1.0)[..., None], col)
            if demodulate and i == iterations - 1:
                out = np.where(amask, out * a64, out)
            col = out
    return np.concatenate([col, rgba[..., 3:4]], axis=-1)
