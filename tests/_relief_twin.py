"""NumPy-only restatement of the reference's shaded-relief rendering (get_relief_map with biome, flow and rgb None) and the seeded
land-and-sea canvases the relief tests render.  Written from the operator definitions, not from the product's code: its own reflect-mode
Gaussian blur (fp64 accumulation, fp32 stored between the axes, as scipy.ndimage does), np.gradient, and a terrain lookup table built with
np.interp.  It gives expected values at sizes tests/golden/relief.npz cannot hold."""
import numpy as np

_TERRAIN = ((0.00, (0.2, 0.2, 0.6)), (0.15, (0.0, 0.6, 1.0)), (0.25, (0.0, 0.8, 0.4)),
            (0.50, (1.0, 1.0, 0.6)), (0.75, (0.5, 0.36, 0.33)), (1.00, (1.0, 1.0, 1.0)))


def land_and_sea(H, W, seed, sea=0.35):
    """Seeded (H, W) float32 elevation in metres: a few random plane waves per octave plus fine noise; about `sea` of it below 0."""
    rng = np.random.default_rng(seed)
    y = np.arange(H, dtype=np.float64)[:, None]
    x = np.arange(W, dtype=np.float64)[None, :]
    e = np.zeros((H, W), dtype=np.float64)
    for octave, amp in ((1, 1.0), (2, 0.5), (4, 0.25), (8, 0.12), (16, 0.06)):
        for _ in range(3):
            ang = rng.uniform(0, 2 * np.pi)
            f = octave * rng.uniform(0.6, 1.4) * 2 * np.pi / 256.0
            e += amp * np.sin(f * (np.cos(ang) * x + np.sin(ang) * y) + rng.uniform(0, 2 * np.pi))
    e += 0.01 * rng.standard_normal((H, W))
    e = (e - np.quantile(e, sea)) * 1800.0
    e = np.where(e < 0, e * 2.5, e)   # deeper sea than land is high
    return e.astype(np.float32)


def terrain_lut(n=256):
    pos = np.array([p for p, _ in _TERRAIN])
    t = np.linspace(0.0, 1.0, n)
    return np.stack([np.interp(t, pos, [c[k] for _, c in _TERRAIN]) for k in range(3)], axis=1).astype(np.float32)


def gaussian_weights(sigma):
    """fp64 weights and radius of scipy's gaussian_filter (truncate 4)."""
    if sigma <= 1e-15:
        return np.ones(1), 0
    r = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 * x * x / (float(sigma) * float(sigma)))
    return w / w.sum(), r


def reflect_index(i, n):
    """mode='reflect' (d c b a | a b c d | d c b a), any number of folds."""
    p = 2 * n
    i = np.mod(i, p)
    return np.where(i < n, i, p - 1 - i)


def blur_axis(a32, sigma, axis):
    w, r = gaussian_weights(sigma)
    n = a32.shape[axis]
    src = np.take(a32, reflect_index(np.arange(-r, n + r), n), axis=axis).astype(np.float64)
    acc = np.zeros(a32.shape, dtype=np.float64)
    for k in range(2 * r + 1):
        acc += w[k] * (src[k:k + n] if axis == 0 else src[:, k:k + n])
    return acc.astype(np.float32)


def gaussian_blur(a32, sigma):
    return blur_axis(blur_axis(a32, sigma, 0), sigma, 1)


def gradient(f):
    """np.gradient of a 2-D fp32 field, unit spacing, edge_order 1 -> (d/dy, d/dx) in fp32."""
    out = []
    for axis in (0, 1):
        g = np.empty_like(f)
        a = np.moveaxis(f, axis, 0)
        ga = np.moveaxis(g, axis, 0)
        ga[1:-1] = (a[2:] - a[:-2]) / np.float32(2.0)
        ga[0] = a[1] - a[0]
        ga[-1] = a[-1] - a[-2]
        out.append(g)
    return out


def hillshade(src, resolution, azimuth_deg):
    dy, dx = gradient(src)
    s = np.float32(15 * resolution / 90)
    dy, dx = dy / s, dx / s
    slope = np.float32(np.pi / 2.0) - np.arctan(np.hypot(dx, dy))
    aspect = np.arctan2(dy, -dx)
    az, alt = np.deg2rad(azimuth_deg), np.deg2rad(45.0)
    hs = np.sin(alt) * np.sin(slope).astype(np.float64) + np.cos(alt) * np.cos(slope).astype(np.float64) * np.cos(az - aspect.astype(np.float64))
    return np.clip(hs, 0.0, 1.0).astype(np.float32)


def relief(elevation, *, azimuths=(315.0, 45.0, 135.0, 225.0), sigma_large=6.0, sigma_small=1.2, resolution=90, relief=1.0, vmin=None, vmax=None):
    elev = np.asarray(elevation, dtype=np.float32)
    az = float(azimuths[0]) if isinstance(azimuths, (tuple, list)) and len(azimuths) > 0 else 315.0
    nan = np.isnan(elev)
    filled = elev
    if nan.any():
        med = np.nanmedian(elev)
        filled = np.nan_to_num(elev, nan=float(med) if np.isfinite(med) else 0.0)
    hs = np.clip(np.float32(0.75) * hillshade(gaussian_blur(filled, sigma_large), resolution, az)
                 + np.float32(0.25) * hillshade(gaussian_blur(filled, sigma_small), resolution, az), 0.0, 1.0) ** np.float32(0.85)
    land = np.where(nan, np.float32(np.nan), np.maximum(elev, np.float32(0)))
    if vmin is None or vmax is None:
        lo, hi = (float(np.nanmin(land)), float(np.nanmax(land))) if not nan.all() else (np.nan, np.nan)
        if not np.isfinite(lo) or not np.isfinite(hi) or lo == hi:
            lo, hi = 0.0, 1.0
    else:
        lo, hi = max(0.0, float(vmin)), float(vmax)
    norm = (land - np.float32(lo)) / np.float32(hi - lo + 1e-8)
    with np.errstate(invalid="ignore"):
        q = np.clip(norm ** np.float32(0.7), 0.0, 1.0)
    if lo == 0.0:
        q = np.float32(0.25) + q * np.float32(0.75)
    xi = q * np.float32(256)
    xi[xi == 256] = 255
    bad = np.isnan(xi)
    idx = np.clip(np.where(bad, 0, xi).astype(np.int64), 0, 255)
    base = terrain_lut()[idx]
    base[bad] = 0.0
    m = np.float32(relief) * (np.float32(0.35) + np.float32(0.65) * hs) + np.float32(1 - relief)
    out = np.clip(base * m[..., None], 0.0, 1.0).astype(np.float32)
    out[nan] = np.nan
    ocean = filled < 0
    t = np.clip(-filled / np.float32(10000.0), 0.0, 1.0) ** np.float32(0.7)
    col = (np.float32(1) - t)[..., None] * np.array([0.68, 0.88, 1.00], np.float32) + t[..., None] * np.array([0.00, 0.10, 0.45], np.float32)
    return np.where(ocean[..., None], col, out).astype(np.float32)


def compare(got, want, tol=1e-4, step_tol=0.025, step_frac=1e-3):
    """The relief tests' bound: identical NaN positions, |diff| <= tol everywhere except at most step_frac of the pixels (a colormap index one
    step away), which stay within step_tol.  Returns a message, or None when the images agree."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return f"NaN positions differ at {int((gn != wn).sum())} values"
    d = np.abs(np.where(wn, 0, got - want)).max(axis=-1) if got.ndim == 3 else np.abs(np.where(wn, 0, got - want))
    off = d > tol
    if d.max() > step_tol or off.sum() > step_frac * d.size:
        return f"max |diff| {d.max():.3g}, {int(off.sum())} of {d.size} pixels above {tol}"
    return None
