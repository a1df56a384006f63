"""NumPy restatement of what libtd_rivers.so computes (include/td_rivers.h), written from the operator definitions: the relief picture with
its rgb / biome / river overlays over the pieces of tests/_relief_twin.py (blur, hillshade, colormap table, land_and_sea, compare), and
smooth_river_bumps in the kernel's operation order, in fp32 (`smooth`) and carried in float64 from the same fp32 input (`smooth_d64`, D64:
what the GPU test's bound is measured against)."""
import numpy as np

import _relief_twin as rt

land_and_sea, compare = rt.land_and_sea, rt.compare
F = np.float32
RIVER = np.array([0.100, 0.450, 0.850], F)


def palette(u8):
    """the (31, 3) fp32 palette of a uint8 table: / 255 in fp32"""
    return np.asarray(u8).astype(F) / F(255.0)


def relief(elevation, *, pal=None, rgb=None, biome=None, flow=None, flow_threshold=7, azimuths=(315.0, 45.0, 135.0, 225.0), sigma_large=6.0,
           sigma_small=1.2, resolution=90, relief=1.0, vmin=None, vmax=None):
    """get_relief_map with its overlays; with rgb, biome and flow None it is _relief_twin.relief.  `pal`: (31, 3) fp32, needed with biome."""
    elev = np.asarray(elevation, dtype=F)
    az = float(azimuths[0]) if isinstance(azimuths, (tuple, list)) and len(azimuths) > 0 else 315.0
    nan = np.isnan(elev)
    filled = elev
    if nan.any():
        med = np.nanmedian(elev)
        filled = np.nan_to_num(elev, nan=float(med) if np.isfinite(med) else 0.0)
    hs = np.clip(F(0.75) * rt.hillshade(rt.gaussian_blur(filled, sigma_large), resolution, az)
                 + F(0.25) * rt.hillshade(rt.gaussian_blur(filled, sigma_small), resolution, az), 0.0, 1.0) ** F(0.85)
    if rgb is not None:
        base = np.array(rgb, dtype=F)
    else:
        land = np.where(nan, F(np.nan), np.maximum(elev, F(0)))
        if vmin is None or vmax is None:
            lo, hi = (float(np.nanmin(land)), float(np.nanmax(land))) if not nan.all() else (np.nan, np.nan)
            if not np.isfinite(lo) or not np.isfinite(hi) or lo == hi:
                lo, hi = 0.0, 1.0
        else:
            lo, hi = max(0.0, float(vmin)), float(vmax)
        with np.errstate(invalid="ignore"):
            q = np.clip(((land - F(lo)) / F(hi - lo + 1e-8)) ** F(0.7), 0.0, 1.0)
        if lo == 0.0:
            q = F(0.25) + q * F(0.75)
        xi = q * F(256)
        xi[xi == 256] = 255
        bad = np.isnan(xi)
        base = rt.terrain_lut()[np.clip(np.where(bad, 0, xi).astype(np.int64), 0, 255)]
        base[bad] = 0.0
    if biome is not None:
        ids = np.clip(np.asarray(biome).astype(np.int64), 0, 30)
        base = np.where((ids > 0)[..., None], np.asarray(pal, F)[ids], base)
    m = F(relief) * (F(0.35) + F(0.65) * hs) + F(1 - relief)
    out = np.clip(base * m[..., None], 0.0, 1.0).astype(F)
    out[nan] = np.nan
    if flow is not None:
        with np.errstate(invalid="ignore"):
            river = np.asarray(flow, F) > F(flow_threshold)
        out[river] = F(0.25) * out[river] + F(0.75) * RIVER
    t = np.clip(-filled / F(10000.0), 0.0, 1.0) ** F(0.7)
    col = (F(1) - t)[..., None] * np.array([0.68, 0.88, 1.00], F) + t[..., None] * np.array([0.00, 0.10, 0.45], F)
    return np.where((filled < 0)[..., None], col, out).astype(F)


def _gradient(f, axis):
    """np.gradient along one axis: central differences / 2 inside, one-sided at the two edges"""
    a = np.moveaxis(f, axis, 0)
    g = np.empty_like(a)
    g[1:-1] = (a[2:] - a[:-2]) / a.dtype.type(2)
    g[0] = a[1] - a[0]
    g[-1] = a[-1] - a[-2]
    return np.moveaxis(g, 0, axis)


def _smooth(h32, slope_thresh, smooth_strength, iterations, T):
    """smooth_river_bumps with every operation in dtype T; the two scalars are the fp32 roundings of the Python floats in either case (what
    NumPy >= 2 makes of them beside a float32 array), so that T = float64 differs from the reference by rounding alone."""
    h = np.asarray(h32, dtype=F).astype(T)
    nan = np.isnan(h)
    thresh, strength = T(F(slope_thresh)), T(F(smooth_strength))
    valid = (~nan).astype(T)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _ in range(int(iterations)):
            hs = np.where(nan, T(0), h)
            gy, gx = _gradient(hs, 0), _gradient(hs, 1)
            slope = np.sqrt(gx * gx + gy * gy)
            nb = [(np.roll(hs, s, a), np.roll(valid, s, a)) for s, a in ((1, 0), (-1, 0), (1, 1), (-1, 1))]   # up, down, left, right: wrapped
            total = ((nb[0][0] + nb[1][0]) + nb[2][0]) + nb[3][0]
            cnt = ((nb[0][1] + nb[1][1]) + nb[2][1]) + nb[3][1]
            lap = total - cnt * hs
            q = slope / thresh
            w = np.exp(-(q * q))
            h = np.where(nan, T(np.nan), hs + (strength * w) * lap)
    return h


def smooth(h32, slope_thresh=50, smooth_strength=0.3, iterations=3):
    """fp32, in the kernel's order (numpy's exp for the device's)"""
    return _smooth(h32, slope_thresh, smooth_strength, iterations, F)


def smooth_d64(h32, slope_thresh=50, smooth_strength=0.3, iterations=3):
    """D64: the same formula in float64 from the same fp32 input"""
    return _smooth(h32, slope_thresh, smooth_strength, iterations, np.float64)


def ulp32(x):
    """one fp32 unit in the last place at magnitude x"""
    return float(np.spacing(F(abs(x))))
