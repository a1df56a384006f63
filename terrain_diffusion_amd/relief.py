"""Shaded-relief rendering of elevation: get_relief_map (terrain_diffusion/inference/relief_map.py:64-199) on the GPU.

The whole per-pixel path -- NaN fill, the two scipy Gaussian blurs, np.gradient hillshades, the terrain colormap, the relief blend, NaN and
ocean colouring -- runs in relief_csrc/relief_kernels.hip through td_relief_map (include/td_relief.h, libtd_relief.so), on the engine's
stream.  This module builds the two kinds of small table the kernels take, in the arithmetic of the libraries the reference calls, and keeps
them on the device per GPU:
  * matplotlib's "terrain" colormap as its 256-entry lookup table (LinearSegmentedColormap: linear interpolation between six control points);
    matplotlib itself is not imported,
  * scipy.ndimage.gaussian_filter's 1-D weights (truncate = 4, radius int(4 sigma + 0.5), normalised in float64).
biome, flow and a caller-supplied rgb image are not supported (no caller of the reference passes them).
The picture with those three inputs is rivers.get_relief_map (libtd_rivers.so, the same kernels with the overlay branch compiled in).
"""
import ctypes as C
import functools

import numpy as np
import torch

from ._lib import Library
from ._plumbing import call, engine_for, f32
from .engine import ptr

_P = C.c_void_p
_SIGS = {
    "td_relief_last_error": (C.c_char_p, []),
    "td_relief_map": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double,
                                C.c_double, C.c_int, C.c_double, _P, C.c_int]),
}
EXPORTS = tuple(_SIGS)
_LIB = Library("libtd_relief.so", _SIGS, "td_relief_last_error", "td_relief")
LIB_PATH, lib, check = _LIB.path, _LIB.lib, _LIB.check

DEFAULT_AZIMUTHS = (315.0, 45.0, 135.0, 225.0)
MAX_RADIUS = 64   # relief_csrc/relief_kernels.hip RELIEF_MAX_RADIUS: sigma below 15.9

# matplotlib's "terrain" colormap: (position, (r, g, b)) control points, linear in between
_TERRAIN_POINTS = ((0.00, (0.2, 0.2, 0.6)), (0.15, (0.0, 0.6, 1.0)), (0.25, (0.0, 0.8, 0.4)),
                   (0.50, (1.0, 1.0, 0.6)), (0.75, (0.5, 0.36, 0.33)), (1.00, (1.0, 1.0, 1.0)))


def _segment_lut(pos, colors, n=256):
    """(n, 3) float32 rows of a piecewise-linear colormap through `colors` at `pos`, as matplotlib's lookup-table builder forms them
    (float64, clipped to [0, 1])."""
    x = np.asarray(pos, dtype=np.float64) * (n - 1)
    xind = (n - 1) * np.linspace(0, 1, n)
    ind = np.searchsorted(x, xind)[1:-1]
    distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    lut = np.empty((n, 3), dtype=np.float64)
    for c in range(3):
        y = np.array([rgb[c] for rgb in colors], dtype=np.float64)
        lut[:, c] = np.concatenate([[y[0]], distance * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]])
    return np.clip(lut, 0.0, 1.0).astype(np.float32)


@functools.lru_cache(maxsize=4)
def terrain_lut(n=256):
    """(n, 3) read-only float32 RGB rows of the terrain colormap."""
    out = _segment_lut([p for p, _ in _TERRAIN_POINTS], [rgb for _, rgb in _TERRAIN_POINTS], n)
    out.flags.writeable = False
    return out


@functools.lru_cache(maxsize=64)
def gaussian_weights(sigma, truncate=4.0):
    """scipy.ndimage.gaussian_filter's 1-D weights for `sigma` -> (float32 weights of length 2 r + 1, r).  A sigma of at most 1e-15 leaves the
    image unchanged in scipy (the axis is skipped): weight [1], radius 0."""
    sigma = float(sigma)
    if not sigma >= 0.0:
        raise ValueError(f"sigma must be >= 0, got {sigma}")
    if sigma <= 1e-15:
        w = np.ones(1, dtype=np.float32)
        w.flags.writeable = False
        return w, 0
    r = int(truncate * sigma + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    w = (phi / phi.sum())[::-1].astype(np.float32)
    w.flags.writeable = False
    return w, r


@functools.lru_cache(maxsize=64)
def _device_tables(device_index, sigma_large, sigma_small):
    """(lut, wl, rl, ws, rs) with the three tables as device tensors: uploaded once per GPU and parameter set."""
    wl, rl = gaussian_weights(sigma_large)
    ws, rs = gaussian_weights(sigma_small)
    if rl > MAX_RADIUS or rs > MAX_RADIUS:
        raise ValueError(f"blur radius int(4 sigma + 0.5) above {MAX_RADIUS}: sigma_large={sigma_large}, sigma_small={sigma_small}")
    dev = torch.device("cuda", device_index)
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)
    tables = (up(terrain_lut()), up(wl), rl, up(ws), rs)
    torch.cuda.synchronize(dev)   # complete before any stream reads them (once per parameter set)
    return tables


def _check_shape(shape):
    if len(shape) != 2:
        raise ValueError(f"elevation must be (H, W), got shape {tuple(shape)}")
    if shape[0] < 2 or shape[1] < 2:
        raise ValueError(f"elevation needs at least 2 rows and 2 columns (np.gradient), got {tuple(shape)}")


def _nanmedian(e):
    """np.nanmedian of a device tensor with torch ops (torch.nanmedian returns the lower middle value; NumPy averages the two in fp32),
    then 0.0 when that is not finite (relief_map.py).  One host sync, for the scalar."""
    flat = e.reshape(-1)
    n = (~torch.isnan(flat)).sum()
    s = torch.sort(flat).values                       # NaN sorts last
    lo = torch.clamp((n - 1) // 2, min=0)
    hi = torch.clamp(n // 2, max=flat.numel() - 1)
    a, b = s[lo], s[hi]
    m = float(torch.where(lo == hi, a, (a + b) / 2))
    return m if np.isfinite(m) else 0.0   # an all-NaN image sorts NaN into s[0]


def _enqueue(engine, e, out, fill, azimuth, sigma_large, sigma_small, resolution, relief, vmin, vmax):
    """td_relief_map on the engine's stream for a contiguous fp32 device image `e` and output `out` (H, W, 3); fill = NaN fill or None.
    Synchronous unless the engine is in enqueue-only mode (Engine.on_stream / option "async")."""
    H, W = int(e.shape[0]), int(e.shape[1])
    lut, wl, rl, ws, rs = _device_tables(engine.device_id, float(sigma_large), float(sigma_small))
    has_range = vmin is not None and vmax is not None
    call(_LIB, "td_relief_map", engine, e.device, ptr(e), H, W, ptr(lut), ptr(wl), rl, ptr(ws), rs, float(azimuth), float(resolution), float(relief),
         int(has_range), float(vmin) if has_range else 0.0, float(vmax) if has_range else 0.0, int(fill is not None),
         float(fill) if fill is not None else 0.0, ptr(out))


@torch.no_grad()
def relief_map(elev, *, azimuths=DEFAULT_AZIMUTHS, sigma_large=6.0, sigma_small=1.2, resolution=90, relief=1.0, vmin=None, vmax=None, engine=None):
    """Shaded relief of a 2-D elevation tensor -> float32 (H, W, 3) tensor on the engine's device (no host copy of the image).

    Same arithmetic as the reference's get_relief_map with biome, flow and rgb None.  Only azimuths[0] is used (315 when azimuths is not a
    non-empty tuple or list).  The NaN check is one host sync per call; only an image that holds a NaN pays for the median (a device sort and
    a second sync for the fill value)."""
    _check_shape(elev.shape)
    H, W = int(elev.shape[0]), int(elev.shape[1])
    engine, dev = engine_for(elev, engine)
    e = f32(elev, dev)
    az = float(azimuths[0]) if isinstance(azimuths, (tuple, list)) and len(azimuths) > 0 else 315.0
    has_fill = bool(torch.isnan(e).any())
    fill = _nanmedian(e) if has_fill else None
    out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    _enqueue(engine, e, out, fill, az, sigma_large, sigma_small, resolution, relief, vmin, vmax)
    return out


def get_relief_map(elevation, climate, biome, flow, *, azimuths=DEFAULT_AZIMUTHS, flow_threshold=7, sigma_large=6.0, sigma_small=1.2,
                   resolution=90, rgb=None, relief=1.0, vmin=None, vmax=None, engine=None):
    """Drop-in for the reference's get_relief_map: numpy array or tensor (H, W) in metres -> numpy float32 (H, W, 3).
    `climate` is ignored, as in the reference; `flow_threshold` only matters with `flow`, which is not supported."""
    for name, value in (("biome", biome), ("flow", flow), ("rgb", rgb)):
        if value is not None:
            raise NotImplementedError(f"get_relief_map: `{name}` is not supported (only None)")
    e = elevation.detach() if torch.is_tensor(elevation) else np.asarray(elevation)
    _check_shape(e.shape)
    out = relief_map(e, azimuths=azimuths, sigma_large=sigma_large, sigma_small=sigma_small, resolution=resolution, relief=relief,
                     vmin=vmin, vmax=vmax, engine=engine)
    return out.cpu().numpy()
