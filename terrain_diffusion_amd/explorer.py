"""The explorer views on the GPU: what the reference's terrain explorer (terrain_diffusion/inference/explorer/server.py: /api/coarse.png,
/api/coarse_stats, /api/coarse_data.json, /api/detail.png, /api/detail_raw) and its random sampler (inference/random_sampler.py:
sample_land_tiles, get_coarse_climate_info) compute after world.coarse[...] and world.get(...).

The work runs in explorer_csrc/explorer_kernels.hip through include/td_explorer.h (libtd_explorer.so), on the engine's stream: the coarse
planes in real units with their NaN-ignoring ranges from one pass, matplotlib's Normalize + colormap lookup + filter dimming + imsave's
quantisation as one kernel behind a device-side range, the raw int16 / fp32 tile, and the sampler's land-fraction search as two separable
box sums and an ordered compaction.

Two layers:
  * device forms -- coarse_channels, colorize, relief_rgba8, raw_tile, land_tiles -- take and return device tensors on the engine's stream
    and only enqueue inside Engine.on_stream(..., asynchronous=True), as relief_map does;
  * drop-ins -- coarse_image, coarse_stats, coarse_data, detail_image, detail_raw, sample_land_tiles, get_coarse_climate_info -- return what
    the reference's route or function returns, for any `world` with .coarse, .get, .seed and .native_resolution.  Each reads the coarse
    region once and makes ONE device-to-host copy (relief mode adds relief_map's NaN check; sample_land_tiles makes two, whatever the window).
There is no Flask app here (DESIGN.md keeps the servers out of scope): these functions are what a route body calls, and png_bytes encodes an
image without matplotlib or PIL.  There is no CPU fallback.
"""
import ctypes as C
import functools
import random
import struct
import zlib

import numpy as np
import torch

from . import relief as _relief
from ._lib import Library
from ._plumbing import MAX_PIXELS, MAX_SIDE, call, engine_for as _engine_for, f32 as _f32, hw, shape as _shape  # noqa: F401
from .engine import get_engine

_P = C.c_void_p
_SIGS = {
    "td_explorer_last_error": (C.c_char_p, []),
    "td_explorer_channels": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P, C.c_int]),
    "td_explorer_colorize": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P,
                                       C.c_int]),
    "td_explorer_quantize": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int]),
    "td_explorer_raw": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int]),
    "td_explorer_land_tiles": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P, C.c_int]),
}
EXPORTS = tuple(_SIGS)
MAX_CHANNELS = 8
MAX_FILTERS = 8
MAX_HALF = 2047
CHANNEL_NAMES = ["Elev", "p5", "Temp", "T std", "Precip", "Precip CV"]
FILTERABLE = (0, 2, 3, 4, 5)   # server.py: p5 (channel 1) cannot be filtered on
HOST_COPIES = 0                # device-to-host copies made by this module so far: each is one host synchronisation
_LIB = Library("libtd_explorer.so", _SIGS, "td_explorer_last_error", "td_explorer")
LIB_PATH, lib, check = _LIB.path, _LIB.lib, _LIB.check


# ------------------------------------------------------------------------------------------------------------------------------ colour tables
_RDBU = ((103, 0, 31), (178, 24, 43), (214, 96, 77), (244, 165, 130), (253, 219, 199), (247, 247, 247), (209, 229, 240), (146, 197, 222),
         (67, 147, 195), (33, 102, 172), (5, 48, 97))   # ColorBrewer RdBu, 11 classes


@functools.lru_cache(maxsize=None)
def colormap_lut(name):
    """(256, 3) read-only float32 rows of 'viridis', 'terrain' or 'RdBu_r': matplotlib's cmap(np.arange(256))[:, :3] as fp32."""
    if name == "terrain":
        return _relief.terrain_lut()
    if name == "viridis":
        from ._viridis import VIRIDIS
        out = np.asarray(VIRIDIS, dtype=np.float64).astype(np.float32)
    elif name == "RdBu_r":
        # RdBu is from_list over linspace(0, 1, 11); the reversed map runs through (1.0 - x, colour) of the reversed list
        pos = [1.0 - x for x in reversed(np.linspace(0, 1, len(_RDBU)))]
        out = _relief._segment_lut(pos, [tuple(v / 255 for v in rgb) for rgb in reversed(_RDBU)])
    else:
        raise ValueError(f"unknown colormap {name!r}: 'viridis', 'terrain' or 'RdBu_r' (or pass a (256, 3) table)")
    out.flags.writeable = False
    return out


@functools.lru_cache(maxsize=16)
def _device_lut(device_index, name):
    t = torch.from_numpy(np.array(colormap_lut(name))).to(torch.device("cuda", device_index))
    torch.cuda.synchronize(t.device)   # complete before any stream reads it (once per table and GPU)
    return t


# ---------------------------------------------------------------------------------------------------------------------------------- plumbing
def _hw(H, W):
    return hw(H, W, "field")


def _plane(x, what):
    if len(_shape(x)) != 2:
        raise ValueError(f"{what} must be (H, W), got {_shape(x)}")
    return _hw(*_shape(x))


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _host(*tensors):
    """ONE device-to-host copy of several device tensors (packed as bytes on the device) -> numpy arrays of their dtypes and shapes."""
    global HOST_COPIES
    flat = [t.contiguous().reshape(-1).view(torch.uint8) for t in tensors]
    blob = (flat[0] if len(flat) == 1 else torch.cat(flat)).cpu().numpy()
    HOST_COPIES += 1
    out, at = [], 0
    for t, f in zip(tensors, flat):
        n = f.numel()
        out.append(blob[at:at + n].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(_shape(t)))
        at += n
    return out


# ------------------------------------------------------------------------------------------------------------------------------ device forms
def _check_channels(sums, n_signed_sq, eps):
    if len(_shape(sums)) != 3:
        raise ValueError(f"coarse must be (C + 1, H, W), got {_shape(sums)}")
    Cn = _shape(sums)[0] - 1
    if Cn < 1 or Cn > MAX_CHANNELS:
        raise ValueError(f"coarse needs 1..{MAX_CHANNELS} channels and the weight plane, got {Cn + 1} planes")
    H, W = _hw(*_shape(sums)[1:])
    if not 0 <= int(n_signed_sq) <= Cn:
        raise ValueError(f"n_signed_sq must be in 0..{Cn}, got {n_signed_sq}")
    if not (np.isfinite(eps) and eps >= 0):
        raise ValueError(f"eps must be finite and >= 0, got {eps!r}")
    return Cn, H, W


def _channels(engine, dev, sums, n_signed_sq, eps, enqueue_only):
    Cn, H, W = _check_channels(sums, n_signed_sq, eps)
    s = _f32(sums, dev)
    out = torch.empty((Cn, H, W), dtype=torch.float32, device=dev)
    minmax = torch.empty((Cn, 2), dtype=torch.float32, device=dev)
    call(_LIB, "td_explorer_channels", engine, dev, _dp(s), Cn, H, W, int(n_signed_sq), float(eps), _dp(out), _dp(minmax),
         enqueue_only=enqueue_only, ordered=True)
    return out, minmax


@torch.no_grad()
def coarse_channels(coarse, *, n_signed_sq=2, eps=1e-8, engine=None):
    """coarse (C + 1, H, W) weighted sums with the weight plane last (world.coarse[:, a:b, c:d]) -> (planes (C, H, W), minmax (C, 2)) fp32
    device tensors: planes = sum / (weight + eps) in real units -- signed square for the first n_signed_sq channels -- bit-equal to torch's
    on the CPU, and each plane's NaN-ignoring minimum and maximum from the same pass.  eps = 0 is the sampler's normalize_tensor."""
    _check_channels(coarse, n_signed_sq, eps)
    engine, dev = _engine_for(coarse, engine)
    return _channels(engine, dev, coarse, n_signed_sq, eps, False)


def _check_colorize(field, cmap, vmin, vmax, filters):
    H, W = _plane(field, "field")
    if (vmin is None) != (vmax is None):
        raise ValueError("pass both vmin and vmax, or neither (the range is then the field's own)")
    if vmin is not None and not (np.isfinite(vmin) and np.isfinite(vmax) and float(vmin) < float(vmax)):
        raise ValueError(f"needs finite vmin < vmax, got {vmin!r}, {vmax!r}")
    if isinstance(cmap, str):
        colormap_lut(cmap)   # validates the name
    elif _shape(cmap) != (256, 3):
        raise ValueError(f"a colour table must be (256, 3), got {_shape(cmap)}")
    filters = list(filters)
    if len(filters) > MAX_FILTERS:
        raise ValueError(f"at most {MAX_FILTERS} filter planes, got {len(filters)}")
    for k, (plane, _, _) in enumerate(filters):
        if _shape(plane) != (H, W):
            raise ValueError(f"filter plane {k} {_shape(plane)} must have the field's shape {(H, W)}")
    return H, W, filters


def _filter_args(filters, dev):
    """[(plane (H, W), lo or None, hi or None)] -> ctypes arrays for td_explorer_colorize (and the tensors kept alive)."""
    keep, n = [], len(filters)
    planes, lo, hi = (_P * max(n, 1))(), (C.c_double * max(n, 1))(), (C.c_double * max(n, 1))()
    use_lo, use_hi = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))()
    for k, (plane, a, b) in enumerate(filters):
        t = _f32(plane, dev)
        keep.append(t)
        planes[k] = t.data_ptr()
        use_lo[k], use_hi[k] = int(a is not None), int(b is not None)
        lo[k], hi[k] = float(a) if a is not None else 0.0, float(b) if b is not None else 0.0
    return n, planes, lo, hi, use_lo, use_hi, keep


def _lut_for(cmap, dev):
    return _device_lut(dev.index, cmap) if isinstance(cmap, str) else _f32(cmap, dev)


def _colorize(engine, dev, field, cmap, log1p, vmin, vmax, filters, enqueue_only):
    H, W, filters = _check_colorize(field, cmap, vmin, vmax, filters)
    has_range = vmin is not None
    lut = _lut_for(cmap, dev)
    f = _f32(field, dev)
    n, planes, lo, hi, use_lo, use_hi, keep = _filter_args(filters, dev)
    out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    rng = torch.empty(2, dtype=torch.float32, device=dev)
    call(_LIB, "td_explorer_colorize", engine, dev, _dp(f), H, W, int(bool(log1p)), int(has_range), float(vmin) if has_range else 0.0,
         float(vmax) if has_range else 0.0, _dp(lut), n, planes, lo, hi, use_lo, use_hi, _dp(out), _dp(rng), enqueue_only=enqueue_only, ordered=True)
    del keep
    return out, rng


@torch.no_grad()
def colorize(field, cmap, *, log1p=False, vmin=None, vmax=None, filters=(), engine=None):
    """field (H, W) -> (rgba8 (H, W, 4) uint8, vmin, vmax) device tensors: matplotlib's cmap(Normalize(vmin, vmax)(d)) as fp32, dimmed by 0.3
    where a filter fails, clipped and quantised as plt.imsave does.  d = log1p(max(field, 0)) when log1p.  cmap: 'viridis', 'terrain',
    'RdBu_r' or a (256, 3) table.  Without vmin / vmax the range is the NaN-ignoring minimum and maximum of d, resolved on the device and used
    there; vmin and vmax come back as 0-d fp32 device tensors (the extremes as found: when they are equal the colours used vmax = vmin + 1,
    see resolved_range).  filters: up to 8 (plane (H, W), lo or None, hi or None); a pixel passes with plane >= lo and plane <= hi."""
    filters = _check_colorize(field, cmap, vmin, vmax, filters)[2]
    engine, dev = _engine_for(field, engine)
    out, rng = _colorize(engine, dev, field, cmap, log1p, vmin, vmax, filters, False)
    return out, rng[0], rng[1]


def resolved_range(vmin, vmax):
    """The (vmin, vmax) Python floats the colours were normalised with, from the two values colorize returned: vmax = vmin + 1 when equal."""
    vmin, vmax = float(vmin), float(vmax)
    return (vmin, vmin + 1) if vmax == vmin else (vmin, vmax)


def _check_rgb(rgb):
    if len(_shape(rgb)) != 3 or _shape(rgb)[2] != 3:
        raise ValueError(f"rgb must be (H, W, 3), got {_shape(rgb)}")
    return _hw(*_shape(rgb)[:2])


def _quantize(engine, dev, rgb, enqueue_only):
    H, W = _check_rgb(rgb)
    r = _f32(rgb, dev)
    out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    call(_LIB, "td_explorer_quantize", engine, dev, _dp(r), H, W, _dp(out), enqueue_only=enqueue_only, ordered=True)
    return out


@torch.no_grad()
def relief_rgba8(rgb, *, engine=None):
    """rgb (H, W, 3) fp32 (a relief_map result) -> (H, W, 4) uint8 device tensor: clip to [0, 1], truncate c * 255, alpha 255 -- the
    explorer's relief image as plt.imsave writes it.  A NaN channel becomes 0 (the reference's cast of NaN is undefined)."""
    _check_rgb(rgb)
    engine, dev = _engine_for(rgb, engine)
    return _quantize(engine, dev, rgb, False)


def _check_raw(elev, temp):
    H, W = _plane(elev, "elev")
    if temp is not None and _shape(temp) != (H, W):
        raise ValueError(f"temp {_shape(temp)} must have the elevation's shape {(H, W)}")
    return H, W


def _raw(engine, dev, elev, temp, enqueue_only):
    H, W = _check_raw(elev, temp)
    e = _f32(elev, dev)
    t = None if temp is None else _f32(temp, dev)
    out = torch.empty((6 if t is not None else 2) * H * W, dtype=torch.uint8, device=dev)
    call(_LIB, "td_explorer_raw", engine, dev, _dp(e), _dp(t), H, W, _dp(out), enqueue_only=enqueue_only, ordered=True)
    return out


@torch.no_grad()
def raw_tile(elev, temp=None, *, engine=None):
    """The body of /api/detail_raw as a uint8 device tensor: clip(floor(elev), -32768, 32767) as int16-le (2 H W bytes; NaN -> 0, the
    convention of minecraft_payload), then temp's fp32-le bytes (4 H W) when given."""
    _check_raw(elev, temp)
    engine, dev = _engine_for(elev, engine)
    return _raw(engine, dev, elev, temp, False)


def _check_land(elev_m, half, min_land_frac):
    H, W = _plane(elev_m, "elev_m")
    half = int(half)
    if half < 0 or half > MAX_HALF:
        raise ValueError(f"half must be in 0..{MAX_HALF}, got {half}")
    if 2 * half > H or 2 * half > W:
        raise ValueError(f"the {2 * half} x {2 * half} window is larger than the {H} x {W} plane")
    if np.isnan(min_land_frac):
        raise ValueError("min_land_frac is NaN")
    return H, W, half


def _land(engine, dev, elev_m, half, min_land_frac, enqueue_only):
    H, W, half = _check_land(elev_m, half, min_land_frac)
    e = _f32(elev_m, dev)
    cap = 0 if half == 0 else (H - 2 * half) * (W - 2 * half)
    idx = torch.empty(cap, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    call(_LIB, "td_explorer_land_tiles", engine, dev, _dp(e), H, W, half, float(min_land_frac), _dp(idx) if cap else None, _dp(count),
         enqueue_only=enqueue_only, ordered=True)
    return idx, count


@torch.no_grad()
def land_tiles(elev_m, half, min_land_frac, *, engine=None):
    """The sampler's search over elev_m (H, W) metres -> (idx int32 (capacity,), count int32 (1,)) device tensors: idx[:count] are the flat
    indices i * W + j, ascending, of the positions half <= i < H - half, half <= j < W - half whose 2 half x 2 half window has a land
    (elev_m > 0) fraction, formed as torch's fp32 mean, >= min_land_frac.  half 0 gives none."""
    _check_land(elev_m, half, min_land_frac)
    engine, dev = _engine_for(elev_m, engine)
    return _land(engine, dev, elev_m, half, min_land_frac, False)


# -------------------------------------------------------------------------------------------------------------------------------- drop-ins
def _world_engine(engine):
    engine = engine or get_engine(None)
    return engine, torch.device("cuda", engine.device_id)


def _coarse_region(world, ci0, ci1, cj0, cj1, engine, dev, eps=1e-8, n_signed_sq=2):
    """ONE read of world.coarse[:, ci0:ci1, cj0:cj1], divided once -> (planes, minmax) device tensors, enqueued only."""
    return _channels(engine, dev, world.coarse[:, int(ci0):int(ci1), int(cj0):int(cj1)], n_signed_sq, eps, True)


def _filter_bounds(filters):
    """{channel: (lo or None, hi or None)} -> [(channel, lo, hi)] for the filterable channels with a bound, in the reference's order."""
    out = []
    for ch in FILTERABLE:
        lo, hi = (filters or {}).get(ch, (None, None))
        if lo is not None or hi is not None:
            out.append((ch, lo, hi))
    return out


@torch.no_grad()
def coarse_image(world, channel=0, ci0=-50, ci1=50, cj0=-50, cj1=50, filters=None, *, engine=None):
    """/api/coarse.png -> (rgba8 ndarray (H, W, 4) -- the decoded pixels of the reference's PNG --, {"X-Vmin", "X-Vmax"}).
    filters: {channel: (lo or None, hi or None)} (the route's ch<k>_min / ch<k>_max); channels other than 0, 2, 3, 4, 5 are ignored, as there.
    The coarse region is read and divided once for the shown channel and every filter channel; one device-to-host copy."""
    channel = int(channel)
    engine, dev = _world_engine(engine)
    planes, _ = _coarse_region(world, ci0, ci1, cj0, cj1, engine, dev)
    if not 0 <= channel < planes.shape[0]:
        raise IndexError(f"channel {channel} outside 0..{planes.shape[0] - 1}")
    fl = [(planes[ch], lo, hi) for ch, lo, hi in _filter_bounds(filters) if ch < planes.shape[0]]
    rgba, rng = _colorize(engine, dev, planes[channel], "viridis", channel == 4, None, None, fl, True)
    img, r = _host(rgba, rng)
    vmin, vmax = resolved_range(r[0], r[1])
    return img, {"X-Vmin": str(round(vmin, 3)), "X-Vmax": str(round(vmax, 3))}


@torch.no_grad()
def coarse_stats(world, ci0=-50, ci1=50, cj0=-50, cj1=50, *, engine=None):
    """/api/coarse_stats -> {channel: {"name", "min", "max"}} (jsonify turns the integer keys into strings); min / max rounded to 3 places."""
    engine, dev = _world_engine(engine)
    _, minmax = _coarse_region(world, ci0, ci1, cj0, cj1, engine, dev)
    (mm,) = _host(minmax)
    return {ch: {"name": CHANNEL_NAMES[ch], "min": round(float(mm[ch, 0]), 3), "max": round(float(mm[ch, 1]), 3)} for ch in range(len(CHANNEL_NAMES))}


@torch.no_grad()
def coarse_data(world, ci0=-50, ci1=50, cj0=-50, cj1=50, *, engine=None):
    """/api/coarse_data.json -> {"ci0", "ci1", "cj0", "cj1", "channels": {name: rows rounded to 2 places}}."""
    engine, dev = _world_engine(engine)
    planes, _ = _coarse_region(world, ci0, ci1, cj0, cj1, engine, dev)
    (p,) = _host(planes)
    return {"ci0": int(ci0), "ci1": int(ci1), "cj0": int(cj0), "cj1": int(cj1),
            "channels": {name: np.round(p[i], 2).tolist() for i, name in enumerate(CHANNEL_NAMES)}}


def _detail_region(world, ci, cj, detail_size, pan_i, pan_j):
    center_i, center_j, half = int(ci) * 256 + int(pan_i), int(cj) * 256 + int(pan_j), int(detail_size) // 2
    return world.get(center_i - half, center_j - half, center_i + half, center_j + half)


def _relief_enqueue(engine, dev, e, resolution):
    """relief_map's render of a contiguous fp32 device image with its defaults, enqueued only (relief_map itself synchronises the host
    for every pointer it takes); the NaN check, and the median of an image that holds a NaN, are relief_map's own host reads."""
    _relief._check_shape(e.shape)
    H, W = _shape(e)
    has_fill = bool(torch.isnan(e).any())
    fill = _relief._nanmedian(e) if has_fill else None
    lut, wl, rl, ws, rs = _relief._device_tables(engine.device_id, 6.0, 1.2)
    out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    call(_relief._LIB, "td_relief_map", engine, dev, _dp(e), H, W, _dp(lut), _dp(wl), rl, _dp(ws), rs, float(_relief.DEFAULT_AZIMUTHS[0]),
         float(resolution), 1.0, 0, 0.0, 0.0, int(has_fill), float(fill) if has_fill else 0.0, _dp(out), enqueue_only=True, ordered=True)
    return out


@torch.no_grad()
def detail_image(world, ci=0, cj=0, detail_size=1024, pan_i=0, pan_j=0, mode="relief", *, engine=None):
    """/api/detail.png -> rgba8 ndarray (H, W, 4), the decoded pixels of the reference's PNG: 'elevation' (terrain colormap over the tile's
    own range), 'temperature' (RdBu_r of climate[0]; relief when the region has no climate), anything else relief (relief_map ->
    relief_rgba8).  One device-to-host copy, plus relief_map's NaN check in relief mode."""
    engine, dev = _world_engine(engine)
    region = _detail_region(world, ci, cj, detail_size, pan_i, pan_j)
    if mode == "elevation":
        rgba, _ = _colorize(engine, dev, region["elev"], "terrain", False, None, None, (), True)
    elif mode == "temperature" and region.get("climate") is not None:
        rgba, _ = _colorize(engine, dev, region["climate"][0], "RdBu_r", False, None, None, (), True)
    else:
        rgba = _quantize(engine, dev, _relief_enqueue(engine, dev, _f32(region["elev"], dev), world.native_resolution), True)
    return _host(rgba)[0]


@torch.no_grad()
def detail_raw(world, ci=0, cj=0, detail_size=1024, pan_i=0, pan_j=0, *, engine=None):
    """/api/detail_raw -> (body bytes, {"X-Height", "X-Width", "X-Has-Temp"}): int16-le elevation, then climate[0] as fp32-le when the
    region has climate.  Built on the device, copied to the host once."""
    engine, dev = _world_engine(engine)
    region = _detail_region(world, ci, cj, detail_size, pan_i, pan_j)
    climate = region.get("climate")
    H, W = _shape(region["elev"])
    body = _host(_raw(engine, dev, region["elev"], None if climate is None else climate[0], True))[0].tobytes()
    return body, {"X-Height": str(H), "X-Width": str(W), "X-Has-Temp": "1" if climate is not None else "0"}


@torch.no_grad()
def sample_land_tiles(world, coarse_window, detail_size, min_land_frac=0.5, n_samples=10, *, engine=None):
    """Drop-in for random_sampler.sample_land_tiles -> list of (ci, cj): the full list of valid tiles in the reference's order, then
    random.sample of it (seed `random` to get the reference's picks); the same warning and the whole list when there are too few.
    Two device-to-host copies (the count, then that many indices), whatever the window."""
    engine, dev = _world_engine(engine)
    ci0 = cj0 = -int(coarse_window)
    planes, _ = _coarse_region(world, ci0, -ci0, cj0, -cj0, engine, dev, eps=0.0)   # normalize_tensor: no epsilon
    W = int(planes.shape[2])
    half = (int(detail_size) // 256) // 2
    idx, count = _land(engine, dev, planes[0], half, min_land_frac, True)
    n = int(_host(count)[0][0])
    flat = _host(idx[:n])[0].astype(np.int64) if n else np.zeros(0, np.int64)
    valid_tiles = list(zip((ci0 + flat // W).tolist(), (cj0 + flat % W).tolist()))
    if len(valid_tiles) < n_samples:
        print(f"Warning: Only found {len(valid_tiles)} valid land tiles (requested {n_samples})")
        return valid_tiles
    return random.sample(valid_tiles, n_samples)


@torch.no_grad()
def get_coarse_climate_info(world, ci, cj, *, engine=None):
    """Drop-in for random_sampler.get_coarse_climate_info -> {"temp", "temp_std", "precip", "precip_cv"} of one coarse pixel."""
    engine, dev = _world_engine(engine)
    planes, _ = _coarse_region(world, ci, int(ci) + 1, cj, int(cj) + 1, engine, dev, eps=0.0, n_signed_sq=0)
    (p,) = _host(planes)
    return {"temp": float(p[2, 0, 0]), "temp_std": float(p[3, 0, 0]), "precip": float(p[4, 0, 0]), "precip_cv": float(p[5, 0, 0])}


# ------------------------------------------------------------------------------------------------------------------------------------- PNG
def png_bytes(rgba8):
    """A PNG file of an (H, W, 4) uint8 RGBA image: 8-bit RGBA, filter 0 on every row, from zlib and struct alone (no matplotlib, no PIL)."""
    a = np.ascontiguousarray(np.asarray(rgba8.cpu() if torch.is_tensor(rgba8) else rgba8))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"png_bytes needs an (H, W, 4) uint8 image, got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + 4 * W), np.uint8)   # a filter-type byte (0: none) before each row
    rows[:, 1:] = a.reshape(H, 4 * W)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6))
            + chunk(b"IEND", b""))
