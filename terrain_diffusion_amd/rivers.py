"""River maps on the GPU: the reference's get_relief_map WITH its biome, flow and rgb inputs (terrain_diffusion/inference/relief_map.py:64-199)
and smooth_river_bumps (terrain_diffusion/inference/postprocessing.py:87-135), through include/td_rivers.h (libtd_rivers.so) on the engine's
stream.

The relief picture is rendered by relief_csrc/relief_kernels.hip, the kernels of libtd_relief.so: the shade kernel is one template, and with
rgb, biome and flow all None the picture equals relief.relief_map's bit for bit.  Three surfaces:
  * device forms -- relief_overlay_map, smooth_bumps: device tensors in and out, no host copy of an image;
  * river_relief_map: the device-resident chain depression fill -> (bump smoothing) -> D8 routing -> flow accumulation -> relief with the
    rivers drawn where the accumulation exceeds flow_threshold;
  * drop-ins with the reference's names, signatures and return type (numpy float32): get_relief_map, smooth_river_bumps.
The tables relief.py builds (colormap, Gaussian weights) and its NaN median are used as they are.  There is no CPU fallback.
"""
import ctypes as C
import functools

import numpy as np
import torch

from . import hydrology, relief as _relief
from ._lib import Library
from ._plumbing import call, engine_for, f32
from .engine import ptr

_P = C.c_void_p
_SIGS = {
    "td_rivers_last_error": (C.c_char_p, []),
    "td_rivers_relief": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double,
                                   C.c_double, C.c_int, C.c_double, _P, _P, _P, _P, C.c_double, _P, C.c_int]),
    "td_rivers_smooth": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, _P, C.c_int]),
}
EXPORTS = tuple(_SIGS)
_LIB = Library("libtd_rivers.so", _SIGS, "td_rivers_last_error", "td_rivers")
LIB_PATH, lib, check = _LIB.path, _LIB.lib, _LIB.check

DEFAULT_AZIMUTHS = _relief.DEFAULT_AZIMUTHS
MAX_SIDE = 1 << 20          # include/td_rivers.h: 2 <= H, W <= 2^20, smoothing also H * W < 2^31
MAX_ITERATIONS = 64

# Colours of the 31 Koeppen-Geiger classes (0 = unknown: the pixel keeps its base colour), uint8; the kernels take them / 255 in fp32.
# tests/test_rivers_cpu.py holds the table against the one recorded from the reference.
BIOME_PALETTE_U8 = np.array([
    (0, 0, 0), (16, 86, 24), (38, 120, 40), (187, 212, 92), (227, 192, 122), (217, 200, 163), (210, 168, 90), (203, 182, 136), (176, 156, 78),
    (162, 148, 84), (148, 140, 104), (132, 178, 96), (112, 164, 96), (96, 148, 96), (124, 186, 84), (96, 168, 84), (76, 140, 76), (120, 140, 160),
    (108, 130, 150), (96, 120, 140), (88, 112, 132), (136, 152, 176), (112, 136, 168), (100, 120, 160), (84, 104, 140), (120, 170, 120),
    (96, 150, 120), (72, 120, 110), (64, 96, 108), (173, 180, 180), (230, 238, 244)], dtype=np.uint8)
BIOME_PALETTE_U8.flags.writeable = False


def biome_palette():
    """(31, 3) float32 palette: uint8 / 255 in fp32, as the reference forms it."""
    return BIOME_PALETTE_U8.astype(np.float32) / np.float32(255.0)


@functools.lru_cache(maxsize=8)
def _device_palette(device_index):
    dev = torch.device("cuda", device_index)
    t = torch.from_numpy(biome_palette()).to(dev)
    torch.cuda.synchronize(dev)   # complete before any stream reads it (once per GPU)
    return t


def _as_input(x):
    return x.detach() if torch.is_tensor(x) else np.asarray(x)


def _check_hw(shape, what="elevation"):
    _relief._check_shape(shape)
    H, W = int(shape[0]), int(shape[1])
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what} (H, W) = {(H, W)} beyond 2^20 rows or columns")
    return H, W


def _check_overlays(H, W, rgb, flow):
    if rgb is not None and tuple(rgb.shape) != (H, W, 3):
        raise ValueError(f"rgb {tuple(rgb.shape)} must be {(H, W, 3)}")
    if flow is not None and tuple(flow.shape) != (H, W):
        raise ValueError(f"flow {tuple(flow.shape)} must have the elevation's shape {(H, W)}")


def _biome_ids(biome, dev):
    """int32 device ids of any integer or floating biome image.  A floating one is truncated toward zero like astype(int32), NaN counts as 0
    (our own statement: that cast is undefined in NumPy).  Ids are limited to [-1, 31] before the cast, which the kernel's clip to [0, 30]
    cannot tell from the full value."""
    b = biome if torch.is_tensor(biome) else torch.from_numpy(np.ascontiguousarray(biome))
    b = b.to(dev)
    if b.is_floating_point():
        b = torch.nan_to_num(b, nan=0.0).trunc()
    elif b.dtype not in (torch.int32, torch.int64):
        b = b.to(torch.int32 if b.element_size() < 4 else torch.int64)   # bool and the unsigned types cannot hold the clamp's -1
    return b.clamp(-1, 31).to(torch.int32).contiguous()


def _enqueue(engine, e, out, fill, rgb, biome, flow, flow_threshold, azimuth, sigma_large, sigma_small, resolution, relief, vmin, vmax):
    """td_rivers_relief on the engine's stream for contiguous device tensors: fp32 `e` (H, W) and `out` (H, W, 3), fp32 rgb / int32 biome / fp32
    flow or None; fill = NaN fill or None.  Synchronous unless the engine is in enqueue-only mode (Engine.on_stream / option "async")."""
    H, W = int(e.shape[0]), int(e.shape[1])
    lut, wl, rl, ws, rs = _relief._device_tables(engine.device_id, float(sigma_large), float(sigma_small))
    pal = _device_palette(engine.device_id) if biome is not None else None
    has_range = vmin is not None and vmax is not None
    call(_LIB, "td_rivers_relief", engine, e.device, ptr(e), H, W, ptr(lut), ptr(wl), rl, ptr(ws), rs, float(azimuth), float(resolution), float(relief),
         int(has_range), float(vmin) if has_range else 0.0, float(vmax) if has_range else 0.0, int(fill is not None),
         float(fill) if fill is not None else 0.0, ptr(rgb), ptr(biome), ptr(pal), ptr(flow), float(flow_threshold), ptr(out))


@torch.no_grad()
def relief_overlay_map(elev, *, rgb=None, biome=None, flow=None, flow_threshold=7, azimuths=DEFAULT_AZIMUTHS, sigma_large=6.0, sigma_small=1.2,
                       resolution=90, relief=1.0, vmin=None, vmax=None, engine=None):
    """Shaded relief of a 2-D elevation with the reference's overlays -> float32 (H, W, 3) tensor on the engine's device (no host copy of an
    image).  rgb (H, W, 3) replaces the terrain colormap (vmin / vmax then mean nothing); biome (H, W), any integer tensor or array (floating:
    truncated toward zero, NaN = 0), paints palette[id] where clip(id, 0, 30) > 0, on top of rgb too; flow (H, W) draws a river where
    flow > fl32(flow_threshold); the ocean ramp comes last and overwrites rivers.  With all three None this is relief.relief_map, bit for bit.
    Wrong shapes raise ValueError.  Host syncs as relief_map: one for the NaN check, a second for the median when there is a NaN."""
    elev, rgb, biome, flow = (None if a is None else _as_input(a) for a in (elev, rgb, biome, flow))
    H, W = _check_hw(elev.shape)
    _check_overlays(H, W, rgb, flow)
    if biome is not None and tuple(biome.shape) != (H, W):
        raise ValueError(f"biome {tuple(biome.shape)} must have the elevation's shape {(H, W)}")
    engine, dev = engine_for(elev, engine)
    e = f32(elev, dev)
    az = float(azimuths[0]) if isinstance(azimuths, (tuple, list)) and len(azimuths) > 0 else 315.0
    c = f32(rgb, dev) if rgb is not None else None
    b = _biome_ids(biome, dev) if biome is not None else None
    fl = f32(flow, dev) if flow is not None else None
    fill = _relief._nanmedian(e) if bool(torch.isnan(e).any()) else None
    out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    _enqueue(engine, e, out, fill, c, b, fl, flow_threshold, az, sigma_large, sigma_small, resolution, relief, vmin, vmax)
    return out


def _check_iterations(iterations):
    it = int(iterations)
    if it != iterations or not 0 <= it <= MAX_ITERATIONS:
        raise ValueError(f"iterations must be an integer in [0, {MAX_ITERATIONS}], got {iterations}")
    return it


@torch.no_grad()
def smooth_bumps(height, slope_thresh=50, smooth_strength=0.3, iterations=3, *, engine=None):
    """smooth_river_bumps of a 2-D elevation -> float32 device tensor (a new one; the input is left as it is).  Each iteration is the reference's,
    in fp32 and its operation order: a 4-neighbour Laplacian that wraps around the image (np.roll) and skips NaN neighbours, weighted by
    exp(-(slope / slope_thresh)^2) of the np.gradient slope.  NaN cells stay NaN.  0 <= iterations <= 64; 0 copies."""
    height = _as_input(height)
    H, W = _check_hw(height.shape, "height")
    if H * W >= 1 << 31:
        raise ValueError(f"height (H, W) = {(H, W)}: H * W must stay below 2^31")
    it = _check_iterations(iterations)
    engine, dev = engine_for(height, engine)
    h = f32(height, dev)
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    call(_LIB, "td_rivers_smooth", engine, dev, ptr(h), H, W, float(slope_thresh), float(smooth_strength), it, ptr(out))
    return out


@torch.no_grad()
def river_relief_map(elev, *, fill=True, smooth=False, flow_threshold=7, biome=None, engine=None, **relief_kw):
    """The relief picture of `elev` with its rivers, device-resident: hydrology.fill_depressions (fill=True), smooth_bumps with its defaults
    (smooth=True), hydrology.flow_directions and flow_accumulation_map on that routed surface, then relief_overlay_map(elev, flow=accumulation).
    The CALLER'S elevation is shaded; only the routing sees the filled (and smoothed) one.  relief_kw goes to relief_overlay_map (azimuths,
    sigmas, resolution, relief, vmin, vmax, rgb).  No image is copied to the host; the syncs are those the pieces document (the fill's
    convergence flags, the accumulation's 4-byte count, the relief's NaN check).  H * W <= 2^24 (flow_accumulation_map)."""
    elev = _as_input(elev)
    H, W = _check_hw(elev.shape)
    engine, dev = engine_for(elev, engine)
    e = f32(elev, dev)
    routed = hydrology.fill_depressions(e, engine=engine) if fill else e
    if smooth:
        routed = smooth_bumps(routed, engine=engine)
    receiver, _, sink = hydrology.flow_directions(routed, engine=engine)
    acc = hydrology.flow_accumulation_map(routed, receiver, sink, engine=engine)
    return relief_overlay_map(e, biome=biome, flow=acc, flow_threshold=flow_threshold, engine=engine, **relief_kw)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Drop-ins: the reference's names, signatures and return type.

def get_relief_map(elevation, climate, biome, flow, *, azimuths=DEFAULT_AZIMUTHS, flow_threshold=7, sigma_large=6.0, sigma_small=1.2,
                   resolution=90, rgb=None, relief=1.0, vmin=None, vmax=None, engine=None):
    """Drop-in for the reference's get_relief_map with its full signature: numpy arrays or tensors -> numpy float32 (H, W, 3).  `climate` is
    ignored, as in the reference.  A `biome` whose shape is not the elevation's is silently ignored, as in the reference; a `flow` or `rgb` of
    the wrong shape raises ValueError (the reference asserts, or fails to broadcast).  One difference: a float64 `rgb` is rounded to fp32
    first and the result is float32; the reference would carry it, and return, float64."""
    e = _as_input(elevation)
    if biome is not None and tuple(_as_input(biome).shape) != tuple(e.shape):
        biome = None
    out = relief_overlay_map(e, rgb=rgb, biome=biome, flow=flow, flow_threshold=flow_threshold, azimuths=azimuths, sigma_large=sigma_large, sigma_small=sigma_small,
                             resolution=resolution, relief=relief, vmin=vmin, vmax=vmax, engine=engine)
    return out.cpu().numpy()


def smooth_river_bumps(height, slope_thresh=50, smooth_strength=0.3, iterations=3, *, engine=None):
    """Drop-in for the reference's smooth_river_bumps -> numpy float32 (a new array)."""
    return smooth_bumps(height, slope_thresh, smooth_strength, iterations, engine=engine).cpu().numpy()
