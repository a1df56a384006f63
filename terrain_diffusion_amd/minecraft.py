"""The Minecraft terrain path on the GPU: the per-request tail of the reference's Minecraft terrain server (terrain_diffusion/inference/
minecraft_api.py: _get_upsampled, _classify_biome, _binary_response, and what _handle_1x / _handle_upsampled compute from them) and of its
REST server's scaled path (api.py: _get_terrain).

The work runs in mc_csrc/mc_kernels.hip through include/td_mc.h (libtd_mc.so), on the engine's stream: a bilinear upsample evaluated only on
the requested box, one fused pass (Sobel, detail noise, climate variables, the biome decision tree) and the int16 payload, which leaves the
device in one copy.  The drop-ins take the reference's names and signatures and any `world` with .get(i1, j1, i2, j2, with_climate=) and
.native_resolution (WorldPipeline, or the reference's), and return device tensors.

Noise: the reference evaluates seven FastNoiseLite Perlin-FBm generators on the host.  pyfastnoiselite is not a dependency, so the built-in
noise is this package's own FBm Perlin noise with the generators' seeds, frequencies, octaves and gains.  Pass
noise_fn(name, coords) -> (N,) float32 -- called with the reference's generator names (NOISE_NAMES) and its (2, N) fp32 coordinate array
(x = absolute column, y = absolute row) -- to use other values, e.g. the reference's own: noise_fn=lambda n, c: getattr(ref, n).gen_from_coords(c).
Index arithmetic is Python's (floor division, also for negative coordinates); noise coordinates are exact for |i|, |j| < 2^24.
Inputs of other dtypes are cast to fp32.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import Library
from ._plumbing import MAX_PIXELS, MAX_SIDE, call, engine_for as _engine_for, f32 as _f32, hw, shape as _shape  # noqa: F401
from .engine import get_engine, ptr

_P = C.c_void_p
_LL = C.c_longlong
_SIGS = {
    "td_mc_last_error": (C.c_char_p, []),
    "td_mc_upsample": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _LL, _LL, C.c_int, C.c_int, _P, C.c_int]),
    "td_mc_finish": (C.c_int, [_P, _P, _LL, _P, _P, C.c_int, C.c_int, C.c_int, _LL, _LL, _P, C.c_double, C.c_double, C.c_double, C.c_double,
                               _P, _P, C.c_int]),
    "td_mc_noise": (C.c_int, [_P, C.c_int, C.c_int, _LL, _LL, _P, C.c_int]),
    "td_mc_payload": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, C.c_int]),
}
EXPORTS = tuple(_SIGS)
NOISE_NAMES = ("_TEMP_NOISE", "_TEMP_NOISE_FINE", "_PRECIP_NOISE", "_SNOW_NOISE", "_SNOW_NOISE_FINE", "_ELEV_NOISE_COARSE", "_ELEV_NOISE_FINE")
_CLIMATE_NOISE, _DETAIL_NOISE = (0, 1, 2, 3, 4), (5, 6)
_LIB = Library("libtd_mc.so", _SIGS, "td_mc_last_error", "td_mc")
LIB_PATH, lib, check = _LIB.path, _LIB.lib, _LIB.check


# ----------------------------------------------------------------------------------------------------------------------------- validation
def _scale(scale):
    if isinstance(scale, bool) or not float(scale).is_integer() or int(scale) < 1:
        raise ValueError(f"scale must be an integer >= 1, got {scale!r}")
    return int(scale)


def _hw(H, W):
    return hw(H, W, "box")


def _box(i1, j1, i2, j2):
    i1, j1, i2, j2 = int(i1), int(j1), int(i2), int(j2)
    return (i1, j1, i2, j2) + _hw(i2 - i1, j2 - j1)


def _native_box(i1, j1, i2, j2, s, pad):
    """The native window of a scaled box: Python's floor division for the start, ceil division for the end, `pad` native pixels around."""
    return i1 // s - pad, j1 // s - pad, -(-i2 // s) + pad, -(-j2 // s) + pad


def _check_climate(climate, H, W):
    if climate is not None and (len(_shape(climate)) != 3 or _shape(climate)[1:] != (H, W)):
        raise ValueError(f"climate {_shape(climate)} must be (C, {H}, {W})")


# ---------------------------------------------------------------------------------------------------------------------------------- plumbing
def _fetch(world, box, with_climate, dev):
    """world.get of a native box -> (elev (h, w), climate (C, h, w) or None) as fp32 device tensors, shapes checked."""
    a, b, c, d = box
    out = world.get(a, b, c, d, with_climate=with_climate)
    elev, climate = out["elev"], out.get("climate")
    if _shape(elev) != (c - a, d - b):
        raise ValueError(f"world.get{box} returned elev {_shape(elev)}, expected {(c - a, d - b)}")
    _check_climate(climate, c - a, d - b)
    return _f32(elev, dev), (None if climate is None else _f32(climate, dev))


def _upsample(src, s, r0, c0, H, W, engine, dev):
    """Rows [r0, r0 + H) x columns [c0, c0 + W) of the bilinear upsample by s of src (C, Hn, Wn) -> (C, H, W)."""
    Cn, Hn, Wn = _shape(src)
    out = torch.empty((Cn, H, W), dtype=torch.float32, device=dev)
    call(_LIB, "td_mc_upsample", engine, dev, ptr(src), Cn, Hn, Wn, s, r0, c0, H, W, ptr(out))
    return out


def _noise_planes(noise_fn, i0, j0, H, W, which, dev):
    """The seven (7, H, W) planes from noise_fn for the generators in `which` (the others stay 0 and are not read), or None: built-in noise."""
    if noise_fn is None:
        return None
    xx, yy = np.meshgrid(np.arange(j0, j0 + W, dtype=np.float32), np.arange(i0, i0 + H, dtype=np.float32))
    coords = np.array([xx.ravel(), yy.ravel()], dtype=np.float32)
    planes = np.zeros((7, H, W), np.float32)
    for k in which:
        v = np.asarray(noise_fn(NOISE_NAMES[k], coords), dtype=np.float32)
        if v.size != H * W:
            raise ValueError(f"noise_fn({NOISE_NAMES[k]!r}) returned {v.size} values for {H * W} coordinates")
        planes[k] = v.reshape(H, W)
    return torch.from_numpy(planes).to(dev)


def _finish(engine, dev, elev, padded, climate, H, W, i0, j0, planes, noise_scale, detail_px, native_res, biome_px, elev_out, biome_out):
    """One td_mc_finish launch.  elev may be the (H, W) interior view of padded (row pitch W + 2)."""
    n_clim = 0 if climate is None else int(climate.shape[0])
    assert elev.stride(1) == 1 and (elev.is_contiguous() or elev.untyped_storage().data_ptr() == padded.untyped_storage().data_ptr())
    ep = ptr(elev) if elev.is_contiguous() else C.c_void_p(elev.data_ptr())    # a view of padded: ptr(padded) below orders it
    call(_LIB, "td_mc_finish", engine, dev, ep, elev.stride(0), ptr(padded), ptr(climate), n_clim, H, W, i0, j0, ptr(planes), float(noise_scale),
         float(detail_px), float(native_res), float(biome_px), ptr(elev_out), ptr(biome_out))


def _upsampled(world, i1, j1, i2, j2, s, H, W, engine):
    """The padded native window of a scaled box, upsampled on the device: (elev_padded (H + 2, W + 2), climate (C, H, W) or None)."""
    engine = engine or get_engine(None)
    dev = torch.device("cuda", engine.device_id)
    en, cn = _fetch(world, _native_box(i1, j1, i2, j2, s, 2), True, dev)
    r0 = 2 * s + (i1 - (i1 // s) * s)
    c0 = 2 * s + (j1 - (j1 // s) * s)
    padded = _upsample(en[None], s, r0 - 1, c0 - 1, H + 2, W + 2, engine, dev)[0]
    climate = None if cn is None else _upsample(cn, s, r0, c0, H, W, engine, dev)
    return engine, dev, padded, climate


# -------------------------------------------------------------------------------------------------------------------------------- drop-ins
@torch.no_grad()
def get_upsampled(world, i1, j1, i2, j2, scale, noise_scale=1.0, pixel_size_m=90.0, *, noise_fn=None, engine=None):
    """Drop-in for minecraft_api._get_upsampled -> {'elev', 'elev_smooth', 'climate', 'elev_padded'} device tensors.  Reads the native window
    with 2 pixels of padding, upsamples only the requested box (elev_padded: the box plus one pixel; elev_smooth is its interior view) and,
    when noise_scale > 0, adds the slope-scaled detail noise on land."""
    s = _scale(scale)
    i1, j1, i2, j2, H, W = _box(i1, j1, i2, j2)
    engine, dev, padded, climate = _upsampled(world, i1, j1, i2, j2, s, H, W, engine)
    smooth = padded[1:-1, 1:-1]
    elev = smooth
    if noise_scale > 0:
        elev = torch.empty((H, W), dtype=torch.float32, device=dev)
        planes = _noise_planes(noise_fn, i1, j1, H, W, _DETAIL_NOISE, dev)
        _finish(engine, dev, padded[1:-1, 1:-1], padded, None, H, W, i1, j1, planes, noise_scale, pixel_size_m, world.native_resolution,
                pixel_size_m, elev, None)
    return {"elev": elev, "elev_smooth": smooth, "climate": climate, "elev_padded": padded}


@torch.no_grad()
def classify_biome(elev, climate, i0, j0, elev_padded, pixel_size_m=90.0, *, noise_fn=None, engine=None):
    """Drop-in for minecraft_api._classify_biome -> int16 (H, W) device tensor of Minecraft biome ids.  climate None or with fewer than 4
    channels gives plains (1) everywhere; elev_padded is (H + 2, W + 2)."""
    if len(_shape(elev)) != 2:
        raise ValueError(f"elev must be (H, W), got {_shape(elev)}")
    H, W = _hw(*_shape(elev))
    if _shape(elev_padded) != (H + 2, W + 2):
        raise ValueError(f"elev_padded {_shape(elev_padded)} must be {(H + 2, W + 2)}")
    _check_climate(climate, H, W)
    engine, dev = _engine_for(elev, engine)
    e, p = _f32(elev, dev), _f32(elev_padded, dev)
    use_climate = climate is not None and int(climate.shape[0]) >= 4
    c = _f32(climate, dev) if use_climate else None
    planes = _noise_planes(noise_fn, int(i0), int(j0), H, W, _CLIMATE_NOISE, dev) if use_climate else None
    biome = torch.empty((H, W), dtype=torch.int16, device=dev)
    _finish(engine, dev, e, p, c, H, W, int(i0), int(j0), planes, 0.0, pixel_size_m, 1.0, pixel_size_m, None, biome)
    return biome


@torch.no_grad()
def get_terrain(world, i1, j1, i2, j2, scale, *, engine=None):
    """Drop-in for api._get_terrain -> {'elev' (H, W), 'climate' (C, H, W) or None}: at scale 1 world.get itself, otherwise the native window
    with 1 pixel of padding upsampled on the requested box only (no noise)."""
    s = _scale(scale)
    i1, j1, i2, j2, H, W = _box(i1, j1, i2, j2)
    if s == 1:
        out = world.get(i1, j1, i2, j2, with_climate=True)
        return {"elev": out["elev"], "climate": out.get("climate")}
    engine = engine or get_engine(None)
    dev = torch.device("cuda", engine.device_id)
    en, cn = _fetch(world, _native_box(i1, j1, i2, j2, s, 1), True, dev)
    r0 = s + (i1 - (i1 // s) * s)
    c0 = s + (j1 - (j1 // s) * s)
    return {"elev": _upsample(en[None], s, r0, c0, H, W, engine, dev)[0],
            "climate": None if cn is None else _upsample(cn, s, r0, c0, H, W, engine, dev)}


@torch.no_grad()
def minecraft_terrain(world, i1, j1, i2, j2, scale=1, noise_scale=1.0, *, noise_fn=None, engine=None):
    """(elev fp32 (H, W), biome int16 (H, W)) device tensors of a Minecraft terrain request: what the reference's _handle_1x (scale 1) and
    _handle_upsampled (scale > 1, pixel size native_resolution / scale) compute before _binary_response.  Scale 1 makes the reference's two
    world.get calls (the padded box without climate, then the box); otherwise one upsample of the padded native window and one fused pass
    for the detail noise and the biome."""
    s = _scale(scale)
    i1, j1, i2, j2, H, W = _box(i1, j1, i2, j2)
    nr = world.native_resolution
    if s == 1:
        engine = engine or get_engine(None)
        dev = torch.device("cuda", engine.device_id)
        padded, _ = _fetch(world, (i1 - 1, j1 - 1, i2 + 1, j2 + 1), False, dev)
        elev, climate = _fetch(world, (i1, j1, i2, j2), True, dev)
        return elev, classify_biome(elev, climate, i1, j1, padded, nr, noise_fn=noise_fn, engine=engine)
    engine, dev, padded, climate = _upsampled(world, i1, j1, i2, j2, s, H, W, engine)
    pix = nr / s
    use_climate = climate is not None and int(climate.shape[0]) >= 4
    detail = noise_scale > 0
    which = (_CLIMATE_NOISE if use_climate else ()) + (_DETAIL_NOISE if detail else ())
    planes = _noise_planes(noise_fn, i1, j1, H, W, which, dev) if which else None
    elev = torch.empty((H, W), dtype=torch.float32, device=dev) if detail else padded[1:-1, 1:-1]
    biome = torch.empty((H, W), dtype=torch.int16, device=dev)
    _finish(engine, dev, padded[1:-1, 1:-1], padded, climate if use_climate else None, H, W, i1, j1, planes, noise_scale, pix, nr, pix,
            elev if detail else None, biome)
    return elev, biome


@torch.no_grad()
def noise_planes(i0, j0, H, W, *, engine=None):
    """The built-in noise (7, H, W) fp32 device tensor of the box at absolute (i0, j0), in the reference's generator order (NOISE_NAMES):
    the values the drop-ins use when noise_fn is None."""
    H, W = _hw(int(H), int(W))
    engine = engine or get_engine(None)
    dev = torch.device("cuda", engine.device_id)
    out = torch.empty((7, H, W), dtype=torch.float32, device=dev)
    call(_LIB, "td_mc_noise", engine, dev, H, W, int(i0), int(j0), ptr(out))
    return out


@torch.no_grad()
def minecraft_payload(elev, biome=None, *, engine=None):
    """The reference's _binary_response -> (body bytes, headers): clip(floor(elev), -32768, 32767) as int16-le, then the biome ids as
    int16-le, built on the device and copied to the host once.  A NaN elevation is written as 0 (the reference's NumPy cast leaves it
    undefined)."""
    if len(_shape(elev)) != 2:
        raise ValueError(f"elev must be (H, W), got {_shape(elev)}")
    H, W = _hw(*_shape(elev))
    if biome is not None and _shape(biome) != (H, W):
        raise ValueError(f"biome {_shape(biome)} must have the elevation's shape {(H, W)}")
    engine, dev = _engine_for(elev, engine)
    e = _f32(elev, dev)
    b = None
    if biome is not None:
        b = (biome.detach() if torch.is_tensor(biome) else torch.from_numpy(np.ascontiguousarray(biome))).to(device=dev, dtype=torch.int16)
        b = b.contiguous()
    out = torch.empty((2 if b is not None else 1) * H * W, dtype=torch.int16, device=dev)
    call(_LIB, "td_mc_payload", engine, dev, ptr(e), ptr(b), H, W, ptr(out))
    body = out.cpu().numpy().astype("<i2", copy=False).tobytes()
    return body, {"X-Height": str(H), "X-Width": str(W), "X-Dtype": "int16-le"}


def parse_minecraft_payload(body, headers):
    """Inverse of minecraft_payload for clients: (elev int16 (H, W), biome int16 (H, W) or None) from the body and its headers."""
    if headers.get("X-Dtype", "int16-le") != "int16-le":
        raise ValueError(f"unsupported X-Dtype {headers.get('X-Dtype')!r}")
    H, W = int(headers["X-Height"]), int(headers["X-Width"])
    a = np.frombuffer(body, dtype="<i2")
    if a.size not in (H * W, 2 * H * W) or len(body) % 2:
        raise ValueError(f"payload of {len(body)} bytes is neither {2 * H * W} nor {4 * H * W} for {H} x {W}")
    elev = a[:H * W].reshape(H, W).astype(np.int16)
    biome = a[H * W:].reshape(H, W).astype(np.int16) if a.size == 2 * H * W else None
    return elev, biome
