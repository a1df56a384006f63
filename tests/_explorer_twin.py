"""NumPy-only restatement of the explorer views (include/td_explorer.h): the arithmetic of the reference's explorer routes (inference/explorer/
server.py) and of its sampler's land-tile search (inference/random_sampler.py), written from the operator definitions -- NumPy's elementwise
fp32 arithmetic, matplotlib's Normalize and colormap lookup as formulas, plt.imsave's quantisation -- not from the product's code.  Colour
tables are parameters (the recorded ones of tests/golden/explorer.npz).  It gives expected values for inputs the fixture does not hold."""
import math
import random
from fractions import Fraction

import numpy as np

import _relief_twin

F = np.float32
CHANNEL_NAMES = ["Elev", "p5", "Temp", "T std", "Precip", "Precip CV"]
FILTERABLE = (0, 2, 3, 4, 5)


def channels(sums, n_signed_sq=2, eps=1e-8):
    """(C + 1, H, W) sums with the weight plane last -> (C, H, W) fp32 real-unit planes."""
    sums = np.asarray(sums, F)
    den = sums[-1:] + F(eps) if eps else sums[-1:]
    with np.errstate(all="ignore"):
        out = (sums[:-1] / den).astype(F)
        out[:n_signed_sq] = np.sign(out[:n_signed_sq]) * np.square(out[:n_signed_sq])
    return out


def nan_range(a):
    """(np.nanmin, np.nanmax) as Python floats; (nan, nan) for an all-NaN array."""
    a = np.asarray(a)
    ok = a[~np.isnan(a)]
    return (float(ok.min()), float(ok.max())) if ok.size else (float("nan"), float("nan"))


def display(field, log1p=False):
    field = np.asarray(field, F)
    with np.errstate(all="ignore"):
        return np.log1p(np.maximum(field, F(0))) if log1p else field


def view_range(d):
    """The routes' vmin, vmax of a displayed field: its NaN-ignoring range, vmax = vmin + 1 when equal."""
    vmin, vmax = nan_range(d)
    return (vmin, vmin + 1) if vmax == vmin else (vmin, vmax)


def normalize(d, vmin, vmax):
    """matplotlib.colors.Normalize(vmin, vmax) on an fp32 array: in-place fp32 array ops with float64 scalars."""
    with np.errstate(all="ignore"):
        t = (d.astype(np.float64) - vmin).astype(F)
        return (t.astype(np.float64) / (vmax - vmin)).astype(F)


def lookup(x, lut):
    """Colormap.__call__ on fp32 x with a (256, 3) table -> (rgba fp32 (H, W, 4), margin): margin is the distance of x * 256 from the nearest
    boundary between two table entries (the integers 1..255: below 1 and above 255 the index is clamped) in fp32 ulps of x * 256; inf
    where x is NaN (the pixel is transparent whatever the index)."""
    lut = np.asarray(lut, F)
    with np.errstate(all="ignore"):
        xa = x * F(256)
        bad = np.isnan(xa)
        raw = np.where(bad, F(1), xa)
        xa = np.where(xa == 256, F(255), xa)
        idx = np.where(xa < 0, 0, np.where(xa >= 256, 255, np.where(bad, 0, xa).astype(np.int64))).astype(np.int64)
        idx = np.clip(idx, 0, 255)
        nearest = np.clip(np.round(raw.astype(np.float64)), 1, 255)
        margin = np.abs(raw.astype(np.float64) - nearest) / np.spacing(np.maximum(np.abs(raw), F(1)).astype(F)).astype(np.float64)
    rgba = np.concatenate([lut[idx], np.ones(idx.shape + (1,), F)], axis=-1)
    rgba[bad] = 0
    margin = np.where(bad, np.inf, margin)
    return rgba, margin


def quantize(rgba):
    """plt.imsave of np.clip(rgba, 0, 1): (c * 255) in fp32, truncated to uint8; a NaN channel is written as 0 (the library's convention)."""
    with np.errstate(all="ignore"):
        c = np.clip(np.asarray(rgba, F), 0, 1) * F(255)
        return np.where(np.isnan(c), 0, c).astype(np.uint8)


def passes(plane, lo, hi):
    """The route's filter of one plane: plane >= lo and plane <= hi with the Python-float bounds brought to the plane's fp32 (a NaN fails)."""
    plane = np.asarray(plane, F)
    mask = np.ones(plane.shape, bool)
    with np.errstate(invalid="ignore"):
        if lo is not None:
            mask &= plane >= F(lo)
        if hi is not None:
            mask &= plane <= F(hi)
    return mask


def colorize(field, lut, log1p=False, vmin=None, vmax=None, filters=()):
    """-> (rgba8 (H, W, 4), vmin, vmax, margin).  filters: (plane, lo or None, hi or None)."""
    d = display(field, log1p)
    if vmin is None:
        vmin, vmax = view_range(d)
    rgba, margin = lookup(normalize(d, vmin, vmax), lut)
    if filters:
        mask = np.ones(d.shape, bool)
        for plane, lo, hi in filters:
            mask &= passes(plane, lo, hi)
        rgba[~mask, :3] *= F(0.3)
    return quantize(rgba), vmin, vmax, margin


def coarse_image(coarse, channel, lut, filters=None):
    """/api/coarse.png from the (7, H, W) block the route read -> (rgba8, headers, margin)."""
    planes = channels(coarse)
    fl = []
    for ch in FILTERABLE:
        lo, hi = (filters or {}).get(ch, (None, None))
        if lo is not None or hi is not None:
            fl.append((planes[ch], lo, hi))
    img, vmin, vmax, margin = colorize(planes[channel], lut, log1p=channel == 4, filters=fl)
    return img, {"X-Vmin": str(round(vmin, 3)), "X-Vmax": str(round(vmax, 3))}, margin


def coarse_stats(coarse):
    planes = channels(coarse)
    return {ch: {"name": CHANNEL_NAMES[ch], "min": round(nan_range(planes[ch])[0], 3), "max": round(nan_range(planes[ch])[1], 3)}
            for ch in range(len(CHANNEL_NAMES))}


def coarse_data(coarse, box):
    planes = channels(coarse)
    ci0, ci1, cj0, cj1 = box
    return {"ci0": ci0, "ci1": ci1, "cj0": cj0, "cj1": cj1, "channels": {n: np.round(planes[i], 2).tolist() for i, n in enumerate(CHANNEL_NAMES)}}


def relief_rgba8(rgb):
    rgb = np.asarray(rgb, F)
    return quantize(np.concatenate([rgb, np.ones(rgb.shape[:2] + (1,), F)], axis=-1))


def detail_image(elev, climate, mode, luts, resolution=90.0):
    """/api/detail.png from the world.get window -> (rgba8, kind, margin or None); kind is the branch taken: elevation, temperature, relief."""
    if mode == "elevation":
        img, _, _, margin = colorize(elev, luts["terrain"])
        return img, "elevation", margin
    if mode == "temperature" and climate is not None:
        img, _, _, margin = colorize(climate[0], luts["RdBu_r"])
        return img, "temperature", margin
    return relief_rgba8(_relief_twin.relief(np.asarray(elev, F), resolution=resolution)), "relief", None


def raw_tile(elev, temp=None):
    """/api/detail_raw's body; NaN elevation -> 0."""
    with np.errstate(invalid="ignore"):
        e = np.clip(np.floor(np.asarray(elev, F)), -32768, 32767)
    body = np.where(np.isnan(e), 0, e).astype("<i2").tobytes()
    return body + (np.asarray(temp).astype("<f4").tobytes() if temp is not None else b"")


def land_tiles(elev_m, half, min_land_frac, exact=False):
    """Flat indices i * W + j, ascending, of the valid positions.  exact=True compares the exact fraction c / (4 half^2) instead of torch's
    fp32 mean: NOT the reference's semantics (kept to show that the two differ)."""
    land = (np.asarray(elev_m, F) > 0).astype(np.int64)
    H, W = land.shape
    if half == 0:
        return np.zeros(0, np.int64)
    s = np.zeros((H + 1, W + 1), np.int64)
    s[1:, 1:] = land.cumsum(0).cumsum(1)
    i = np.arange(half, H - half)[:, None]
    j = np.arange(half, W - half)[None, :]
    c = s[i + half, j + half] - s[i - half, j + half] - s[i + half, j - half] + s[i - half, j - half]
    cells = 4 * half * half
    if exact:
        valid = c >= math.ceil(Fraction(min_land_frac) * cells)
    else:
        valid = (c.astype(F) / F(cells)).astype(np.float64) >= min_land_frac
    return (i * W + j)[valid].astype(np.int64)


def block_offsets(counts, round_size=1024):
    """Exclusive prefix sums of the per-block counts and their total, taken as the device takes them: in rounds of `round_size` blocks with
    the sum of all earlier rounds carried into the next."""
    counts = np.asarray(counts, np.int64)
    out, carry = np.zeros(counts.size, np.int64), 0
    for base in range(0, counts.size, round_size):
        part = counts[base:base + round_size]
        out[base:base + round_size] = carry + np.cumsum(part) - part
        carry += int(part.sum())
    return out, carry


def compact(valid, offsets=block_offsets, block=256):
    """The ordered compaction of an (H, W) validity mask as the device states it: blocks of `block` consecutive flat indices, their counts,
    `offsets(counts)`, and each block's valid indices written from its offset on -> (idx, count).  Equal to np.flatnonzero(valid) when
    `offsets` is right; slots nobody wrote hold -1."""
    flat = np.asarray(valid, bool).ravel()
    nb = -(-flat.size // block)
    padded = np.zeros(nb * block, bool)
    padded[:flat.size] = flat
    counts = padded.reshape(nb, block).sum(1)
    off, total = offsets(counts)
    idx = np.full(int(counts.sum()), -1, np.int64)
    where = np.flatnonzero(padded)
    rank = np.arange(where.size) - np.repeat(np.cumsum(counts) - counts, counts)        # position within its block
    at = np.repeat(off, counts) + rank
    ok = at < idx.size
    idx[at[ok]] = where[ok]
    return idx, int(total)


def sample_land_tiles(coarse, coarse_window, detail_size, min_land_frac=0.5, n_samples=10):
    """random_sampler.sample_land_tiles from the (7, 2 w, 2 w) block it read (normalize_tensor: no epsilon); uses the global `random`."""
    elev_m = channels(coarse, eps=0.0)[0]
    W = elev_m.shape[1]
    flat = land_tiles(elev_m, (detail_size // 256) // 2, min_land_frac)
    tiles = [(-coarse_window + int(p) // W, -coarse_window + int(p) % W) for p in flat]
    return tiles if len(tiles) < n_samples else random.sample(tiles, n_samples)


def climate_info(coarse11):
    p = channels(coarse11, n_signed_sq=0, eps=0.0)
    return {"temp": float(p[2, 0, 0]), "temp_std": float(p[3, 0, 0]), "precip": float(p[4, 0, 0]), "precip_cv": float(p[5, 0, 0])}


def decode_png(data):
    """Pixels (H, W, 4) uint8 of an 8-bit RGBA, non-interlaced PNG, from zlib alone (all five row filters)."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, W = 8, b"", None
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert zlib.crc32(kind + body) & 0xFFFFFFFF == struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0]
        if kind == b"IHDR":
            W, H, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body)
            assert (depth, ctype, interlace) == (8, 6, 0)
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 4 * W)
    out = np.zeros((H, 4 * W), np.int64)
    for y in range(H):
        ft, line = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(4 * W, np.int64)
        if ft == 0:
            out[y] = line
        elif ft == 2:
            out[y] = (line + up) & 255
        else:
            for x in range(4 * W):
                a = out[y, x - 4] if x >= 4 else 0
                b, c = up[x], (up[x - 4] if x >= 4 else 0)
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                out[y, x] = (line[x] + pred) & 255
    return out.astype(np.uint8).reshape(H, W, 4)
