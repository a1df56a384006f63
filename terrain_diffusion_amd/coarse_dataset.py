"""The data of the coarse model on the GPU: what the reference's CoarseDataset (terrain_diffusion/training/datasets/coarse_dataset.py) computes
when it builds its HDF5 file, and the crop score of its __getitem__.

  1. area_resize_width    a latitude band shrunk in width by cos(latitude): F.interpolate(mode='area') with the height unchanged (:277-281),
                          with the no-data rules (:305-309) or the signed square root (:266) applied as the values are read,
  2. tile_stats           26 x 26 tiles reduced to a mean, a 5 % quantile or a NaN-ignoring mean (:284-289, :325-327),
  3. fill_oceans          the oceans of the climate layers filled by a Laplace inpainting (:17-220): Jacobi-preconditioned CG from a
                          coarse-grid start, the whole of it on the device,
  4. crop_scores          the 0.9 quantile of a crop's squared 3 x 3 blur residual (:396-403),
  5. build_coarse_bands   :253-347 over arrays the caller has read: the nine bands, their means / stds / weights.

The per-element work runs in coarse_csrc/coarse_kernels.hip through libtd_coarse.so (include/td_coarse.h) on the engine's stream; there is no CPU
fallback.  The solver enqueues two plain launches per CG iteration; its iteration limit and stop flag live in device memory.

Stated, not reproduced:
  * Anchors (anchor_stride with anchor_strength > 0) raise NotImplementedError: CoarseDataset never passes them, and their coast mean wraps
    around the image through np.roll.
  * The iterates differ from scipy's in the last bits (another summation order of the dot products); tests/_coarse_twin.py states the bound the
    result is held to and the iteration counts are the reference's on every committed case.
  * Reading rasters and HDF5, the CoarseDataset class itself and its host RNG calls stay with the caller.  means / stds go through
    dataset.moments, which takes the bands as float32 and sums in float64.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import dataset as _dataset
from ._lib import Library
from ._plumbing import call, engine_for as _engine_for, f32 as _f32, shape as _shape

_P = C.c_void_p
_SIGS = {
    "td_coarse_last_error": (C.c_char_p, []),
    "td_coarse_area_resize_w": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "td_coarse_tile_stats": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P, _P, C.c_int]),
    "td_coarse_crop_scores": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, C.c_float, _P, C.c_int, C.c_int, _P, C.c_int]),
    "td_coarse_fill_oceans": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _P, _P, C.c_int]),
    "td_coarse_fill_oceans_chunked": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
}
EXPORTS = tuple(_SIGS)
_LIB = Library("libtd_coarse.so", _SIGS, "td_coarse_last_error", "td_coarse")
LIB_PATH, lib, check = _LIB.path, _LIB.lib, _LIB.check

MAX_WIDTH = 65536           # include/td_coarse.h TD_COARSE_MAX_WIDTH
MAX_TILE = 32               # TD_COARSE_MAX_TILE
MAX_SIDE = 8192             # TD_COARSE_MAX_SIDE
MAX_FACTOR = 32             # TD_COARSE_MAX_FACTOR
DEFAULT_CHUNK = 32          # TD_COARSE_DEFAULT_CHUNK
MAX_CROPS = 1 << 20
LOAD_RULES = {None: 0, "none": 0, "int16_nodata": 1, "float_nodata": 2, "signed_sqrt": 3}
TILE_PX = 26                # CoarseDataset's tile_px
ELEV_QUANTILE = 0.05        # :289
FILL_TOL = 1e-2             # :328
N_BANDS = 9                 # :269: np.linspace(0, rows, 10)
BAND_SLOTS = 50             # :254: band_widths = np.zeros((50,))


def _dp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _plane(x, what, limit):
    s = _shape(x) if hasattr(x, "shape") else np.shape(x)
    if len(s) != 2:
        raise ValueError(f"{what} must be (H, W), got {tuple(s)}")
    H, W = int(s[0]), int(s[1])
    if H < 1 or W < 1 or H > limit or W > limit:
        raise ValueError(f"{what} {H} x {W} outside the library's limit (1 <= H, W <= {limit})")
    return H, W


# ------------------------------------------------------------------------------------------------------------------------------ device forms
def _check_resize(x, w_out, load_rule):
    s = _shape(x) if hasattr(x, "shape") else np.shape(x)
    if len(s) != 2:
        raise ValueError(f"x must be (H, W), got {tuple(s)}")
    H, W = int(s[0]), int(s[1])
    w_out = int(w_out)
    if H < 1 or W < 1 or W > MAX_WIDTH or H * W >= 1 << 31:
        raise ValueError(f"x {H} x {W} outside the library's limit (H >= 1, 1 <= W <= {MAX_WIDTH}, H * W < 2^31)")
    if w_out < 1 or w_out > W:
        raise ValueError(f"w_out must be in 1 .. {W} (the resize only shrinks), got {w_out}")
    if load_rule not in LOAD_RULES and load_rule not in (0, 1, 2, 3):
        raise ValueError(f"load_rule must be one of {sorted(k for k in LOAD_RULES if k)} or 0 .. 3, got {load_rule!r}")
    return H, W, w_out, LOAD_RULES.get(load_rule, load_rule)


@torch.no_grad()
def area_resize_width(x, w_out, load_rule=None, *, engine=None):
    """x (H, W) -> fp32 (H, w_out) device tensor: F.interpolate(x[None, None], size=(H, w_out), mode='area'), the mean of the window
    [floor(j W / w_out), ceil((j + 1) W / w_out)) summed from the left in fp32; a NaN in a window gives NaN.  load_rule is applied to every value
    as it is read: "int16_nodata" (|x - 32768| < 1e-6 -> NaN), "float_nodata" (|x| > 1e6 -> NaN), "signed_sqrt" (sign(x) sqrt(|x|))."""
    H, W, w_out, rule = _check_resize(x, w_out, load_rule)
    engine, dev = _engine_for(x, engine)
    a = _f32(x, dev)
    out = torch.empty((H, w_out), dtype=torch.float32, device=dev)
    call(_LIB, "td_coarse_area_resize_w", engine, dev, _dp(a), H, W, w_out, rule, _dp(out), ordered=True)
    return out


def _check_tiles(x, t, q):
    H, W = _plane(x, "x", MAX_WIDTH)
    if H * W >= 1 << 31:
        raise ValueError(f"x {H} x {W} outside the library's limit (H * W < 2^31)")
    t = int(t)
    if t < 1 or t > min(MAX_TILE, H, W):
        raise ValueError(f"t must be in 1 .. min({MAX_TILE}, H, W), got {t} for {H} x {W}")
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"q must be in 0 .. 1, got {q!r}")
    return H, W, t, q


@torch.no_grad()
def tile_stats(x, t=TILE_PX, q=ELEV_QUANTILE, *, stats=("mean", "nanmean", "quantile"), engine=None):
    """x (Hs, Ws) -> {name: fp32 (Hs // t, Ws // t) device tensor} for the names in `stats`, over the whole t x t tiles (what is left over at
    the far edges belongs to none): `mean` (np.mean, NaN where the tile holds one), `nanmean` (np.nanmean, NaN for a tile without a value),
    `quantile` (np.quantile(q), NaN where the tile holds one).  Sums and the interpolation in float64, rounded once."""
    H, W, t, q = _check_tiles(x, t, q)
    stats = tuple(stats)
    if not stats or any(s not in ("mean", "nanmean", "quantile") for s in stats):
        raise ValueError(f"stats must name some of mean, nanmean, quantile, got {stats!r}")
    engine, dev = _engine_for(x, engine)
    a = _f32(x, dev)
    outs = {s: torch.empty((H // t, W // t), dtype=torch.float32, device=dev) for s in stats}
    call(_LIB, "td_coarse_tile_stats", engine, dev, _dp(a), H, W, t, q, _dp(outs.get("mean")), _dp(outs.get("nanmean")), _dp(outs.get("quantile")),
         ordered=True)
    return outs


def _check_crops(plane, offsets, c):
    H, W = _plane(plane, "plane", MAX_WIDTH)
    if H * W >= 1 << 31:
        raise ValueError(f"plane {H} x {W} outside the library's limit (H * W < 2^31)")
    c = int(c)
    if c < 3 or c > min(MAX_TILE, H, W):
        raise ValueError(f"c must be in 3 .. min({MAX_TILE}, H, W), got {c} for {H} x {W}")
    s = tuple(int(d) for d in np.shape(offsets))
    if len(s) != 2 or s[1] != 2 or s[0] < 1 or s[0] > MAX_CROPS:
        raise ValueError(f"offsets must be (N, 2) with 1 <= N <= 2^20, got {s}")
    if not torch.is_tensor(offsets) or not offsets.is_cuda:          # host offsets are checked here; device ones by the kernel (NaN for a crop outside)
        o = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets)
        if not np.issubdtype(o.dtype, np.integer):
            raise ValueError(f"offsets must be integers, got {o.dtype}")
        if (o < 0).any() or (o[:, 0] > H - c).any() or (o[:, 1] > W - c).any():
            raise ValueError(f"a {c} x {c} crop leaves the {H} x {W} plane")
    return H, W, c, s[0]


@torch.no_grad()
def crop_scores(plane, mean0, std0, offsets, c, *, engine=None):
    """The score CoarseDataset.__getitem__ ranks its candidate crops by (:396-403), for N crops at once: plane (H, W) is the normalised channel 0
    of a band, offsets (N, 2) the (i, j) of the c x c crops -> fp32 (N,) device tensor: with s = v * std0 + mean0 and e = sign(s) s^2 clamped at
    0, the 0.9 quantile (torch.quantile's arithmetic) of (e - avg_pool2d(e, 3, 1, 1))^2.  All in fp32."""
    H, W, c, N = _check_crops(plane, offsets, c)
    engine, dev = _engine_for(plane, engine)
    a = _f32(plane, dev)
    o = (offsets if torch.is_tensor(offsets) else torch.from_numpy(np.ascontiguousarray(offsets))).to(device=dev, dtype=torch.int32).contiguous()
    out = torch.empty(N, dtype=torch.float32, device=dev)
    call(_LIB, "td_coarse_crop_scores", engine, dev, _dp(a), H, W, C.c_float(float(mean0)), C.c_float(float(std0)), _dp(o), N, c, _dp(out), ordered=True)
    return out


def _check_fill(a, tol, maxiter, multires_factor, chunk):
    s = tuple(int(d) for d in np.shape(a))
    if len(s) != 2:
        raise ValueError("a must be a 2D array")                                  # the reference's own message
    H, W = _plane(a, "a", MAX_SIDE)
    f = int(multires_factor)
    if f < 1:
        raise ValueError("multires_factor must be >= 1")                           # the reference's own message
    if f > MAX_FACTOR:
        raise ValueError(f"multires_factor must be in 1 .. {MAX_FACTOR}, got {f}")
    tol = float(tol)
    if not tol >= 0.0:
        raise ValueError(f"tol must not be negative, got {tol!r}")
    if maxiter is not None and int(maxiter) < 1:
        raise ValueError(f"maxiter must be None or at least 1, got {maxiter}")
    maxiter = 0 if maxiter is None else int(maxiter)        # the C-ABI's 0: the default per level
    chunk = DEFAULT_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    return H, W, tol, maxiter, f, chunk


def _f64(x, dev):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float64))
    return x.detach().to(device=dev, dtype=torch.float64).contiguous()


@torch.no_grad()
def fill_oceans_device(a, *, tol=1e-6, maxiter=None, multires_factor=8, chunk=None, enqueue_only=False, return_info=False, engine=None):
    """a (H, W), NaN = ocean -> float64 (H, W) device tensor: the reference's fill_oceans without anchors.  Land keeps its bits; an input
    without NaN comes back unchanged.  maxiter=None is the reference's default per level, max(50, int(10 sqrt(unknowns))).  chunk: the CG
    iterations enqueued between two reads of the stop flag (result and counts do not depend on it); enqueue_only=True reads nothing back and
    enqueues up to the largest limit the shape allows.  return_info=True also returns the int32 (4,) device tensor: coarse iterations, coarse
    scipy info, fine iterations, fine info (0, or the limit when the limit ended the loop)."""
    H, W, tol, maxiter, f, chunk = _check_fill(a, tol, maxiter, multires_factor, chunk)
    engine, dev = _engine_for(a, engine)
    x = _f64(a, dev)
    out = torch.empty((H, W), dtype=torch.float64, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    call(_LIB, "td_coarse_fill_oceans_chunked", engine, dev, _dp(x), H, W, tol, maxiter, f, chunk, _dp(out), _dp(info), enqueue_only=enqueue_only,
         ordered=True)
    return (out, info) if return_info else out


# ------------------------------------------------------------------------------------------------------------------------------ drop-ins
def fill_oceans(a, *, tol=1e-6, maxiter=None, anchor_stride=None, anchor_strength=0.0, multires_factor=8):
    """Drop-in for coarse_dataset.py:17-220: a (H, W) array with the ocean as NaN -> float64 NumPy array.  anchor_stride=None or
    anchor_strength <= 0 is accepted (the reference ignores the anchors then); real anchors raise NotImplementedError."""
    if anchor_stride is not None and anchor_strength > 0.0:
        raise NotImplementedError("fill_oceans: anchors are not supported (CoarseDataset never passes them)")
    a = np.asarray(a)
    _check_fill(a, tol, maxiter, multires_factor, None)
    return fill_oceans_device(a.astype(np.float64), tol=tol, maxiter=maxiter, multires_factor=multires_factor).cpu().numpy()


def latitude_bands(height, top, bottom, n_bands=N_BANDS):
    """The row arithmetic of coarse_dataset.py:258-273 for a raster of `height` rows between latitudes `top` and `bottom` (degrees) ->
    (start_row, end_row, [(row_top, row_bottom, mid_latitude_deg)]): the rows of +60 .. -60 degrees, cut into n_bands bands by
    np.linspace(0, rows, n_bands + 1, dtype=int); row_top / row_bottom count from start_row."""
    height = int(height)
    top, bottom = float(top), float(bottom)
    if height < 1 or not top > bottom:
        raise ValueError(f"needs height >= 1 and top > bottom, got {height}, {top}, {bottom}")
    lat_res = (top - bottom) / height
    start_row = int((top - 60) / lat_res)
    end_row = int((top + 60) / lat_res)
    rows = len(range(height)[start_row:end_row])          # data = src.read(1)[start_row:end_row]
    if rows < n_bands:
        raise ValueError(f"{rows} rows between +60 and -60 degrees: fewer than {n_bands} bands")
    row_indices = np.linspace(0, rows, n_bands + 1, dtype=int)
    bands = [(int(a), int(b), top - (int(a) + int(b) + start_row * 2) / 2 * lat_res) for a, b in zip(row_indices[:-1], row_indices[1:])]
    return start_row, end_row, bands


def band_width(width, mid_latitude_deg):
    """:273-276: round(width / (1 / cos(latitude)))"""
    return round(int(width) / (1 / np.cos(np.deg2rad(mid_latitude_deg))))


def _check_build(etopo, layers, top, bottom, tile_px):
    H, W = _plane(etopo, "etopo", 1 << 30)
    layers = list(layers)
    if len(layers) != 4:
        raise ValueError(f"layers must be the four climate rasters (mean / std temperature, mean / std precipitation), got {len(layers)}")
    for k, l in enumerate(layers):
        if tuple(int(d) for d in np.shape(l)) != (H, W):
            raise ValueError(f"layer {k} is {tuple(np.shape(l))}, etopo is {(H, W)}: the rasters share one grid")
    tile_px = int(tile_px)
    if tile_px < 1 or tile_px > MAX_TILE:
        raise ValueError(f"tile_px must be in 1 .. {MAX_TILE}, got {tile_px}")
    if W > MAX_WIDTH:
        raise ValueError(f"rasters of {W} columns beyond the library's limit ({MAX_WIDTH})")
    start_row, end_row, bands = latitude_bands(H, top, bottom)
    plan = []
    for row_top, row_bottom, mid in bands:
        w = band_width(W, mid)
        if row_bottom - row_top < tile_px or w < tile_px:
            raise ValueError(f"band rows {row_top} .. {row_bottom} scaled to {w} columns hold no {tile_px} x {tile_px} tile")
        plan.append((start_row + row_top, start_row + row_bottom, w))
    return layers, tile_px, plan


@torch.no_grad()
def build_coarse_bands(etopo, layers, top, bottom, tile_px=TILE_PX, *, engine=None):
    """coarse_dataset.py:253-347 over arrays the caller has read: etopo (height, width) and the four climate layers on the same grid (an int16
    layer takes the int16 no-data rule, any other the float one), `top` / `bottom` the raster's latitude bounds.  Returns a mapping shaped like
    the reference's HDF5 file: gan_band_<i> float64 (6, h, w) NumPy arrays -- channel 0 the tile means of the signed square root of the
    elevation, 1 the means minus the 5 % quantile, 2 .. 5 the NaN-ignoring tile means of the layers with their oceans filled (tol 1e-2) --,
    `means` and `stds` (6,) float64 over all bands (dataset.moments, ddof 0) and `band_weights` float32 (50,), as the reference stores them."""
    layers, tile_px, plan = _check_build(etopo, layers, top, bottom, tile_px)
    engine, dev = _engine_for(etopo, engine)

    def rows(x, r0, r1):
        return x[r0:r1] if torch.is_tensor(x) else np.asarray(x)[r0:r1]
    out, widths, flat = {}, np.zeros((BAND_SLOTS,), dtype=int), []
    for i, (r0, r1, w) in enumerate(plan):
        scaled = area_resize_width(rows(etopo, r0, r1), w, "signed_sqrt", engine=engine)
        st = tile_stats(scaled, tile_px, ELEV_QUANTILE, stats=("mean", "quantile"), engine=engine)
        band = torch.zeros((6,) + tuple(st["mean"].shape), dtype=torch.float64, device=dev)
        band[0] = st["mean"].double()
        band[1] = (st["mean"] - st["quantile"]).double()
        for k, layer in enumerate(layers):
            rule = "int16_nodata" if (layer.dtype in (np.int16, torch.int16)) else "float_nodata"
            scaled = area_resize_width(rows(layer, r0, r1), w, rule, engine=engine)
            means = tile_stats(scaled, tile_px, stats=("nanmean",), engine=engine)["nanmean"]
            band[k + 2] = fill_oceans_device(means.double(), tol=FILL_TOL, engine=engine)
        out[f"gan_band_{i}"] = band.cpu().numpy()
        widths[i] = band.shape[1]                          # :296 stores lat_band.shape[1], the band's number of tile rows
        flat.append(band.reshape(6, 1, -1))
    count, mean, m2 = _dataset.moments(torch.cat(flat, dim=2), engine=engine)
    out["means"] = mean.cpu().numpy()
    out["stds"] = np.sqrt(m2.cpu().numpy() / np.float64(int(count.cpu())))
    out["band_weights"] = widths.astype(np.float32) / np.sum(widths).astype(np.float32)
    return out
