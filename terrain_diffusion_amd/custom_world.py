"""Import a custom map and export the generated elevation: the reference's azgaar-to-tiff (inference/utils/azgaar_to_tiff.py) and tiff-export
(inference/tiff_export.py) workflow, array in / array out.

  1. azgaar_layers        a full Azgaar JSON export -> the five conditioning layers (rasterize_layer + fill_nodata per layer),
  2. import_conditioning  pads and installs them (WorldPipeline.set_custom_conditioning_import, origin (0, 0), 64 cells of edge padding),
  3. export_elevation     reads the generated elevation back chunk by chunk as the export's int16.

The per-pixel work -- the cell rasteriser, the nearest-valid fill, the clip-and-truncate to int16 -- runs in custom_csrc/custom_kernels.hip
through libtd_custom.so (include/td_custom.h) on the engine's stream; there is no CPU fallback.  The Azgaar JSON, the padding and the chunk
loop are host code.  GeoTIFF reading and writing is not part of the package (rasterio is not a dependency): layers travel as arrays;
INTEGRATION.md shows where rasterio's read and write plug in.

Stated, not reproduced:
  * The pixel-CENTRE rule of rasterize_cells is this project's statement of GDAL's all_touched=False.  It was not compared with GDAL; a
    difference is possible only for a pixel centre that lies on an edge to within rounding.
  * A layer without one valid pixel is REFUSED (fill_nearest and fill_nodata raise ValueError) rather than reproduced: the reference's
    result for it is meaningless.
  * A NaN pixel is always invalid for the fill, also under a sentinel nodata (the reference then treats NaN as a value).
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from ._lib import Library
from ._plumbing import call, engine_for as _engine_for, f32 as _f32, shape as _shape

_P = C.c_void_p
_SIGS = {
    "td_custom_last_error": (C.c_char_p, []),
    "td_custom_rasterize": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int, C.c_int, C.c_int, C.c_double, _P, C.c_int]),
    "td_custom_fill_nearest": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, _P, _P, _P, C.c_int]),
    "td_custom_elev_int16": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int]),
}
EXPORTS = tuple(_SIGS)
_LIB = Library("libtd_custom.so", _SIGS, "td_custom_last_error", "td_custom")
LIB_PATH, lib, check = _LIB.path, _LIB.lib, _LIB.check

MAX_SIDE = 16384            # include/td_custom.h TD_CUSTOM_MAX_SIDE: 1 <= H, W <= 16384
MAX_ELEMENTS = 1 << 30      # TD_CUSTOM_MAX_ELEMENTS, per call of td_custom_elev_int16
PADDING = 64                # tiff_export.py: cells of edge padding around an imported layer
PIXELS_PER_CELL = 256       # output pixels per conditioning cell

# tiff_export.py CHANNEL_FILES by file stem: (conditioning channel, multiplier to the pipeline's internal units, default value outside the import)
CHANNELS = {"heightmap": (0, 1.0, -1000.0), "temperature": (1, 1.0, None), "temperature_std": (2, 100.0, None),
            "precipitation": (3, 1.0, None), "precipitation_cv": (4, 1.0, None)}
LAYERS = tuple(CHANNELS)

# azgaar_to_tiff.py: Azgaar biome id -> (temperature std in degrees C, precipitation coefficient of variation in %); marine has none
BIOME_VARIABILITY = (
    (float("nan"), float("nan")),  # 0 marine
    (5.0, 80.0),                   # 1 hot desert
    (15.0, 33.0),                  # 2 cold desert
    (5.0, 28.6),                   # 3 savanna
    (10.0, 25.0),                  # 4 grassland
    (3.0, 26.7),                   # 5 tropical seasonal forest
    (8.0, 22.2),                   # 6 temperate deciduous forest
    (2.0, 16.0),                   # 7 tropical rainforest
    (6.0, 25.0),                   # 8 temperate rainforest
    (15.0, 20.0),                  # 9 taiga
    (15.0, 25.0),                  # 10 tundra
    (10.0, 30.0),                  # 11 glacier
    (8.0, 20.0),                   # 12 wetland
)
KM_PER_DEGREE = 111.32


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _hw(H, W, noun):
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{noun} {H} x {W} outside the library's limit (1 <= H, W <= {MAX_SIDE})")
    return H, W


def _plane(x, what):
    if len(_shape(x)) != 2:
        raise ValueError(f"{what} must be (H, W), got {_shape(x)}")
    return _hw(*_shape(x), what)


def _dev(x, dtype, dev):
    """Contiguous device tensor of `dtype` of a numpy array, sequence or tensor."""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=dtype))
    return x.detach().to(device=dev, dtype=getattr(torch, np.dtype(dtype).name)).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------ device forms
def _check_cells(xy, offsets, values, shape):
    if len(tuple(shape)) != 2:
        raise ValueError(f"shape must be (H, W), got {tuple(shape)}")
    H, W = _hw(*shape, "raster")
    sxy, so, sv = np.shape(xy), np.shape(offsets), np.shape(values)
    n_xy = int(np.prod(sxy)) // 2
    if not ((len(sxy) == 2 and sxy[1] == 2) or n_xy == 0):
        raise ValueError(f"xy must be (n_vertices, 2) pixel coordinates, got {tuple(sxy)}")
    if len(so) != 1 or so[0] < 1:
        raise ValueError(f"offsets must be (n + 1,), got {tuple(so)}")
    n = so[0] - 1
    if len(sv) != 1 or sv[0] != n:
        raise ValueError(f"values must be (n,) = ({n},), got {tuple(sv)}")
    if n_xy >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 vertices (int32 offsets)")
    if not torch.is_tensor(offsets) and n > 0:
        o = np.asarray(offsets, dtype=np.int64)
        if o[0] < 0 or o[-1] > n_xy or np.any(np.diff(o) < 0):
            raise ValueError(f"offsets must ascend within [0, {n_xy}]")
    return H, W, n, n_xy


@torch.no_grad()
def rasterize_cells(xy, offsets, values, shape, fill, *, engine=None):
    """n polygons in CSR form -> fp32 (H, W) device tensor: polygon p is the implicitly closed ring xy[offsets[p]:offsets[p + 1]] ((x, y) in
    pixel units, float64) and burns values[p] into every pixel whose centre (c + 0.5, r + 0.5) it holds by the crossing-number test in
    float64 (include/td_custom.h); the later polygon wins an overlap, rings of fewer than 3 vertices burn nothing, pixels no polygon
    covers get `fill`.  rasterize_layer's arithmetic with all_touched=False, under the centre rule this module's docstring states."""
    H, W, n, n_xy = _check_cells(xy, offsets, values, shape)
    engine, dev = _engine_for(xy if torch.is_tensor(xy) else None, engine)
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    dxy = _dev(xy, np.float64, dev) if n_xy else None
    doff, dval = (_dev(offsets, np.int32, dev), _f32(values, dev)) if n else (None, None)
    call(_LIB, "td_custom_rasterize", engine, dev, _dp(dxy), n_xy, _dp(doff), _dp(dval), n, H, W, float(fill), _dp(out), ordered=True)
    return out


def _fill(engine, dev, arr, nodata, return_index, enqueue_only=False):
    H, W = _plane(arr, "arr")
    a = _f32(arr, dev)
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    index = torch.empty((H, W), dtype=torch.int32, device=dev) if return_index else None
    valid = torch.empty(1, dtype=torch.int32, device=dev)
    call(_LIB, "td_custom_fill_nearest", engine, dev, _dp(a), H, W, float(nodata), _dp(out), _dp(index), _dp(valid),
         enqueue_only=enqueue_only, ordered=True)
    return out, index, valid


@torch.no_grad()
def fill_nearest(arr, nodata=float("nan"), *, return_index=False, engine=None):
    """arr (H, W) -> fp32 device tensor in which every invalid pixel (NaN, or equal to `nodata`) holds the value of the nearest valid pixel in
    exact Euclidean distance; valid pixels keep their bits.  Ties go to the smallest column, then the smallest row (scipy's
    distance_transform_edt indices, which the reference's fill_nodata uses).  return_index=True also returns the int32 (H, W) flat index
    r * W + c each pixel was taken from.  Raises ValueError when no pixel is valid (a stated deviation: the reference's result is
    meaningless then); that check is the call's one 4-byte read-back."""
    _plane(arr, "arr")
    engine, dev = _engine_for(arr, engine)
    out, index, valid = _fill(engine, dev, arr, nodata, return_index)
    if int(valid) == 0:
        raise ValueError("fill_nearest: the layer holds no valid pixel")
    return (out, index) if return_index else out


@torch.no_grad()
def elevation_int16(elev, *, engine=None):
    """elev (any shape) -> int16 device tensor of that shape: np.clip(elev, -32768, 32767).astype(np.int16) of the export -- clip, then
    truncate toward zero (explorer.raw_tile floors) -- with NaN written as 0."""
    n = int(np.prod(_shape(elev)))
    if n > MAX_ELEMENTS:
        raise ValueError(f"{n} elements beyond the library's limit of 2^30 per call")
    engine, dev = _engine_for(elev, engine)
    e = _f32(elev, dev)
    out = torch.empty(_shape(elev), dtype=torch.int16, device=dev)
    call(_LIB, "td_custom_elev_int16", engine, dev, _dp(e), n, _dp(out), ordered=True)
    return out


# ------------------------------------------------------------------------------------------------------------------------------ azgaar_to_tiff
def h_to_meters(h, exponent, ocean_max_depth=4000.0, ocean_power=1.5):
    """Azgaar's internal height (0-100) in metres, host float64.  From h = 20 up it is land, Azgaar's own getHeight: the height above 18
    raised to `exponent`.  Below 20 it is ocean: the share of the way down from 20 to 0, raised to ocean_power, of ocean_max_depth."""
    sea_level, land_base = 20, 18
    if h >= sea_level:
        return float(h - land_base) ** exponent
    share = (sea_level - h) / sea_level
    return -(ocean_max_depth * share ** ocean_power)


def fill_nodata(arr, nodata):
    """Drop-in for the reference's fill_nodata: numpy (H, W) in, numpy float32 out, nodata pixels replaced by the nearest valid pixel's value
    (fill_nearest); the input itself when nothing is invalid.  Raises ValueError when everything is."""
    a = np.asarray(arr)
    if a.ndim != 2:
        raise ValueError(f"arr must be (H, W), got {a.shape}")
    nodata = float(nodata)
    mask = np.isnan(a) if np.isnan(nodata) else (np.isnan(a) | (a == np.float32(nodata)))
    if not mask.any():
        return arr
    return fill_nearest(a, nodata).cpu().numpy()


def _float32_only(dtype):
    try:
        ok = np.dtype(dtype) == np.float32
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"rasterize_layer: only dtype 'float32' is supported, got {dtype!r}")


def _no_value(value):
    return value is None or (type(value) is float and value != value)


def cells_csr(cells, verts, scale_x, scale_y, value_fn):
    """(xy (nv, 2) float64, offsets (n + 1,) int32, values (n,) float32): one ring per cell, its vertices verts[vi] scaled to pixels, in
    list order.  Left out, as the reference leaves them out: a cell without a value (None, or a float NaN) and a cell that names a vertex
    `verts` does not hold."""
    kept = [(cell["v"], value) for cell, value in ((cell, value_fn(cell)) for cell in cells)
            if not _no_value(value) and all(vi in verts for vi in cell["v"])]
    offsets = np.zeros(len(kept) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(ring) for ring, _ in kept], dtype=np.int64)
    xy = np.array([verts[vi] for ring, _ in kept for vi in ring], dtype=np.float64).reshape(-1, 2) * np.array([scale_x, scale_y], dtype=np.float64)
    return xy, offsets, np.array([value for _, value in kept], dtype=np.float32)


def rasterize_layer(cells, verts, scale_x, scale_y, shape, value_fn, dtype, fill, *, engine=None):
    """Drop-in for the reference's rasterize_layer (same arguments): burns value_fn(cell) into the pixels of every cell's polygon -> numpy
    float32 (H, W).  Only dtype "float32" is accepted (the only one the reference passes)."""
    _float32_only(dtype)
    if len(tuple(shape)) != 2:
        raise ValueError(f"shape must be (H, W), got {tuple(shape)}")
    _hw(*shape, "raster")
    xy, offsets, values = cells_csr(cells, verts, scale_x, scale_y, value_fn)
    return rasterize_cells(xy, offsets, values, shape, fill, engine=engine).cpu().numpy()


def _pixels(extent_km, scale):
    """Pixels of `scale` km along an extent, at least one; Python's round (half to even)."""
    return max(1, round(extent_km / scale))


def output_geometry(coords, map_w, map_h, scale=100.0):
    """The reference's output grid for an Azgaar map: {"out_h", "out_w", "scale_x", "scale_y", "lon_w", "lon_e", "lat_s", "lat_n",
    "pixel_lon", "pixel_lat"}.  Pixels of `scale` km: 111.32 km per degree of latitude, times cos(middle latitude) per degree of longitude;
    max(1, round(...)) with Python's round (half to even)."""
    west, east, south, north = (coords[k] for k in ("lonW", "lonE", "latS", "latN"))
    km_per_degree_east = KM_PER_DEGREE * np.cos(np.radians((north + south) / 2))
    out_h, out_w = int(_pixels((north - south) * KM_PER_DEGREE, scale)), int(_pixels((east - west) * km_per_degree_east, scale))
    return {"out_h": out_h, "out_w": out_w, "scale_x": out_w / map_w, "scale_y": out_h / map_h, "lon_w": west, "lon_e": east,
            "lat_s": south, "lat_n": north, "pixel_lon": (east - west) / out_w, "pixel_lat": (north - south) / out_h}


def _cell_number(key, factor=1.0):
    """value_fn of a grid cell's own number: float(cell[key]) * factor, no value when the cell lacks the key."""
    return lambda cell: None if key not in cell else float(cell[key]) * factor


def _biome_value(column):
    def fn(cell):
        b = cell.get("biome", 0)
        return BIOME_VARIABILITY[int(b)][column] if b in range(len(BIOME_VARIABILITY)) else float("nan")
    return fn


def azgaar_layers(map_or_path, scale=100.0, ocean_max_depth=4000.0, ocean_power=1.5, *, engine=None):
    """A full Azgaar JSON export (the parsed dict, or a path to the file) -> (layers, geo): the five float32 (out_h, out_w) arrays the
    reference writes as heightmap / temperature / temperature_std / precipitation / precipitation_cv .tif, and output_geometry's dict.
    Grid cells give the height in metres (h 0 when a cell has none), the temperature and the precipitation x 100; pack cells give the two
    biome-derived layers (biome 0 when a cell has none).  Each layer is rasterised over its fill (NaN for the height, -9999 for the rest)
    and then filled from the nearest valid pixel."""
    if isinstance(map_or_path, (str, os.PathLike)):
        with open(map_or_path) as f:
            data = json.load(f)
    else:
        data = map_or_path
    exponent = float(data["settings"]["heightExponent"])
    geo = output_geometry(data["mapCoordinates"], data["info"]["width"], data["info"]["height"], scale)
    shape = _hw(geo["out_h"], geo["out_w"], "raster")
    height = lambda cell: h_to_meters(cell.get("h", 0), exponent, ocean_max_depth, ocean_power)
    # layer -> (which cells, value of a cell, fill and nodata)
    spec = {"heightmap": ("grid", height, float("nan")), "temperature": ("grid", _cell_number("temp"), -9999.0),
            "temperature_std": ("pack", _biome_value(0), -9999.0), "precipitation": ("grid", _cell_number("prec", 100.0), -9999.0),
            "precipitation_cv": ("pack", _biome_value(1), -9999.0)}
    verts = {kind: {v["i"]: v["p"] for v in data[kind]["vertices"]} for kind in ("grid", "pack")}
    layers = {}
    for name in LAYERS:
        kind, value_fn, fill = spec[name]
        xy, offsets, values = cells_csr(data[kind]["cells"], verts[kind], geo["scale_x"], geo["scale_y"], value_fn)
        raster = rasterize_cells(xy, offsets, values, shape, fill, engine=engine)
        layers[name] = fill_nearest(raster, fill, engine=engine).cpu().numpy()
    return layers, geo


# ------------------------------------------------------------------------------------------------------------------------------ tiff_export
def load_and_pad(arr, nodata, internal_scale, default_value, padding=PADDING):
    """What the reference's _load_and_pad makes of a layer once it is read (host): float32; every pixel that equals nodata (when given) or
    is not finite becomes default_value, 0 without one; the layer times internal_scale in float32; `padding` cells on every side that
    repeat the nearest edge pixel."""
    layer = np.array(arr, dtype=np.float32)
    if layer.ndim != 2:
        raise ValueError(f"a layer must be (H, W), got {layer.shape}")
    unusable = ~np.isfinite(layer)
    if nodata is not None:
        unusable |= layer == nodata
    layer[unusable] = np.float32(0.0 if default_value is None else default_value)
    layer *= np.float32(internal_scale)
    return np.pad(layer, int(padding), mode="edge")


def import_conditioning(world, layers, nodata=None):
    """Install every layer of `layers` ({stem: (H, W) array}, stems of LAYERS; e.g. azgaar_layers' dict or an opened .npz) as custom
    conditioning of `world`, as tiff-export does with a folder of TIFFs: load_and_pad with the channel's internal scale and default value,
    then set_custom_conditioning_import(channel, padded, 0, 0, default_value).  `nodata` is one value for all layers or {stem: value}.  A
    stem that is absent is skipped (the synthetic conditioning stays for that channel).  Returns (H_cells, W_cells) of the first layer
    present, the size export_elevation takes; raises ValueError when none is, or when the layers differ in shape."""
    present = [name for name in LAYERS if name in layers]
    if not present:
        raise ValueError(f"import_conditioning: no layer given (expected any of {', '.join(LAYERS)})")
    shapes = {name: tuple(np.shape(layers[name])) for name in present}
    for name, s in shapes.items():
        if len(s) != 2:
            raise ValueError(f"layer {name} must be (H, W), got {s}")
        if s != shapes[present[0]]:
            raise ValueError(f"layer {name} is {s}, layer {present[0]} is {shapes[present[0]]}: the layers of one map have one shape")
    for name in present:
        channel, internal_scale, default_value = CHANNELS[name]
        nd = nodata.get(name) if isinstance(nodata, dict) else nodata
        world.set_custom_conditioning_import(channel, load_and_pad(layers[name], nd, internal_scale, default_value), 0, 0, default_value=default_value)
    return shapes[present[0]]


def export_boxes(H_cells, W_cells, chunk_size=8 * PIXELS_PER_CELL):
    """[(row, col, (i1, j1, i2, j2))]: the export's chunks in its order (row-major) -- the output offset in pixels and the world.get box,
    which lies PADDING cells in (the import is anchored at (0, 0) with its padding)."""
    H_cells, W_cells, chunk_size = int(H_cells), int(W_cells), int(chunk_size)
    if chunk_size <= 0 or chunk_size % PIXELS_PER_CELL != 0:
        raise ValueError(f"chunk_size must be a positive multiple of {PIXELS_PER_CELL}, got {chunk_size}")
    if H_cells < 1 or W_cells < 1:
        raise ValueError(f"empty map: {H_cells} x {W_cells} cells")
    extent, shift = PIXELS_PER_CELL, PADDING * PIXELS_PER_CELL

    def spans(n_cells):
        return [(a, min(a + chunk_size, n_cells * extent)) for a in range(0, n_cells * extent, chunk_size)]
    return [(r0, c0, (r0 + shift, c0 + shift, r1 + shift, c1 + shift)) for r0, r1 in spans(H_cells) for c0, c1 in spans(W_cells)]


@torch.no_grad()
def export_elevation(world, H_cells, W_cells, chunk_size=8 * PIXELS_PER_CELL, *, engine=None):
    """The elevation tiff-export writes, as a numpy int16 (H_cells * 256, W_cells * 256) array: world.get(..., with_climate=False) over the
    reference's chunks (chunk_size output pixels a side, a multiple of 256), each converted on the device (elevation_int16) and copied to the
    host once.  `world` is bound and stays open."""
    boxes = export_boxes(H_cells, W_cells, chunk_size)
    out = np.empty((int(H_cells) * PIXELS_PER_CELL, int(W_cells) * PIXELS_PER_CELL), dtype=np.int16)
    for row, col, box in boxes:
        q = elevation_int16(world.get(*box, with_climate=False)["elev"], engine=engine).cpu().numpy()
        out[row:row + q.shape[0], col:col + q.shape[1]] = q
    return out
