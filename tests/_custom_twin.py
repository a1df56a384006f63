"""NumPy twin of the custom-map import library (include/td_custom.h, terrain_diffusion_amd/custom_world.py): the rasteriser's crossing-number
rule in float64, the nearest-valid fill as a brute-force minimum with the (column, row) tie rule, the export's clip-and-truncate,
tiff_export's _load_and_pad on an array, the layers of a whole Azgaar map, and a synthetic Azgaar map built from a Voronoi diagram.
Restated from the header's rules, not from the kernels; keep the two in step."""
import numpy as np

F = np.float32
LAYERS = ("heightmap", "temperature", "temperature_std", "precipitation", "precipitation_cv")
PADDING, PIXELS_PER_CELL = 64, 256
TAME = 1.0e9


# ---------------------------------------------------------------------------------------------------------------------------------- rasteriser
def inside(ring, px, py):
    """Crossing-number test of the points (px, py) (float64 arrays of one shape) against the implicitly closed ring (nv, 2) float64: an edge
    (x0, y0) -> (x1, y1) counts when (y0 > py) != (y1 > py) and px < x0 + (py - y0) * (x1 - x0) / (y1 - y0), evaluated in that order."""
    x0, y0 = ring[:, 0].reshape(-1, *([1] * px.ndim)), ring[:, 1].reshape(-1, *([1] * px.ndim))
    x1, y1 = np.roll(x0, -1, axis=0), np.roll(y0, -1, axis=0)
    with np.errstate(all="ignore"):
        straddle = (y0 > py) != (y1 > py)
        xi = x0 + (py - y0) * (x1 - x0) / (y1 - y0)
        return (np.count_nonzero(straddle & (px < xi), axis=0) & 1).astype(bool)


def owners(xy, offsets, shape):
    """(H, W) int32: the index of the LAST polygon of the CSR list whose ring holds the pixel's centre (c + 0.5, r + 0.5), -1 where none does.
    A ring with fewer than 3 vertices, or with offsets outside xy, holds nothing.  Only the pixels near a ring's bounding box are tested (two
    pixels of margin; the whole raster for a ring with a coordinate beyond 1e9 or not finite): a centre outside the box is outside the ring."""
    H, W = shape
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    offsets = np.asarray(offsets, np.int64)
    own = np.full((H, W), -1, np.int32)
    for p in range(len(offsets) - 1):
        o0, o1 = int(offsets[p]), int(offsets[p + 1])
        if o0 < 0 or o1 > len(xy) or o1 - o0 < 3:
            continue
        ring = xy[o0:o1]
        r0, r1, c0, c1 = 0, H - 1, 0, W - 1
        if np.all(np.abs(ring) <= TAME):
            r0, r1 = max(0, int(np.floor(ring[:, 1].min())) - 2), min(H - 1, int(np.floor(ring[:, 1].max())) + 2)
            c0, c1 = max(0, int(np.floor(ring[:, 0].min())) - 2), min(W - 1, int(np.floor(ring[:, 0].max())) + 2)
            if r0 > r1 or c0 > c1:
                continue
        py, px = np.meshgrid(np.arange(r0, r1 + 1) + 0.5, np.arange(c0, c1 + 1) + 0.5, indexing="ij")
        box = own[r0:r1 + 1, c0:c1 + 1]
        box[inside(ring, px, py)] = p
    return own


def rasterize(xy, offsets, values, shape, fill):
    """(H, W) float32: values[owner] where a polygon holds the pixel's centre (the later polygon wins), else fill."""
    own = owners(xy, offsets, shape)
    values = np.asarray(values, F)
    out = np.full(shape, fill, F)
    out[own >= 0] = values[own[own >= 0]]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------- nearest fill
def invalid_mask(arr, nodata):
    """NaN, or equal to the sentinel (compared in float32); a NaN sentinel means NaN only."""
    arr = np.asarray(arr, F)
    nodata = float(nodata)
    return np.isnan(arr) if np.isnan(nodata) else (np.isnan(arr) | (arr == F(nodata)))


def fill_sources(arr, nodata=np.nan):
    """(H, W) int64 flat index of the pixel each pixel is taken from: its own when valid (or when nothing is valid), else the valid pixel at
    the smallest squared Euclidean distance (exact, in integers) -- on a tie the smallest column, and within that column the smallest row."""
    arr = np.asarray(arr, F)
    H, W = arr.shape
    bad = invalid_mask(arr, nodata)
    src = np.arange(H * W, dtype=np.int64).reshape(H, W)
    vr, vc = np.nonzero(~bad)
    if len(vr) == 0 or not bad.any():
        return src
    order = np.lexsort((vr, vc))            # column first, then row: argmin's first hit is the tie rule
    vr, vc = vr[order].astype(np.int64), vc[order].astype(np.int64)
    hr, hc = np.nonzero(bad)
    for a in range(0, len(hr), 2048):       # blocks of holes against every valid pixel
        r, c = hr[a:a + 2048, None], hc[a:a + 2048, None]
        k = np.argmin((r - vr[None]) ** 2 + (c - vc[None]) ** 2, axis=1)
        src[hr[a:a + 2048], hc[a:a + 2048]] = vr[k] * W + vc[k]
    return src


def fill_nearest(arr, nodata=np.nan):
    arr = np.asarray(arr, F)
    return arr.reshape(-1)[fill_sources(arr, nodata)]


# ---------------------------------------------------------------------------------------------------------------------------------- export
def elev_int16(elev):
    """np.clip(elev, -32768, 32767).astype(np.int16) with NaN written as 0: clip, then truncate toward zero."""
    e = np.asarray(elev, F)
    c = np.clip(np.where(np.isnan(e), F(0), e), F(-32768), F(32767))
    return np.trunc(c).astype(np.int32).astype(np.int16)


def load_and_pad(arr, nodata, internal_scale, default_value, padding=PADDING):
    """The padded import of a layer, pixel by pixel: a pixel that equals nodata or is NaN or infinite is default_value (0 without one), every
    pixel is multiplied by internal_scale in float32, and output pixel (i, j) is the pixel of the layer nearest to (i - padding, j - padding)."""
    a = np.asarray(arr).astype(F)
    H, W = a.shape
    fill = F(0.0) if default_value is None else F(default_value)
    out = np.empty((H + 2 * padding, W + 2 * padding), F)
    for i in range(out.shape[0]):
        r = min(max(i - padding, 0), H - 1)
        for j in range(out.shape[1]):
            v = a[r, min(max(j - padding, 0), W - 1)]
            if (nodata is not None and v == nodata) or np.isnan(v) or np.isinf(v):
                v = fill
            out[i, j] = v * F(internal_scale)
    return out


def export_boxes(H_cells, W_cells, chunk_size):
    """[(ci, cj, (i1, j1, i2, j2))] in row-major order: chunk (a, b) of chunk_size / 256 cells a side starts at cell (ci, cj), ends at the
    map's edge at the latest, and is read from the world 64 cells further down and right, 256 pixels per cell."""
    n = chunk_size // PIXELS_PER_CELL
    px = lambda cell: (cell + PADDING) * PIXELS_PER_CELL
    out = []
    for k in range(-(-H_cells // n) * -(-W_cells // n)):
        a, b = divmod(k, -(-W_cells // n))
        out.append((a * n, b * n, (px(a * n), px(b * n), px(min(a * n + n, H_cells)), px(min(b * n + n, W_cells)))))
    return out


def export_elevation(get_elev, H_cells, W_cells, chunk_size):
    """int16 (H_cells * 256, W_cells * 256): every chunk of get_elev(i1, j1, i2, j2) -> (h, w) float32, converted, at its place."""
    out = np.zeros((H_cells * PIXELS_PER_CELL, W_cells * PIXELS_PER_CELL), np.int16)
    for ci, cj, box in export_boxes(H_cells, W_cells, chunk_size):
        e = elev_int16(get_elev(*box))
        out[ci * PIXELS_PER_CELL:ci * PIXELS_PER_CELL + e.shape[0], cj * PIXELS_PER_CELL:cj * PIXELS_PER_CELL + e.shape[1]] = e
    return out


# ---------------------------------------------------------------------------------------------------------------------------------- Azgaar maps
def h_to_meters(h, exponent, ocean_max_depth=4000.0, ocean_power=1.5):
    """Metres of Azgaar's height h: pow(h - 18, exponent) from 20 up, else minus ocean_max_depth times pow((20 - h) / 20, ocean_power)."""
    import math
    return math.pow(h - 18.0, exponent) if h >= 20 else -(ocean_max_depth * math.pow((20 - h) / 20, ocean_power))


def output_shape(coords, scale):
    """(out_h, out_w): the map's height and width in km (111.32 km per degree, a degree of longitude shortened by the cosine of the middle
    latitude) in pixels of `scale` km, rounded as Python rounds, at least 1."""
    import math
    km_h = (coords["latN"] - coords["latS"]) * 111.32
    km_w = (coords["lonE"] - coords["lonW"]) * (111.32 * math.cos(math.radians((coords["latN"] + coords["latS"]) / 2)))
    return tuple(max(1, round(km / scale)) for km in (km_h, km_w))


def _csr(cells, verts, sx, sy, value_fn):
    xy, offsets, values = [], [0], []
    for cell in cells:
        value = value_fn(cell)
        if value is None or (isinstance(value, float) and np.isnan(value)):
            continue
        if any(vi not in verts for vi in cell["v"]):
            continue
        xy.extend([verts[vi][0] * sx, verts[vi][1] * sy] for vi in cell["v"])
        offsets.append(len(xy))
        values.append(value)
    return np.array(xy, np.float64).reshape(-1, 2), np.array(offsets, np.int32), np.array(values, F)


def azgaar_layers(m, biome_table, scale=100.0, ocean_max_depth=4000.0, ocean_power=1.5):
    """The five layers of azgaar_to_tiff's main for the parsed map `m`, with `biome_table` (13, 2) [temperature std, precipitation CV]."""
    out_h, out_w = output_shape(m["mapCoordinates"], scale)
    sx, sy = out_w / m["info"]["width"], out_h / m["info"]["height"]
    exponent = float(m["settings"]["heightExponent"])
    gv = {v["i"]: v["p"] for v in m["grid"]["vertices"]}
    pv = {v["i"]: v["p"] for v in m["pack"]["vertices"]}

    def number(cell, key, times):
        return float(cell[key]) * times if key in cell else None

    def biome(col):
        def fn(c):
            b = c.get("biome", 0)
            return float(biome_table[b][col]) if 0 <= b < len(biome_table) else float("nan")
        return fn
    spec = {"heightmap": (m["grid"]["cells"], gv, lambda c: h_to_meters(c.get("h", 0), exponent, ocean_max_depth, ocean_power), np.nan),
            "temperature": (m["grid"]["cells"], gv, lambda c: number(c, "temp", 1.0), -9999.0),
            "temperature_std": (m["pack"]["cells"], pv, biome(0), -9999.0),
            "precipitation": (m["grid"]["cells"], gv, lambda c: number(c, "prec", 100.0), -9999.0),
            "precipitation_cv": (m["pack"]["cells"], pv, biome(1), -9999.0)}
    layers = {}
    for name, (cells, verts, fn, fill) in spec.items():
        layers[name] = fill_nearest(rasterize(*_csr(cells, verts, sx, sy, fn), (out_h, out_w), fill), fill)
    return layers, (out_h, out_w)


def voronoi_cells(n_sites, width, height, seed):
    """(sites (n, 2), vertices (nv, 2), rings: one list of vertex indices per site) of the Voronoi diagram of n_sites seeded sites in
    [0, width] x [0, height].  The sites are mirrored across the four edges, so every inner cell is bounded and the cells tile the rectangle."""
    from scipy.spatial import Voronoi
    rng = np.random.default_rng(seed)
    s = rng.random((n_sites, 2)) * [width, height]
    mirrored = np.concatenate([s, s * [-1, 1], s * [1, -1], [2 * width, 0] - s * [1, -1], [0, 2 * height] - s * [-1, 1]])
    vor = Voronoi(mirrored)
    rings = []
    for i in range(n_sites):
        region = vor.regions[vor.point_region[i]]
        assert region and -1 not in region
        rings.append(list(region))
    return s, vor.vertices, rings


def csr_of(vertices, rings, sx=1.0, sy=1.0):
    xy = np.concatenate([vertices[r] for r in rings]) * [sx, sy]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
    return np.ascontiguousarray(xy, np.float64), offsets


def synthetic_azgaar_map(n_grid=300, n_pack=200, width=960.0, height=540.0, seed=5, lat=(-30.0, 40.0), lon=(-60.0, 70.0)):
    """A full-export-shaped dict from two Voronoi diagrams: info, mapCoordinates, settings.heightExponent, grid.vertices / grid.cells with
    v / h / temp / prec, pack.vertices / pack.cells with v / biome.  Some grid cells are ocean (h < 20), a few lack temp or prec, one names a
    missing vertex; pack cells over the first biomes include biome 0 (marine: NaN, so skipped) and one without a biome key."""
    rng = np.random.default_rng(seed + 1000)

    def block(n, s):
        sites, verts, rings = voronoi_cells(n, width, height, s)
        return sites, [{"i": int(i), "p": [float(x), float(y)]} for i, (x, y) in enumerate(verts)], rings
    gs, gverts, grings = block(n_grid, seed)
    ps, pverts, prings = block(n_pack, seed + 1)
    gcells = []
    for i, ring in enumerate(grings):
        x, y = gs[i]
        h = int(np.clip(35 + 40 * np.sin(x / 150.0) * np.cos(y / 110.0) + rng.integers(-4, 5), 0, 100))
        c = {"i": i, "v": [int(v) for v in ring], "h": h, "temp": int(round(25 - 40 * y / height)), "prec": int(rng.integers(0, 40))}
        if i % 37 == 5:
            del c["temp"]
        if i % 41 == 7:
            del c["prec"]
        gcells.append(c)
    gcells[3]["v"] = gcells[3]["v"] + [10 ** 7]      # a vertex the export does not hold: the cell is skipped
    pcells = []
    for i, ring in enumerate(prings):
        c = {"i": i, "v": [int(v) for v in ring], "biome": int(rng.integers(0, 13))}
        if i % 29 == 3:
            del c["biome"]
        pcells.append(c)
    return {"info": {"width": width, "height": height}, "settings": {"heightExponent": "1.8"},
            "mapCoordinates": {"latN": lat[1], "latS": lat[0], "lonW": lon[0], "lonE": lon[1]},
            "grid": {"vertices": gverts, "cells": gcells}, "pack": {"vertices": pverts, "cells": pcells}}
