"""Float64 / NumPy twin of the dataset-preparation library (include/td_dataset.h, terrain_diffusion_amd/dataset.py): the five operations and the
chunk routine of the reference's process_single_file_base (terrain_diffusion/data/preprocessing/elevation_dataset.py:231-301) and the Welford
loop of calculate_stats_welford (data/preprocessing/calculate_stds.py:7-71), stated independently of the kernels.

  fill_voids      the void rule on an exact Euclidean distance transform (edt: integer squared distances, float64 sqrt -- what
                  scipy.ndimage.distance_transform_edt returns; tests/golden/dataset.npz pins it to scipy bit for bit).  fill_voids_capped states the
                  kernels' search (column distances capped at radius, row pass over |dx| < radius) in NumPy: the CPU test holds the two equal.
  block_median    np.median over the reshaped blocks (pinned to np.median of every block on its own by the fixture).
  residual_ref    x - up(low) in float64 with the fp32 taps of torch's upsample_bilinear2d (align_corners=False), and the bound E per element.
  land_counts     counts of low > 0 per sub-chunk.
  moments         count / mean / sum of centred squares in float64 over the positions where no plane holds a NaN.
  welford         the reference's loop, restated line by line (the fixture holds the outputs of the reference's own function).
  prepare_chunks  the chunk routine on the CPU; its low band is oracle.compose.laplacian_encode.

PARITY-UNPINNED, as terrain_diffusion_amd/composition.py and oracle/compose.py state: torchvision is not installed here, so TF.resize(BILINEAR) and
TF.gaussian_blur are restated as torch's own F.interpolate(antialias=True) / reflect-padded conv2d, the calls torchvision makes; the low band of
laplacian_encode is pinned to those, not to torchvision itself.

The residual's bound ("Dataset preparation"), u = 2^-24.  The kernel evaluates, in fp32 without contraction,
    up = wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * d),   out = x - up
with the fp32 weights as given (they are inputs of the formula: the twin uses the same fp32 weights).  Every tap's term w_y w_x t passes through
four roundings on its way into up -- its product with w_x, the inner sum, the product with w_y, the outer sum -- so in the standard model
|up_fp32 - up| <= ((1 + u)^4 - 1) M, M = sum over the four taps of |w_y w_x t|: the magnitude of the four taps.  The subtraction adds one rounding
of the result, half an ulp of the difference: u |out|.  With (1 + u)^4 - 1 <= 4 u (1 + 2^-10) and the products of two roundings under the same factor:
    E = (4 u M + u |out_ref|) (1 + 2^-10).
Nothing here is tuned: RESIDUAL_ROUNDINGS is the count above.
"""
import numpy as np

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -10
RESIDUAL_ROUNDINGS = 4              # roundings between a tap and the upsampled value (see the module docstring)
F = np.float32
VOID_RADIUS = 32


# ------------------------------------------------------------------------------------------------------------------------------ void fill
def _column_distances(mask):
    """int64 (H, W): vertical distance from every pixel to the nearest valid (False) pixel of its column, BIG where the column has none"""
    H, W = mask.shape
    BIG = 1 << 20
    g = np.full((H, W), BIG, np.int64)
    d = np.full(W, BIG, np.int64)
    for r in range(H):
        d = np.where(mask[r], d + 1, 0)
        g[r] = d
    d = np.full(W, BIG, np.int64)
    for r in range(H - 1, -1, -1):
        d = np.where(mask[r], d + 1, 0)
        g[r] = np.minimum(g[r], d)
    return np.minimum(g, BIG)


def edt2(mask):
    """int64 (H, W): the exact squared Euclidean distance from every void (True) pixel to the nearest valid pixel, 0 on valid pixels (a mask
    without a valid pixel gives a huge number everywhere)"""
    mask = np.asarray(mask, bool)
    g = _column_distances(mask)
    W = mask.shape[1]
    dx2 = (np.arange(W)[:, None] - np.arange(W)[None, :]).astype(np.int64) ** 2
    out = np.empty(mask.shape, np.int64)
    for r in range(mask.shape[0]):
        out[r] = (dx2 + (g[r] ** 2)[None, :]).min(1)
    return out


def edt(mask):
    """float64 (H, W): scipy.ndimage.distance_transform_edt(mask)"""
    return np.sqrt(edt2(mask).astype(np.float64))


def signed_sqrt(v):
    v = np.asarray(v, F)
    return (np.sign(v) * np.sqrt(np.abs(v))).astype(F)


def fill_voids(dem, base, radius=VOID_RADIUS, signed=False, distance=None):
    """(out fp32 (H, W), number of voids): elevation_dataset.py:231-240, and :269 with signed; `distance`: edt(isnan(dem)) where the caller has it"""
    dem, base = np.asarray(dem, F), np.asarray(base, F)
    mask = np.isnan(dem)
    out = dem.copy()
    if mask.all():
        out = base.copy()
    elif mask.any():
        alpha = np.minimum(1.0, (edt(mask) if distance is None else distance)[mask] / np.float64(radius))
        out[mask] = (base[mask].astype(np.float64) * alpha).astype(F)
    return (signed_sqrt(out) if signed else out), int(mask.sum())


def fill_voids_capped(dem, base, radius=VOID_RADIUS):
    """The same through the search the kernels make: column distances capped at radius, then min(dx^2 + g^2) over |dx| < radius; alpha = 1
    from radius^2 on."""
    dem, base = np.asarray(dem, F), np.asarray(base, F)
    mask = np.isnan(dem)
    H, W = mask.shape
    g = np.minimum(_column_distances(mask), radius)
    padded = np.full((H, W + 2 * (radius - 1)), radius, np.int64)
    padded[:, radius - 1:radius - 1 + W] = g
    best = np.full((H, W), 1 << 40, np.int64)
    for dx in range(-(radius - 1), radius):
        best = np.minimum(best, dx * dx + padded[:, radius - 1 + dx:radius - 1 + dx + W] ** 2)
    alpha = np.where(best < radius * radius, np.sqrt(best.astype(np.float64)) / np.float64(radius), 1.0)
    out = dem.copy()
    out[mask] = (base[mask].astype(np.float64) * alpha[mask]).astype(F)
    return out


# ------------------------------------------------------------------------------------------------------------------------------ block median
def blocks_of(x, r):
    """(H / r, W / r, r * r): the values of every r x r block, row-major inside the block"""
    H, W = x.shape
    return x.reshape(H // r, r, W // r, r).transpose(0, 2, 1, 3).reshape(H // r, W // r, r * r)


def block_median(x, r):
    """skimage.measure.block_reduce(x, (r, r), np.median) for r dividing both sides"""
    with np.errstate(invalid="ignore"), __import__("warnings").catch_warnings():
        __import__("warnings").simplefilter("ignore", RuntimeWarning)
        return np.median(blocks_of(np.asarray(x, F), r), axis=-1).astype(F)


# ------------------------------------------------------------------------------------------------------------------------------ residual
def bilinear_taps(n_in, n_out):
    """torch upsample_bilinear2d, align_corners=False, in fp32: (i0, i1 int64 (n_out,), l0, l1 fp32 (n_out,))"""
    scale = F(n_in) / F(n_out)
    dst = np.arange(n_out, dtype=F)
    src = np.maximum(scale * (dst + F(0.5)) - F(0.5), F(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(F)).astype(F)
    l0 = (F(1) - l1).astype(F)
    return i0, i1, l0, l1


def upsample_ref(low, H, W):
    """float64 (up, M): the bilinear upsampling of the fp32 plane low to (H, W) with the fp32 weights, and M = sum |w_y w_x tap|"""
    low = np.asarray(low, F).astype(np.float64)
    h, w = low.shape
    i0, i1, wy0, wy1 = bilinear_taps(h, H)
    j0, j1, wx0, wx1 = bilinear_taps(w, W)
    wy0, wy1, wx0, wx1 = (v.astype(np.float64) for v in (wy0, wy1, wx0, wx1))
    a, b, c, d = low[i0][:, j0], low[i0][:, j1], low[i1][:, j0], low[i1][:, j1]
    terms = [wy0[:, None] * wx0[None] * a, wy0[:, None] * wx1[None] * b, wy1[:, None] * wx0[None] * c, wy1[:, None] * wx1[None] * d]
    return sum(terms), sum(np.abs(t) for t in terms)


def residual_ref(x, low):
    """float64 (ref, E) of td_dataset_residual on the fp32 inputs: ref = x - up(low), E per element as the module docstring derives it"""
    x = np.asarray(x, F).astype(np.float64)
    up, M = upsample_ref(low, *x.shape)
    ref = x - up
    return ref, (RESIDUAL_ROUNDINGS * U * M + U * np.abs(ref)) * SECOND_ORDER


# ------------------------------------------------------------------------------------------------------------------------------ land counts
def land_counts(low, num_chunks):
    low = np.asarray(low, F)
    sh, sw = low.shape[0] // num_chunks, low.shape[1] // num_chunks
    with np.errstate(invalid="ignore"):
        return np.array([[int((low[ch * sh:(ch + 1) * sh, cw * sw:(cw + 1) * sw] > 0).sum()) for cw in range(num_chunks)]
                         for ch in range(num_chunks)], np.int64)


# ------------------------------------------------------------------------------------------------------------------------------ statistics
def moments(x):
    """(count, mean float64 (C,), m2 float64 (C,)) of x -- (C, H, W): C planes, any other shape: one -- over the positions where no plane is NaN"""
    x = np.asarray(x)
    planes = x.reshape(x.shape[0], -1) if x.ndim == 3 else x.reshape(1, -1)
    planes = planes[:, ~np.isnan(planes).any(axis=0)].astype(np.float64)
    n = planes.shape[1]
    if n == 0:
        return 0, np.zeros(planes.shape[0]), np.zeros(planes.shape[0])
    mean = planes.sum(1) / n
    return n, mean, ((planes - mean[:, None]) ** 2).sum(1)


class Data:
    """An array with .attrs, as an HDF5 dataset"""

    def __init__(self, array, pct_land):
        self.array, self.attrs, self.shape = array, {"pct_land": pct_land}, array.shape

    def __getitem__(self, key):
        return self.array[key]


def welford(res_group, dataset_name, min_stat_landcover_pct=0.0):
    """calculate_stds.py:7-71 restated: the reference's running update, chunk by chunk, in the arithmetic NumPy gives the data's type"""
    first = None
    for chunk_id in res_group.keys():
        for subchunk_id in res_group[chunk_id].keys():
            if dataset_name in res_group[chunk_id][subchunk_id]:
                first = res_group[chunk_id][subchunk_id][dataset_name][:]
        if first is not None:
            break
    assert first is not None
    if first.ndim == 3:
        C = first.shape[0]
        means, M2s, counts = np.zeros(C, np.float64), np.zeros(C, np.float64), np.zeros(C, np.int64)
    else:
        means, M2s, counts = 0.0, 0.0, 0
    for chunk_id in res_group.keys():
        for subchunk_id in res_group[chunk_id].keys():
            sub = res_group[chunk_id][subchunk_id]
            if dataset_name in sub and sub[dataset_name].attrs["pct_land"] >= min_stat_landcover_pct:
                data = sub[dataset_name][:]
                if data.ndim == 3:
                    cd = data.reshape(C, -1)
                    cd = cd[:, ~np.isnan(cd).any(axis=0)]
                    if cd.shape[1] == 0:
                        continue
                    counts += cd.shape[1]
                    delta = cd - means[:, np.newaxis]
                    means += np.sum(delta, axis=1) / counts
                    M2s += np.sum(delta * (cd - means[:, np.newaxis]), axis=1)
                else:
                    data = data.flatten()
                    data = data[~np.isnan(data)]
                    if len(data) == 0:
                        continue
                    counts += len(data)
                    delta = data - means
                    means += np.sum(delta) / counts
                    M2s += np.sum(delta * (data - means))
    return means, np.sqrt(M2s / (counts - 1))


def stats_group(seed=4100, n_chunks=5, side=256, planes=3, plane_side=48):
    """The group of the statistics checks, from the project's portable generator (oracle/rng.py: the same values on every machine; the fixture
    holds a CRC of them): per chunk one sub-chunk `chunk_0_0` with a 2-D `residual` (side x side fp32, a few NaNs) and a 3-D `climate`
    (planes x plane_side x plane_side, NaNs in one plane), and pct_land rising from 0 with the chunk."""
    from oracle import rng
    group = {}
    for k in range(n_chunks):
        res = (rng.standard_normal(seed + k, (side, side)) * F(1.3 + 0.2 * k) + F(0.9 - 0.1 * k)).astype(F)
        res.reshape(-1)[(k * 7919) % 1000::10007] = np.nan
        cl = (rng.standard_normal(seed + 100 + k, (planes, plane_side, plane_side)) * np.array([10.0, 0.5, 300.0], F)[:planes, None, None]
              + np.array([15.0, -2.0, 1000.0], F)[:planes, None, None]).astype(F)
        cl[1].reshape(-1)[k::97] = np.nan
        group[f"{k}"] = {"chunk_0_0": {"residual": Data(res, k / n_chunks), "climate": Data(cl, k / n_chunks)}}
    return group


def group_crc(group):
    import zlib
    crc = 0
    for c in group:
        for s in group[c]:
            for name in sorted(group[c][s]):
                crc = zlib.crc32(np.ascontiguousarray(group[c][s][name].array).tobytes(), crc)
    return crc


def cast_group(group, dtype):
    return {c: {s: {n: Data(d.array.astype(dtype), d.attrs["pct_land"]) for n, d in sub.items()} for s, sub in subs.items()} for c, subs in group.items()}


# ------------------------------------------------------------------------------------------------------------------------------ the chunk routine
def reference_boxes(highres_size, lowres_size, num_chunks, edge_margin):
    """elevation_dataset.py:199 and 273-287, the index arithmetic as written there, then clipped as NumPy clips a slice of the cropped planes:
    (highres_margin, [(subchunk_id, (h0, h1, w0, w1), (l0, l1, m0, m1))])"""
    highres_margin = edge_margin * highres_size // lowres_size
    highres_chunk_size = (highres_size - highres_margin * 2) // num_chunks
    lowres_chunk_size = (lowres_size - edge_margin * 2) // num_chunks
    high_side, low_side = highres_size - 2 * highres_margin, lowres_size - 2 * edge_margin
    boxes = []
    for chunk_h in range(num_chunks):
        for chunk_w in range(num_chunks):
            highres_start_h = chunk_h * highres_chunk_size
            highres_start_w = chunk_w * highres_chunk_size
            highres_end_h = min(highres_start_h + highres_chunk_size, highres_size)
            highres_end_w = min(highres_start_w + highres_chunk_size, highres_size)
            lowres_start_h = chunk_h * lowres_chunk_size
            lowres_start_w = chunk_w * lowres_chunk_size
            lowres_end_h = min(lowres_start_h + lowres_chunk_size, lowres_size)
            lowres_end_w = min(lowres_start_w + lowres_chunk_size, lowres_size)
            hh, hw = slice(highres_start_h, highres_end_h).indices(high_side), slice(highres_start_w, highres_end_w).indices(high_side)
            lh, lw = slice(lowres_start_h, lowres_end_h).indices(low_side), slice(lowres_start_w, lowres_end_w).indices(low_side)
            boxes.append((f"chunk_{chunk_h}_{chunk_w}", (hh[0], hh[1], hw[0], hw[1]), (lh[0], lh[1], lw[0], lw[1])))
    return highres_margin, boxes


def prepare_chunks(highres_dem, scaled_base, lowres_size, lowres_sigma, num_chunks=1, edge_margin=0, chunk_id=None):
    """elevation_dataset.py:218-219 and 228-301 on the CPU for arrays at highres_size; the low band through oracle.compose.laplacian_encode"""
    import torch
    from oracle import compose
    dem, base = np.asarray(highres_dem, F), np.asarray(scaled_base, F)
    size = dem.shape[0]
    margin, boxes = reference_boxes(size, lowres_size, num_chunks, edge_margin)
    if margin > 0:
        dem, base = dem[margin:-margin, margin:-margin], base[margin:-margin, margin:-margin]
    filled, _ = fill_voids(dem, base, VOID_RADIUS, True)
    lowres_exact = block_median(filled, size // lowres_size)
    res, low = compose.laplacian_encode(torch.from_numpy(filled), lowres_size - 2 * edge_margin, lowres_sigma)
    res, low = res.numpy(), low.numpy()
    out = []
    for sub, (h0, h1, w0, w1), (l0, l1, m0, m1) in boxes:
        out.append({"residual": res[h0:h1, w0:w1], "lowfreq": low[l0:l1, m0:m1], "lowres_exact": lowres_exact[l0:l1, m0:m1],
                    "pct_land": float(np.mean(low[l0:l1, m0:m1] > 0)), "chunk_id": chunk_id, "subchunk_id": sub})
    return out


# ------------------------------------------------------------------------------------------------------------------------------ the committed cases
def void_cases():
    """name -> (dem fp32 with NaN voids, base fp32): the smallest shapes at which the two passes can go wrong.  The column pass sweeps bands of
    128 rows, the row pass segments of 256 columns."""
    rng = np.random.default_rng(20251)
    cases = {}

    def planes(shape, mask):
        ii, jj = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
        dem = (900.0 * np.sin(ii / 23.0) * np.cos(jj / 31.0) + 37.0 * np.sin(ii * 0.9 + jj * 0.4) - 50.0).astype(F)
        base = (-(3.0 + 200.0 * (1 + np.sin(ii / 11.0 + jj / 17.0)))).astype(F)
        dem[mask] = np.nan
        return dem, base

    m = rng.random((150, 170)) < 0.2
    m[20:120, 30:140] = True                                # a hole of 100 x 110: wider than 2 x 32, deeper than one band boundary
    cases["hole_150x170"] = planes(m.shape, m)
    m = np.zeros((70, 90), bool)
    m[:9], m[-40:], m[:, :35], m[:, -5:] = True, True, True, True       # voids on all four borders, a valid island inside
    cases["borders_70x90"] = planes(m.shape, m)
    m = rng.random((1, 90)) < 0.6
    m[0, 10:80] = True
    m[0, 45] = False
    cases["row_1x90"] = planes(m.shape, m)
    m = rng.random((70, 1)) < 0.6
    m[5:60] = True
    cases["column_70x1"] = planes(m.shape, m)
    cases["no_void_40x50"] = planes((40, 50), np.zeros((40, 50), bool))
    cases["all_void_30x40"] = planes((30, 40), np.ones((30, 40), bool))
    m = rng.random((67, 259)) < 0.5                         # sides that are a multiple of nothing; a second row segment of 3 columns
    m[10:60, 200:259] = True
    cases["odd_67x259"] = planes(m.shape, m)
    m = rng.random((300, 37)) < 0.3                         # three bands of rows; voids across both band boundaries, one valid row far away
    m[90:290] = True
    m[200, ::2] = False
    cases["tall_300x37"] = planes(m.shape, m)
    return cases


MEDIAN_SHAPE = (96, 192)
MEDIAN_RS = (1, 2, 3, 8, 16, 32)


def median_input():
    """96 x 192 fp32: the left half full-precision values, the right half values on a coarse grid (many repeated values inside every block), a
    few exact duplicates of neighbours, zeros of both signs, and one NaN"""
    rng = np.random.default_rng(20252)
    x = (rng.standard_normal(MEDIAN_SHAPE) * 40.0).astype(F)
    x[:, 96:] = np.round(x[:, 96:] / 8.0) * 8.0
    x[::5, 1::7] = x[::5, 0::7][:, : x[::5, 1::7].shape[1]]
    x[40, 100], x[41, 101] = 0.0, -0.0
    x[70, 30] = np.nan
    return x
