"""Dataset preparation on the GPU: from a DEM array to the `residual` chunk the autoencoder encodes, and the statistics that normalise it.

The reference does this on the CPU in the tail of process_single_file_base (terrain_diffusion/data/preprocessing/elevation_dataset.py:231-301)
and in calculate_stats_welford (data/preprocessing/calculate_stds.py:7-71):

  1. fill_voids          NaN pixels blended towards a low-resolution base by Euclidean distance (lines 231-240), the signed square root (269),
  2. block_median        lowres_exact: skimage.measure.block_reduce(x, (r, r), np.median) (270),
  3. laplacian_encode    data/laplacian_encoder.py:63-91 -> (residual, lowres) (271),
  4. land_share          the share of lowres > 0 per sub-chunk (273-289),
  5. moments             count, mean and sum of centred squares of a chunk; RunningStats combines them as the reference's Welford loop does.

The per-pixel work runs in dataset_csrc/dataset_kernels.hip through libtd_dataset.so (include/td_dataset.h) on the engine's stream; there is no
CPU fallback.  The low band of laplacian_encode comes from the engine's resampler (composition.resize_bilinear, anti-aliased, and
composition.gaussian_blur); the residual is evaluated per pixel (td_dataset_residual) and the upsampled plane is never written.

Stated, not reproduced:
  * TF.resize(BILINEAR) and TF.gaussian_blur are PARITY-UNPINNED against torchvision, as composition.py states: torchvision is not installed
    here, they are pinned against torch's own F.interpolate / conv2d (oracle/compose.py), which is what torchvision calls.
  * Reading rasters (read_raster, extract_mask_from_tiffs), HDF5, the debug PNG and the skimage.transform.resize / skimage.filters.gaussian
    calls of lines 212-229 stay with the caller: prepare_chunks takes the two arrays they produce.  Climate layers pass through untouched and
    are not part of the returned dicts.
"""
import ctypes as C

import numpy as np
import torch

from . import composition
from ._lib import Library
from ._plumbing import call, engine_for as _engine_for, f32 as _f32, shape as _shape

_P = C.c_void_p
_SIGS = {
    "td_dataset_last_error": (C.c_char_p, []),
    "td_dataset_fill_voids": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
    "td_dataset_block_median": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "td_dataset_residual": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "td_dataset_land_counts": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "td_dataset_moments": (C.c_int, [_P, _P, C.c_int, C.c_int64, _P, _P, _P, C.c_int]),
}
EXPORTS = tuple(_SIGS)
_LIB = Library("libtd_dataset.so", _SIGS, "td_dataset_last_error", "td_dataset")
LIB_PATH, lib, check = _LIB.path, _LIB.lib, _LIB.check

MAX_SIDE = 16384            # include/td_dataset.h TD_DATASET_MAX_SIDE: 1 <= H, W <= 16384
MAX_RADIUS = 64             # TD_DATASET_MAX_RADIUS
MAX_BLOCK = 32              # TD_DATASET_MAX_BLOCK
MAX_CHUNKS = 64             # TD_DATASET_MAX_CHUNKS
MAX_PLANES = 1024           # TD_DATASET_MAX_PLANES
MAX_ELEMENTS = 1 << 30      # TD_DATASET_MAX_ELEMENTS
VOID_RADIUS = 32            # elevation_dataset.py:238: alpha = min(1, distance / 32)


def _dp(t):
    return C.c_void_p(t.data_ptr())


def _plane(x, what):
    s = _shape(x) if hasattr(x, "shape") else np.shape(x)
    if len(s) != 2:
        raise ValueError(f"{what} must be (H, W), got {tuple(s)}")
    H, W = int(s[0]), int(s[1])
    if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what} {H} x {W} outside the library's limit (1 <= H, W <= {MAX_SIDE})")
    return H, W


# ------------------------------------------------------------------------------------------------------------------------------ device forms
def _check_fill(dem, base, radius):
    H, W = _plane(dem, "dem")
    if _plane(base, "base") != (H, W):
        raise ValueError(f"base is {tuple(np.shape(base))}, dem is {(H, W)}: the two planes have one shape")
    radius = int(radius)
    if radius < 1 or radius > MAX_RADIUS:
        raise ValueError(f"radius must be in 1 .. {MAX_RADIUS}, got {radius}")
    return H, W, radius


@torch.no_grad()
def fill_voids(dem, base, radius=VOID_RADIUS, signed_sqrt=False, *, return_count=False, engine=None):
    """dem, base (H, W) -> fp32 (H, W) device tensor: every NaN pixel p of dem takes fp32(float64(base[p]) * min(1, d / radius)), d the exact
    Euclidean distance to the nearest valid pixel (scipy.ndimage.distance_transform_edt of the NaN mask); valid pixels keep their bits; a dem
    without one valid pixel comes out as base.  signed_sqrt=True stores sign(v) * sqrt(|v|) of every value (the reference takes it after the
    fill).  return_count=True also returns the number of voids as an int32 device tensor of one element (no read-back here)."""
    H, W, radius = _check_fill(dem, base, radius)
    engine, dev = _engine_for(dem, engine)
    d, b = _f32(dem, dev), _f32(base, dev)
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    voids = torch.empty(1, dtype=torch.int32, device=dev)
    call(_LIB, "td_dataset_fill_voids", engine, dev, _dp(d), _dp(b), H, W, radius, int(bool(signed_sqrt)), _dp(out), _dp(voids), ordered=True)
    return (out, voids) if return_count else out


def _check_median(x, r):
    H, W = _plane(x, "x")
    r = int(r)
    if r < 1 or r > MAX_BLOCK:
        raise ValueError(f"r must be in 1 .. {MAX_BLOCK}, got {r}")
    if H % r or W % r:
        raise ValueError(f"r = {r} does not divide {H} x {W}")
    return H, W, r


@torch.no_grad()
def block_median(x, r, *, engine=None):
    """x (H, W) -> fp32 (H / r, W / r) device tensor: skimage.measure.block_reduce(x, (r, r), np.median); a block with a NaN gives NaN."""
    H, W, r = _check_median(x, r)
    engine, dev = _engine_for(x, engine)
    a = _f32(x, dev)
    out = torch.empty((H // r, W // r), dtype=torch.float32, device=dev)
    call(_LIB, "td_dataset_block_median", engine, dev, _dp(a), H, W, r, _dp(out), ordered=True)
    return out


def _lowres_size(H, W, downsample_size):
    """The (h, w) TF.resize(x, downsample_size) gives: an int is the smaller edge (composition._resize_int_size), a pair is taken as it is."""
    if isinstance(downsample_size, (tuple, list)):
        if len(downsample_size) != 2:
            raise ValueError(f"downsample_size must be an int or (h, w), got {downsample_size!r}")
        h, w = int(downsample_size[0]), int(downsample_size[1])
    else:
        h, w = composition._resize_int_size(H, W, int(downsample_size))
    if h < 1 or w < 1 or h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f"downsample_size {downsample_size!r} gives a {h} x {w} low band (1 <= h, w <= {MAX_SIDE})")
    return h, w


def _check_encode(x, downsample_size, sigma, interp_mode, extrapolate):
    if extrapolate:
        raise ValueError("laplacian_encode: extrapolate=True is not supported (the dataset preparation never passes it)")
    if str(getattr(interp_mode, "value", interp_mode)).lower() != "bilinear":
        raise ValueError(f"laplacian_encode: only bilinear interpolation is supported, got {interp_mode!r}")
    H, W = _plane(x, "x")
    if not float(sigma) > 0:
        raise ValueError(f"sigma must be positive, got {sigma!r}")
    return (H, W) + _lowres_size(H, W, downsample_size)


@torch.no_grad()
def residual(x, low, *, out=None, engine=None):
    """x (H, W), low (h, w) -> fp32 (H, W) device tensor x - up(low), up = torch's bilinear upsampling with align_corners=False evaluated per
    pixel (td_dataset_residual).  out=x writes in place."""
    H, W = _plane(x, "x")
    h, w = _plane(low, "low")
    engine, dev = _engine_for(x, engine)
    a, l = _f32(x, dev), _f32(low, dev)
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and _shape(out) == (H, W) and out.is_contiguous()):
        raise ValueError("out must be a contiguous fp32 device tensor of x's shape")
    call(_LIB, "td_dataset_residual", engine, dev, _dp(a), _dp(l), H, W, h, w, _dp(out), ordered=True)
    return out


@torch.no_grad()
def laplacian_encode(x, downsample_size, sigma, interp_mode="bilinear", extrapolate=False, *, engine=None):
    """laplacian_encoder.py:63-91 for one plane x (H, W) -> (residual (H, W), lowres (h, w)) fp32 device tensors: lowres = gaussian_blur(
    resize(x, downsample_size)) on the engine's resampler (anti-aliased bilinear; kernel_size int(2 sigma) // 2 * 2 + 1, reflect padding),
    residual = x - resize(lowres, (H, W)).  extrapolate=True and other interpolation modes are refused."""
    H, W, h, w = _check_encode(x, downsample_size, sigma, interp_mode, extrapolate)
    engine, dev = _engine_for(x, engine)
    a = _f32(x, dev)
    low = composition.gaussian_blur(engine, composition.resize_bilinear(engine, a, (h, w)), sigma).contiguous()
    return residual(a, low, engine=engine), low


def _check_chunks(low, num_chunks):
    h, w = _plane(low, "low")
    num_chunks = int(num_chunks)
    if num_chunks < 1 or num_chunks > min(MAX_CHUNKS, h, w):
        raise ValueError(f"num_chunks must be in 1 .. min({MAX_CHUNKS}, h, w), got {num_chunks} for {h} x {w}")
    return h, w, num_chunks


@torch.no_grad()
def land_counts(low, num_chunks=1, *, engine=None):
    """low (h, w) -> int32 (num_chunks, num_chunks) device tensor: the number of low > 0 in each sub-chunk of side h // num_chunks,
    w // num_chunks (NaN is not > 0)."""
    h, w, num_chunks = _check_chunks(low, num_chunks)
    engine, dev = _engine_for(low, engine)
    a = _f32(low, dev)
    counts = torch.empty((num_chunks, num_chunks), dtype=torch.int32, device=dev)
    call(_LIB, "td_dataset_land_counts", engine, dev, _dp(a), h, w, num_chunks, _dp(counts), ordered=True)
    return counts


@torch.no_grad()
def land_share(low, num_chunks=1, *, engine=None):
    """low (h, w) -> float64 (num_chunks, num_chunks) device tensor: np.mean(sub-chunk > 0) of elevation_dataset.py:289 for every sub-chunk."""
    h, w, num_chunks = _check_chunks(low, num_chunks)
    counts = land_counts(low, num_chunks, engine=engine).double()
    # a tensor divisor: a true float64 division per element (a Python scalar may be turned into a multiplication by its reciprocal)
    return counts / torch.full((), float((h // num_chunks) * (w // num_chunks)), dtype=torch.float64, device=counts.device)


def _check_moments(x):
    s = tuple(int(d) for d in np.shape(x))
    if len(s) == 0 or any(d < 1 for d in s):
        raise ValueError(f"x must hold at least one value, got shape {s}")
    planes = s[0] if len(s) == 3 else 1                  # calculate_stds.py:31: a 3-D array is (channels, H, W), anything else one plane
    n = int(np.prod(s)) // planes
    if planes > MAX_PLANES or n > MAX_ELEMENTS or planes * n > 1 << 32:
        raise ValueError(f"{planes} planes of {n} values beyond the library's limit (C <= {MAX_PLANES}, n <= 2^30, C * n <= 2^32)")
    return planes, n


@torch.no_grad()
def moments(x, *, engine=None):
    """The chunk summary of calculate_stats_welford: x (C, H, W) is C planes, any other shape one plane -> (count int64 (1,), mean float64
    (C,), m2 float64 (C,)) device tensors over the positions where no plane holds a NaN: their number, the mean per plane and the sum of
    (x - mean)^2 per plane, all sums in float64 through a fixed tree (two calls give the same bits)."""
    planes, n = _check_moments(x)
    engine, dev = _engine_for(x, engine)
    a = _f32(x, dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    mean = torch.empty(planes, dtype=torch.float64, device=dev)
    m2 = torch.empty(planes, dtype=torch.float64, device=dev)
    call(_LIB, "td_dataset_moments", engine, dev, _dp(a), planes, n, _dp(count), _dp(mean), _dp(m2), ordered=True)
    return count, mean, m2


# ------------------------------------------------------------------------------------------------------------------------------ drop-ins
def mask_voids(dem, data_source):
    """elevation_dataset.py:206-210: the DEM as float32 with its nodata pixels as NaN -- `merit`: below -1000, `copernicus`: equal to 0.
    A numpy array gives a numpy array, a tensor a tensor on its device."""
    if data_source not in ("merit", "copernicus"):
        raise ValueError(f"data_source must be 'merit' or 'copernicus', got {data_source!r}")
    if torch.is_tensor(dem):
        bad = dem < -1000 if data_source == "merit" else dem == 0.0
        return torch.where(bad, torch.full((), float("nan"), dtype=torch.float32, device=dem.device), dem.to(torch.float32))
    a = np.asarray(dem)
    bad = a < -1000 if data_source == "merit" else a == 0.0
    return np.where(bad, np.nan, a).astype(np.float32)


def chunk_boxes(highres_size, lowres_size, num_chunks=1, edge_margin=0):
    """elevation_dataset.py:199 and 273-287 as index arithmetic -> (highres_margin, [(subchunk_id, (h0, h1, w0, w1) in the cropped high-resolution
    plane, (l0, l1, m0, m1) in the low-resolution planes)]), row-major over the sub-chunks; the ends are already clipped to the planes."""
    highres_size, lowres_size, num_chunks, edge_margin = int(highres_size), int(lowres_size), int(num_chunks), int(edge_margin)
    if lowres_size < 1 or highres_size % lowres_size != 0:
        raise ValueError(f"highres_size {highres_size} must be a multiple of lowres_size {lowres_size}")
    if edge_margin < 0 or 2 * edge_margin >= lowres_size:
        raise ValueError(f"edge_margin {edge_margin} leaves nothing of a {lowres_size} x {lowres_size} low band")
    low_side = lowres_size - 2 * edge_margin
    if num_chunks < 1 or num_chunks > min(MAX_CHUNKS, low_side):
        raise ValueError(f"num_chunks must be in 1 .. min({MAX_CHUNKS}, {low_side}), got {num_chunks}")
    highres_margin = edge_margin * highres_size // lowres_size
    high_side = highres_size - 2 * highres_margin
    hc, lc = high_side // num_chunks, low_side // num_chunks
    boxes = []
    for ch in range(num_chunks):
        for cw in range(num_chunks):
            hs, ws, ls, ms = ch * hc, cw * hc, ch * lc, cw * lc
            high = (hs, min(hs + hc, highres_size, high_side), ws, min(ws + hc, highres_size, high_side))
            low = (ls, min(ls + lc, lowres_size, low_side), ms, min(ms + lc, lowres_size, low_side))
            boxes.append((f"chunk_{ch}_{cw}", high, low))
    return highres_margin, boxes


def _check_prepare(highres_dem, scaled_base_lowres_dem, lowres_size, lowres_sigma, num_chunks, edge_margin):
    H, W = _plane(highres_dem, "highres_dem")
    if H != W:
        raise ValueError(f"highres_dem must be square (highres_size x highres_size), got {H} x {W}")
    if _plane(scaled_base_lowres_dem, "scaled_base_lowres_dem") != (H, W):
        raise ValueError(f"scaled_base_lowres_dem is {tuple(np.shape(scaled_base_lowres_dem))}, highres_dem is {(H, W)}: both are at highres_size")
    margin, boxes = chunk_boxes(H, lowres_size, num_chunks, edge_margin)
    ratio = H // int(lowres_size)
    if ratio > MAX_BLOCK:
        raise ValueError(f"highres_size / lowres_size = {ratio} beyond the block median's limit of {MAX_BLOCK}")
    if not float(lowres_sigma) > 0:
        raise ValueError(f"lowres_sigma must be positive, got {lowres_sigma!r}")
    return H, margin, ratio, boxes


@torch.no_grad()
def prepare_chunks(highres_dem, scaled_base_lowres_dem, lowres_size, lowres_sigma, num_chunks=1, edge_margin=0, chunk_id=None, *, beauty_scores=False,
                   engine=None):
    """elevation_dataset.py:218-219 and 228-301 for arrays already at highres_size: highres_dem (voids as NaN, see mask_voids) and
    scaled_base_lowres_dem, both (highres_size, highres_size).  The margin crop, the void fill (radius 32), the signed square root, lowres_exact
    (the block median over highres_size // lowres_size), laplacian_encode(..., lowres_size - 2 * edge_margin, lowres_sigma) and the land share.
    Returns the reference's list of dicts, one per sub-chunk in row-major order: residual, lowfreq, lowres_exact (fp32 device tensors, views of
    the whole planes), pct_land (float), chunk_id, subchunk_id; `climate` is absent.  One device-to-host copy per call: the land counts.
    beauty_scores=True adds `beauty_score` to every dict: beauty.calculate_beauty_score of its lowfreq and residual (data/preprocessing/
    beauty_score.py), all sub-chunks in one device batch before the planes leave the device, with one more small read-back; the sub-chunk side
    must then be a power of two in 8 .. 4096 (NotImplementedError otherwise)."""
    size, margin, ratio, boxes = _check_prepare(highres_dem, scaled_base_lowres_dem, lowres_size, lowres_sigma, num_chunks, edge_margin)
    engine, dev = _engine_for(highres_dem, engine)
    dem, base = _f32(highres_dem, dev), _f32(scaled_base_lowres_dem, dev)
    if margin > 0:
        dem, base = dem[margin:-margin, margin:-margin], base[margin:-margin, margin:-margin]
    filled = fill_voids(dem, base, VOID_RADIUS, True, engine=engine)
    lowres_exact = block_median(filled, ratio, engine=engine)
    res, lowfreq = laplacian_encode(filled, int(lowres_size) - 2 * int(edge_margin), lowres_sigma, engine=engine)
    counts = land_counts(lowfreq, num_chunks, engine=engine).cpu().numpy().reshape(-1)
    chunks = []
    for k, (subchunk_id, (h0, h1, w0, w1), (l0, l1, m0, m1)) in enumerate(boxes):
        chunks.append({"residual": res[h0:h1, w0:w1], "lowfreq": lowfreq[l0:l1, m0:m1], "lowres_exact": lowres_exact[l0:l1, m0:m1],
                       "pct_land": float(counts[k]) / float((l1 - l0) * (m1 - m0)), "chunk_id": chunk_id, "subchunk_id": subchunk_id})
    if beauty_scores:
        from . import beauty
        scores = beauty._scores(torch.stack([c["lowfreq"] for c in chunks]), torch.stack([c["residual"] for c in chunks]), engine)
        for chunk, score in zip(chunks, scores):
            chunk["beauty_score"] = score
    return chunks


@torch.no_grad()
def prepare_and_encode(autoencoder, highres_dem, scaled_base_lowres_dem, lowres_size, lowres_sigma, residual_mean, residual_std, num_chunks=1,
                       edge_margin=0, chunk_id=None, *, engine=None):
    """prepare_chunks, then autoencoder.encode_dihedral(residual, residual_mean, residual_std) on every sub-chunk (build_encoded_dataset.py:68-94):
    each dict gains `latents`, the (8, 2 (L + D), S / down, S / down) float16 device tensor.  The residual does not visit the host."""
    chunks = prepare_chunks(highres_dem, scaled_base_lowres_dem, lowres_size, lowres_sigma, num_chunks, edge_margin, chunk_id, engine=engine)
    for chunk in chunks:
        chunk["latents"] = autoencoder.encode_dihedral(chunk["residual"][None].contiguous(), residual_mean, residual_std)
    return chunks


class RunningStats:
    """The running mean / M2 of calculate_stats_welford, fed with chunk summaries (moments) instead of the chunks themselves.  With m0 the
    running mean before an update and m1 after it, a chunk of n values with mean mean_c and centred squares m2_c gives
        cnt += n;  m1 = m0 + n (mean_c - m0) / cnt;  M2 += m2_c + n (mean_c - m0) (mean_c - m1),
    algebraically the reference's sum(delta) / cnt and sum(delta * delta2).  Host float64, per plane."""

    def __init__(self, planes=None):
        """planes=None: one plane, result() gives scalars (the reference's 2-D path); an int: that many planes, result() gives arrays."""
        self.scalar = planes is None
        k = 1 if planes is None else int(planes)
        self.count = 0
        self.mean = np.zeros(k, dtype=np.float64)
        self.m2 = np.zeros(k, dtype=np.float64)

    def update(self, count, mean, m2):
        n = int(count)
        mean_c = np.asarray(mean, dtype=np.float64).reshape(-1)
        m2_c = np.asarray(m2, dtype=np.float64).reshape(-1)
        if mean_c.shape != self.mean.shape or m2_c.shape != self.mean.shape:
            raise ValueError(f"a summary of {mean_c.size} planes for statistics of {self.mean.size}")
        if n < 0:
            raise ValueError(f"count must not be negative, got {n}")
        if n == 0:
            return self
        self.count += n
        m0 = self.mean
        m1 = m0 + np.float64(n) * (mean_c - m0) / np.float64(self.count)
        self.m2 = self.m2 + (m2_c + np.float64(n) * (mean_c - m0) * (mean_c - m1))
        self.mean = m1
        return self

    def result(self):
        """(means, stds), stds = sqrt(M2 / (count - 1)); scalars for one plane (planes=None), arrays otherwise."""
        with np.errstate(divide="ignore", invalid="ignore"):
            stds = np.sqrt(self.m2 / np.float64(self.count - 1))
        return (np.float64(self.mean[0]), np.float64(stds[0])) if self.scalar else (self.mean.copy(), stds)


def calculate_stats_welford(res_group, dataset_name, min_stat_landcover_pct=0.0, *, engine=None):
    """Drop-in for calculate_stds.py:7-71 over any mapping shaped like the HDF5 group -- res_group[chunk][subchunk][dataset_name] array-like
    with .attrs['pct_land'] -- (h5py is not required): (means, stds) in float64, scalars for 2-D datasets and arrays per channel for 3-D ones.
    Every chunk is summarised on the GPU (moments: float64 sums over the positions where no channel holds a NaN) and the summaries are combined
    on the host (RunningStats); one small read-back per chunk.  The data is taken as float32, the type the dataset is written in; every sum is
    in float64, where the reference's 2-D path subtracts and multiplies in float32."""
    first = None
    for chunk_id in res_group.keys():
        for subchunk_id in res_group[chunk_id].keys():
            if dataset_name in res_group[chunk_id][subchunk_id]:
                first = res_group[chunk_id][subchunk_id][dataset_name]
        if first is not None:
            break
    if first is None:
        raise ValueError(f"No {dataset_name} data found in the dataset")
    stats = RunningStats(int(np.shape(first)[0]) if len(np.shape(first)) == 3 else None)
    for chunk_id in res_group.keys():
        chunk_group = res_group[chunk_id]
        for subchunk_id in chunk_group.keys():
            subchunk_group = chunk_group[subchunk_id]
            if dataset_name in subchunk_group and subchunk_group[dataset_name].attrs["pct_land"] >= min_stat_landcover_pct:
                data = subchunk_group[dataset_name]
                data = data if torch.is_tensor(data) else np.asarray(data[:])
                count, mean, m2 = moments(data, engine=engine)
                stats.update(int(count.cpu()), mean.cpu().numpy(), m2.cpu().numpy())
    return stats.result()
