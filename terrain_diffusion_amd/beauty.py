"""Beauty scores on the GPU: the last step of the reference's dataset build, and a radial log-spectrum for comparing terrain.

The reference does this on the CPU in terrain_diffusion/data/preprocessing/beauty_score.py, once per res / chunk / subchunk group:

  1. decode_terrain        laplacian_decode(residual, lowfreq), sign(d) d^2, the share of pixels <= 0, the clamp at 0, torch.std (lines 62-70),
  2. radial_spectrum       analyze_terrain_frequency (9-50): fft2, log|F|, the mean over `bins` rings of the frequency plane,
  3. the seven features and the linear model (71-87), on the host in Python floats exactly as the reference spells them,
  4. beauty_class          the bucket H5LatentsDataset sorts a group into (data/datasets/h5_latents_dataset.py:107).

The per-pixel work runs in spectrum_csrc/spectrum_kernels.hip through libtd_spectrum.so (include/td_spectrum.h) on the engine's stream; there
is no CPU fallback and no rocFFT / hipFFT: the transform is the library's own, for sides that are powers of two in 8 .. 4096 (anything else
raises NotImplementedError).  Every device form takes a leading batch of planes.

The bin map is not computed on the device: bin_map builds it once per (H, W, bins) on the host with the reference's own expressions --
torch.linspace(-1, 1, n), sqrt(x^2 + y^2), linspace(0, 1, bins + 1), all fp32, `>=` and `<` -- undoes the fftshift and keeps it on the device.
Membership is the reference's by construction; about a quarter of the positions lie outside the unit circle and belong to no bin.

Stated, not reproduced:
  * laplacian_decode's TF.resize(BILINEAR) is PARITY-UNPINNED against torchvision, as composition.py states; upsampling is pinned against
    torch's own F.interpolate (bilinear, align_corners=False), which is what torchvision calls and what td_spectrum_decode evaluates per pixel.
  * A plane whose std is 0 makes the reference divide by zero (250 / std); so does calculate_beauty_score here.
  * The shuffle, tqdm, the plots and the HDF5 file of assign_beauty_scores stay with the caller.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import Library
from ._plumbing import call, engine_for as _engine_for, f32 as _f32, shape as _shape

_P = C.c_void_p
_SIGS = {
    "td_spectrum_last_error": (C.c_char_p, []),
    "td_spectrum_decode": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int]),
    "td_spectrum_fft2": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
    "td_spectrum_radial_bins": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int]),
}
EXPORTS = tuple(_SIGS)
_LIB = Library("libtd_spectrum.so", _SIGS, "td_spectrum_last_error", "td_spectrum")
LIB_PATH, lib, check = _LIB.path, _LIB.lib, _LIB.check

MIN_SIDE = 8                # include/td_spectrum.h TD_SPECTRUM_MIN_SIDE: the transform takes powers of two in 8 .. 4096
MAX_SIDE = 4096             # TD_SPECTRUM_MAX_SIDE
MAX_BATCH = 1024            # TD_SPECTRUM_MAX_BATCH
MAX_BINS = 64               # TD_SPECTRUM_MAX_BINS
NO_BIN = 255                # TD_SPECTRUM_NO_BIN
SCORE_BINS = 4              # beauty_score.py:69
OCEAN_SHARE = 0.99          # beauty_score.py:64
COEFFICIENTS = [0.551959, -1.774091, 3.117426, -1.835090, -1.996856, -0.053519, 0.488380]      # beauty_score.py:79-82
INTERCEPT = 4.44            # beauty_score.py:83
BATCH_PIXELS = 1 << 26      # assign_beauty_scores: pixels of one device call at most (four chunks of 4096 x 4096)


def _dp(t):
    return C.c_void_p(t.data_ptr())


def _on_device(x, what):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise ValueError(f"{what} must be a device tensor (the device forms take no host arrays)")


def _planes(x, what, fft=False):
    """(B, H, W, squeeze) of a plane (H, W) or a batch (B, H, W) within the library's limits; fft=True: of sides the transform takes"""
    s = _shape(x) if hasattr(x, "shape") else tuple(np.shape(x))
    if len(s) not in (2, 3):
        raise ValueError(f"{what} must be (H, W) or (B, H, W), got {tuple(s)}")
    B, H, W = (1, *s) if len(s) == 2 else s
    if fft:
        _check_fft_size(H, W)
    if B < 1 or B > MAX_BATCH or H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"{what} {tuple(s)} outside the library's limit (1 <= B <= {MAX_BATCH}, 1 <= H, W <= {MAX_SIDE})")
    return int(B), int(H), int(W), len(s) == 2


def _check_fft_size(H, W):
    """NotImplementedError unless H and W are each a power of two in 8 .. 4096"""
    for n in (H, W):
        if n < MIN_SIDE or n > MAX_SIDE or n & (n - 1):
            raise NotImplementedError(f"the transform takes sides that are powers of two in {MIN_SIDE} .. {MAX_SIDE}, got {H} x {W}")


def _check_bins(bins):
    bins = int(bins)
    if bins < 1 or bins > MAX_BINS:
        raise ValueError(f"bins must be in 1 .. {MAX_BINS}, got {bins}")
    return bins


def _check_decode(lowfreq, residual):
    B, H, W, squeeze = _planes(residual, "residual")
    b, h, w, sq = _planes(lowfreq, "lowfreq")
    if b != B or sq != squeeze:
        raise ValueError(f"lowfreq is {tuple(np.shape(lowfreq))}, residual is {tuple(np.shape(residual))}: one low band per residual plane")
    if H * W < 2:
        raise ValueError("a plane of one pixel has no standard deviation")
    return B, H, W, h, w, squeeze


# ------------------------------------------------------------------------------------------------------------------------------ the bin map
def bin_edges(bins):
    """(edges, centres) of analyze_terrain_frequency as fp32 tensors: linspace(0, 1, bins + 1) and the midpoints"""
    edges = torch.linspace(0, 1, bins + 1)
    return edges, (edges[:-1] + edges[1:]) / 2


def host_bin_map(H, W, bins):
    """uint8 (H, W) host tensor in torch's UNSHIFTED index order: the bin analyze_terrain_frequency puts every coefficient in, NO_BIN where it
    puts it in none.  The reference's own expressions on the shifted plane (beauty_score.py:28-29, 35, 43), then the inverse of fftshift."""
    y, x = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    dist_from_center = torch.sqrt(x**2 + y**2)
    edges, _ = bin_edges(bins)
    shifted = torch.full((H, W), NO_BIN, dtype=torch.uint8)
    for i in range(bins):
        shifted[(dist_from_center >= edges[i]) & (dist_from_center < edges[i + 1])] = i
    return torch.fft.ifftshift(shifted).contiguous()


_MAPS = {}


def bin_map(H, W, bins, dev):
    """host_bin_map on device `dev`, built once per (H, W, bins, device)"""
    key = (int(H), int(W), int(bins), str(dev))
    if key not in _MAPS:
        _MAPS[key] = host_bin_map(int(H), int(W), int(bins)).to(dev)
    return _MAPS[key]


# ------------------------------------------------------------------------------------------------------------------------------ device forms
@torch.no_grad()
def decode_terrain(lowfreq, residual, *, return_stats=False, engine=None):
    """lowfreq (B, h, w), residual (B, H, W) device tensors (or one plane each) -> the decoded elevation of calculate_beauty_score's head, fp32
    (B, H, W): d = residual + up(lowfreq), sign(d) d^2, negatives clamped to 0.  return_stats=True also returns a dict of device tensors per
    plane: nonpos (int32, the number of pixels <= 0 before the clamp), mean and m2 (float64), std (fp32, unbiased).  No read-back."""
    B, H, W, h, w, squeeze = _check_decode(lowfreq, residual)
    _on_device(lowfreq, "lowfreq")
    _on_device(residual, "residual")
    engine, dev = _engine_for(residual, engine)
    lo, rs = _f32(lowfreq, dev), _f32(residual, dev)
    out = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    nonpos = torch.empty(B, dtype=torch.int32, device=dev)
    mean = torch.empty(B, dtype=torch.float64, device=dev)
    m2 = torch.empty(B, dtype=torch.float64, device=dev)
    std = torch.empty(B, dtype=torch.float32, device=dev)
    call(_LIB, "td_spectrum_decode", engine, dev, _dp(lo), _dp(rs), B, H, W, h, w, _dp(out), _dp(nonpos), _dp(mean), _dp(m2), _dp(std), ordered=True)
    plane = out[0] if squeeze else out
    return (plane, {"nonpos": nonpos, "mean": mean, "m2": m2, "std": std}) if return_stats else plane


@torch.no_grad()
def fft2(x, *, spectrum=True, logabs=False, engine=None):
    """x (B, H, W) real device tensor -> (half spectrum complex64 (B, H, W / 2 + 1) or None, log|F| fp32 (B, H, W) or None): torch.fft.rfft2's
    layout and values, and torch.log(torch.abs(torch.fft.fft2(x))).  A plane (H, W) gives planes."""
    B, H, W, squeeze = _planes(x, "x", fft=True)
    _on_device(x, "x")
    if not (spectrum or logabs):
        raise ValueError("fft2: neither output asked for")
    engine, dev = _engine_for(x, engine)
    a = _f32(x, dev)
    half = torch.empty((B, H, W // 2 + 1, 2), dtype=torch.float32, device=dev) if spectrum else None
    la = torch.empty((B, H, W), dtype=torch.float32, device=dev) if logabs else None
    call(_LIB, "td_spectrum_fft2", engine, dev, _dp(a), B, H, W, _dp(half) if spectrum else None, _dp(la) if logabs else None, ordered=True)
    if spectrum:
        half = torch.view_as_complex(half)
        half = half[0] if squeeze else half
    if logabs and squeeze:
        la = la[0]
    return half, la


@torch.no_grad()
def radial_bins(logabs, bins, *, engine=None):
    """log|F| (B, H, W) device tensor -> (counts int32 (B, bins), means fp32 (B, bins)) device tensors over the rings of bin_map(H, W, bins)"""
    B, H, W, _ = _planes(logabs, "logabs")
    bins = _check_bins(bins)
    _on_device(logabs, "logabs")
    engine, dev = _engine_for(logabs, engine)
    a = _f32(logabs, dev)
    m = bin_map(H, W, bins, dev)
    counts = torch.empty((B, bins), dtype=torch.int32, device=dev)
    means = torch.empty((B, bins), dtype=torch.float32, device=dev)
    call(_LIB, "td_spectrum_radial_bins", engine, dev, _dp(a), _dp(m), B, H, W, bins, _dp(counts), _dp(means), ordered=True)
    return counts, means


@torch.no_grad()
def radial_spectrum(x, bins, *, return_spectrum=False, engine=None):
    """analyze_terrain_frequency on the device: x (B, H, W) or (H, W) real device tensor -> (bin_centres fp32 (bins,) host tensor, bin_means
    fp32 device tensor (B, bins) or (bins,)); return_spectrum=True appends the half spectrum (complex64, torch.fft.rfft2's layout)."""
    B, H, W, squeeze = _planes(x, "x", fft=True)
    bins = _check_bins(bins)
    half, la = fft2(x, spectrum=return_spectrum, logabs=True, engine=engine)
    _, means = radial_bins(la, bins, engine=engine)
    means = means[0] if squeeze else means
    centres = bin_edges(bins)[1]
    return (centres, means, half) if return_spectrum else (centres, means)


@torch.no_grad()
def beauty_features(lowfreq, residual, *, engine=None):
    """lowfreq (B, h, w), residual (B, H, W) -> (bin_means fp32 (B, 4), std fp32 (B,), ocean bool (B,)) device tensors: what
    calculate_beauty_score reads off a chunk.  ocean is the reference's early return: fp32(share of pixels <= 0) > 0.99.  No read-back."""
    B, H, W, h, w, squeeze = _check_decode(lowfreq, residual)
    _check_fft_size(H, W)
    decoded, stats = decode_terrain(lowfreq, residual, return_stats=True, engine=engine)
    _, means = radial_spectrum(decoded.reshape(B, H, W), SCORE_BINS, engine=engine)
    share = stats["nonpos"].to(torch.float32) / torch.full((), float(H * W), dtype=torch.float32, device=means.device)
    return means, stats["std"], share.to(torch.float64) > OCEAN_SHARE


# ------------------------------------------------------------------------------------------------------------------------------ drop-ins
def score_from_features(powers, std):
    """beauty_score.py:71-87 on Python floats: the four bin means and the std, each the float of an fp32 value -> the score"""
    powers, std = [float(p) for p in powers], float(std)
    std_features = [
        np.log(std),          # log of std
        250 / std,            # inverse scaled std
        np.sqrt(std),         # square root of std
    ]
    features = powers + std_features
    score = sum(coef * feat for coef, feat in zip(COEFFICIENTS, features)) + INTERCEPT
    return float(score)


def beauty_class(score):
    """h5_latents_dataset.py:107: the class 0 .. 4 a group's beauty_score puts it in"""
    return max(1, min(5, round(score))) - 1


def _scores(lowfreq, residual, engine):
    """the scores of a batch, one read-back: [float] * B"""
    means, std, ocean = beauty_features(lowfreq, residual, engine=engine)
    host = torch.cat([means.to(torch.float32), std[:, None], ocean[:, None].to(torch.float32)], dim=1).cpu().numpy()
    return [1.0 if row[5] != 0 else score_from_features([v.item() for v in row[:4]], row[4].item()) for row in host]


def analyze_terrain_frequency(heightmap, bins, *, engine=None):
    """Drop-in for beauty_score.py:9-50: heightmap (H, W) array or tensor -> (bin centres, bin means) as lists of floats"""
    B, H, W, squeeze = _planes(heightmap, "heightmap", fft=True)
    if not squeeze:
        raise ValueError(f"heightmap must be (H, W), got {tuple(np.shape(heightmap))}")
    bins = _check_bins(bins)
    engine, dev = _engine_for(heightmap, engine)
    centres, means = radial_spectrum(_f32(heightmap, dev), bins, engine=engine)
    return centres.tolist(), means.cpu().tolist()


def calculate_beauty_score(lowfreq, residual, *, engine=None):
    """Drop-in for beauty_score.py:52-87: lowfreq (h, w), residual (H, W) arrays or tensors -> the score as a float; 1.0 when more than 99 % of
    the decoded pixels are <= 0.  One read-back."""
    B, H, W, h, w, squeeze = _check_decode(lowfreq, residual)
    if not squeeze:
        raise ValueError(f"residual must be (H, W), got {tuple(np.shape(residual))}")
    _check_fft_size(H, W)
    engine, dev = _engine_for(residual, engine)
    return _scores(_f32(lowfreq, dev), _f32(residual, dev), engine)[0]


def assign_beauty_scores(groups, *, engine=None):
    """The loop of beauty_score.py:120-130 over any mapping path -> {'lowfreq', 'residual'} shaped like the HDF5 groups: {path: score}, in the
    given order; groups of one shape go through the device together, BATCH_PIXELS pixels per call at most; a NaN score becomes 1.0."""
    paths = list(groups.keys())
    by_shape = {}
    for p in paths:
        g = groups[p]
        by_shape.setdefault((tuple(np.shape(g["lowfreq"])), tuple(np.shape(g["residual"]))), []).append(p)
    found = {}
    for (low_shape, res_shape), members in by_shape.items():
        first = groups[members[0]]
        B, H, W, h, w, squeeze = _check_decode(first["lowfreq"], first["residual"])
        if not squeeze:
            raise ValueError(f"{members[0]}: residual must be (H, W), got {res_shape}")
        _check_fft_size(H, W)
        per_call = max(1, min(MAX_BATCH, BATCH_PIXELS // (H * W)))
        for at in range(0, len(members), per_call):
            batch = members[at:at + per_call]
            eng, dev = _engine_for(first["residual"], engine)
            take = lambda name: torch.stack([_f32(groups[p][name] if torch.is_tensor(groups[p][name]) else groups[p][name][:], dev) for p in batch])
            for p, s in zip(batch, _scores(take("lowfreq"), take("residual"), eng)):
                found[p] = 1.0 if np.isnan(s) else s
    return {p: found[p] for p in paths}
