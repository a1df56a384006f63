"""Float64 / NumPy twin of the spectrum library (include/td_spectrum.h, terrain_diffusion_amd/beauty.py): the reference's beauty score
(terrain_diffusion/data/preprocessing/beauty_score.py) stated independently of the kernels, the committed cases, and the bounds the tests hold
the device to.

  decode_ref      residual + up(lowfreq) in float64 with the fp32 taps of torch's upsample_bilinear2d (tests/_dataset_twin.py), sign(d) d^2, the
                  clamp; with the bound per element.
  spectrum        np.fft.fft2 of the fp32 plane in float64.
  bin_masks       the reference's ring membership, its own expressions in torch fp32 on the SHIFTED plane (the twin shifts the spectrum as the
                  reference does, where the package un-shifts the map).
  bin_means       the mean of log|F| per ring in float64; an empty ring gives 0.0.
  score           the seven features and the linear model in float64.

PARITY-UNPINNED, as terrain_diffusion_amd/composition.py states: torchvision is not installed here, laplacian_decode's TF.resize(BILINEAR) is
restated as torch's F.interpolate(bilinear, align_corners=False), the call torchvision makes.

Bounds ("Beauty scores"), u = 2^-24, rho the relative L2 error of the reference's own fp32 torch.fft.fft2 against this float64 one
(recorded per case in tests/golden/beauty.npz):
  spectrum   ||F_gpu - F64||_2 / ||F64||_2 <= 4 rho: twice the butterfly stages of the reference's mixed-radix plan at most, fp32 twiddles.
  bin mean   |gpu - D64| <= (4 rho ||x||_2 + ||dx||_2) mean_{k in bin}(1 / |F64_k|) + 2 ulp32(|D64|): the spectrum bound spread evenly over the
             coefficients (per coefficient 4 rho ||F64||_2 / sqrt(N) = 4 rho ||x||_2) and pushed through log, whose derivative is 1 / |F|; then
             log's ulp and the final rounding.  dx is the bound on the input plane itself (zero for a plane given exactly, the decode's bound
             where the plane comes from td_spectrum_decode): a perturbation dx of the plane moves the spectrum by ||dx||_2 per coefficient in
             the same even spread.  The fixtures keep min |F64_k| >= 64 rho ||x||_2, so the first-order bound holds.
  decode     d within E of _dataset_twin.residual_ref's count (four roundings per tap, one for the sum: the same expression with a + for the -);
             v = sign(d) fp32(d^2) within 2 |d| E + E^2 + u d^2 (1 + 2^-10).
  std        within 1 ulp32 of the float64 std of the same plane; against this twin's own plane additionally ||dv||_2 / sqrt(N - 1).
  score      sum |coef_i| bound_i with the std terms differentiated: |c4| / s + 250 |c5| / s^2 + |c6| / (2 sqrt s) per unit of std error.
Nothing here is tuned.
"""
import zlib

import numpy as np

import _dataset_twin as dtwin

U = 2.0 ** -24
F = np.float32
SECOND_ORDER = 1.0 + 2.0 ** -10
COEFFICIENTS = [0.551959, -1.774091, 3.117426, -1.835090, -1.996856, -0.053519, 0.488380]
INTERCEPT = 4.44
SPECTRUM_FACTOR = 4.0               # the issue's factor on rho
FLOOR_FACTOR = 64.0                 # min |F64_k| >= 64 rho ||x||_2 in every fixture but the flat plane


# ------------------------------------------------------------------------------------------------------------------------------ inputs
def uniform(seed, n):
    """n float64 in [0, 1) from splitmix64 of seed + index: the same on every NumPy"""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x632BE59BD9B4E019)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def terrain(H, W, seed, land=0.7):
    """float64 (H, W) metres: a steep spectrum (white noise summed along both axes), a floor of white noise, shifted so that a share `land`
    of it lies above 0"""
    u = uniform(seed, H * W).reshape(H, W) - 0.5
    t = np.cumsum(np.cumsum(u, 0), 1)
    t = (t - t.mean()) / t.std() * 600.0 + 40.0 * (uniform(seed + 1000, H * W).reshape(H, W) - 0.5)
    return t - np.quantile(t, 1.0 - land)


def plane(kind, H, W, seed):
    """one fp32 input plane of the spectrum cases"""
    if kind == "impulse":
        x = np.zeros((H, W), F)
        x[(3 * H) // 8 | 1, (5 * W) // 8 | 1] = 1.0               # odd offsets: every twiddle of both axes appears
        return x
    if kind == "cosine":                                # one mode (u, v) of amplitude 1 over a unit impulse: the impulse is the floor of |F|
        r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        x = np.cos(2.0 * np.pi * (2.0 * r / H + 3.0 * c / W) + 0.7)
        x[1, 2] += 1.0
        return x.astype(F)
    if kind == "noise":
        return ((uniform(seed, H * W).reshape(H, W) - 0.5) * 200.0).astype(F)
    if kind == "terrain":
        return np.maximum(terrain(H, W, seed), 0.0).astype(F)
    if kind == "flat":
        return np.full((H, W), 7.5, F)
    raise ValueError(kind)


# (name, kind, H, W, seed); batch3 is three unlike planes of one shape
SPECTRUM_CASES = (
    ("impulse_8", "impulse", 8, 8, 0), ("cosine_16", "cosine", 16, 16, 0), ("noise_64", "noise", 64, 64, 11), ("terrain_256", "terrain", 256, 256, 12),
    ("impulse_8x64", "impulse", 8, 64, 0), ("cosine_128x16", "cosine", 128, 16, 0), ("noise_4096x8", "noise", 4096, 8, 13),
    ("noise_8x4096", "noise", 8, 4096, 14), ("terrain_1024", "terrain", 1024, 1024, 15), ("flat_16", "flat", 16, 16, 0),
    ("batch3_a", "impulse", 32, 64, 0), ("batch3_b", "noise", 32, 64, 16), ("batch3_c", "terrain", 32, 64, 17),
)
BATCH3 = ("batch3_a", "batch3_b", "batch3_c")
BINS = (4, 7)                                           # the score's four rings, and a count that does not divide the radius evenly

# (name, S, ratio, seed, land): lowfreq (S / ratio)^2, residual S^2 in the signed-square-root domain
SCORE_CASES = (
    ("score_64", 64, 8, 21, 0.7), ("score_256", 256, 8, 22, 0.55), ("score_128_r4", 128, 4, 23, 0.9), ("ocean995_64", 64, 8, 24, 0.0045),
    ("ocean98_64", 64, 8, 25, 0.0202),
)


def spectrum_planes():
    return {name: plane(kind, H, W, seed) for name, kind, H, W, seed in SPECTRUM_CASES}


def score_inputs(name):
    """(lowfreq (S / ratio, S / ratio), residual (S, S)) fp32 of a score case: the signed square root of a terrain, its block mean, and what
    remains after the bilinear upsampling of that mean"""
    _, S, ratio, seed, land = next(c for c in SCORE_CASES if c[0] == name)
    t = terrain(S, S, seed, land)
    s = np.sign(t) * np.sqrt(np.abs(t))
    low = s.reshape(S // ratio, ratio, S // ratio, ratio).mean((1, 3)).astype(F)
    up, _ = dtwin.upsample_ref(low, S, S)
    return low, (s - up).astype(F)


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


# ------------------------------------------------------------------------------------------------------------------------------ decode
def decode_ref(lowfreq, residual):
    """float64 (d, E, v, Ev, out): d = residual + up(lowfreq) and its bound, v = sign(d) d^2 and its bound, out = max(v, 0)"""
    res = np.asarray(residual, F).astype(np.float64)
    up, M = dtwin.upsample_ref(lowfreq, *res.shape)
    d = res + up
    E = (dtwin.RESIDUAL_ROUNDINGS * U * M + U * np.abs(d)) * SECOND_ORDER
    v = np.sign(d) * d * d
    Ev = 2.0 * np.abs(d) * E + E * E + U * d * d * SECOND_ORDER
    return d, E, v, Ev, np.maximum(v, 0.0)


def std_ref(x):
    x = np.asarray(x, np.float64)
    return float(np.sqrt(((x - x.mean()) ** 2).sum() / (x.size - 1)))


def ulp32(v):
    v = np.abs(np.asarray(v, np.float64)).astype(F)
    return (np.nextafter(v, F(np.inf)) - v).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------------ spectrum
def spectrum(x):
    return np.fft.fft2(np.asarray(x, F).astype(np.float64))


def half_of(Fk):
    return Fk[:, :Fk.shape[1] // 2 + 1]


def bin_masks(H, W, bins):
    """[bool (H, W)] * bins on the SHIFTED plane: beauty_score.py:28-29, 35, 43 in torch fp32"""
    import torch
    y, x = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    dist_from_center = torch.sqrt(x**2 + y**2)
    bin_edges = torch.linspace(0, 1, bins + 1)
    return [((dist_from_center >= bin_edges[i]) & (dist_from_center < bin_edges[i + 1])).numpy() for i in range(bins)]


def bin_means(x, bins, dx_norm=0.0, rho=0.0):
    """(counts int64 (bins,), D64 float64 (bins,), bound float64 (bins,)) of the fp32 plane x; see the module docstring for the bound"""
    x = np.asarray(x, F).astype(np.float64)
    mag = np.abs(np.fft.fftshift(np.fft.fft2(x)))
    with np.errstate(divide="ignore"):
        logabs = np.log(mag)
    norm = float(np.sqrt((x * x).sum()))
    counts, means, bounds = [], [], []
    for mask in bin_masks(*x.shape, bins):
        n = int(mask.sum())
        counts.append(n)
        if n == 0:
            means.append(0.0)
            bounds.append(0.0)
            continue
        m = float(logabs[mask].mean())
        with np.errstate(divide="ignore"):
            spread = float((1.0 / mag[mask]).mean())
        means.append(m)
        bounds.append((SPECTRUM_FACTOR * rho * norm + dx_norm) * spread + 2.0 * float(ulp32(m)) if np.isfinite(m) else 0.0)
    return np.array(counts, np.int64), np.array(means), np.array(bounds)


def min_magnitude(x):
    x = np.asarray(x, F).astype(np.float64)
    return float(np.abs(np.fft.fft2(x)).min()), float(np.sqrt((x * x).sum()))


# ------------------------------------------------------------------------------------------------------------------------------ score
def score_of(powers, std):
    f = [float(p) for p in powers] + [float(np.log(std)), 250.0 / std, float(np.sqrt(std))]
    return float(sum(c * v for c, v in zip(COEFFICIENTS, f)) + INTERCEPT)


def score_bound(power_bounds, std, std_bound):
    c = [abs(v) for v in COEFFICIENTS]
    b = sum(ci * bi for ci, bi in zip(c[:4], power_bounds))
    return float(b + std_bound * (c[4] / std + 250.0 * c[5] / std ** 2 + c[6] / (2.0 * np.sqrt(std))))


def score_ref(lowfreq, residual, rho):
    """dict of a score case in float64: the share of pixels <= 0, the four ring means with their bounds, std with its bound, the score with its
    bound (against a device that decodes within Ev, transforms within 4 rho, sums in float64 and rounds each feature once)"""
    d, E, v, Ev, out = decode_ref(lowfreq, residual)
    x32 = out.astype(F)
    dx = float(np.sqrt((Ev * Ev).sum()))
    counts, powers, pb = bin_means(x32, 4, dx_norm=dx, rho=rho)
    std = std_ref(out)
    sb = float(ulp32(std)) + dx / np.sqrt(out.size - 1.0)
    return {"nonpos": int((v <= 0).sum()), "share": float((v <= 0).mean()), "powers": powers, "power_bounds": pb, "std": std, "std_bound": sb,
            "score": score_of(powers, std), "score_bound": score_bound(pb, std, sb)}
