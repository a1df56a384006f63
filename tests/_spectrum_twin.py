"""NumPy restatement of the spectrum library's fp32 arithmetic (terrain_diffusion_amd/spectrum_csrc/spectrum_kernels.hip, spectrum.hip), held
to the device BIT FOR BIT, and the running bound its coefficients are held to against float64.  The float64 twin of the same library, the
committed cases and the aggregate bounds are in tests/_beauty_twin.py; this file restates the kernels, that one the reference.

The library is built with contraction off and has no floating-point atomic, so every fp32 product and sum rounds once, in an order the sizes
fix: NumPy float32 arrays do the same, operation by operation, and the two can be compared as int32.

  fft2_fp32    the half spectrum (H, W / 2 + 1) as sp_fft_rows_kernel and sp_fft_cols_kernel compute it.  Keep in step with the header comment
               of spectrum_kernels.hip:
                 twiddles   one table exp(-2 pi i k / 4096), k = 0 .. 2047, built on the host: cos and -sin of (2 pi / 4096) k in float64 from
                            the C library (Python's math calls the same one), each rounded once to fp32; entries 0 and 1024 set to (1, 0)
                            and (0, -1) exactly.
                 transform  radix-2 decimation in time: s[bitrev(i)] = in[i]; stage t = 1 .. log2 n joins s[at] and s[at + half],
                            half = 2^(t-1), at = (f >> (t-1) << t) + j, j = f & (half - 1), with w = table[j * (4096 >> t)]:
                                br = b.x * w.x - b.y * w.y,  bi = b.x * w.y + b.y * w.x     (four products, two sums, each rounded)
                                s[at] = (a.x + br, a.y + bi),  s[at + half] = (a.x - br, a.y - bi)
                 row pass   rows 2p and 2p + 1 of a plane are one complex transform z = row(2p) + i row(2p + 1) of length W; with
                            c = s[(W - k) & (W - 1)], k = 0 .. W / 2:
                                row 2p:     ((z.x + c.x) * 0.5, (z.y - c.y) * 0.5)
                                row 2p + 1: ((z.y + c.y) * 0.5, (c.x - z.x) * 0.5)          (the halvings are exact)
                 column pass  the same transform along H of every column of the row pass's output.
  fft2_bound   E[r, k] >= |F_fp32[r, k] - F64[r, k]|, float64: a running error analysis over the same network (below).
  decode_fp32  the fp32 values of sp_decode_kernel: the taps of sp_taps (tests/_dataset_twin.bilinear_taps is that arithmetic in fp32,
               operation by operation: scale = fp32(n_in) / fp32(n_out), src = max(scale * (dst + 0.5) - 0.5, 0), i0 = min(int(src), n_in - 1),
               l1 = src - i0, l0 = 1 - l1), up = wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * d) in that association, d = res + up,
               v = d > 0 ? d * d : (d < 0 ? -(d * d) : d), the count of v <= 0 (a NaN is not counted), out = v < 0 ? 0 : v (so a -0.0 stays).

The bound.  u = 2^-24.  fft2_bound runs the network in float64 with twiddles cos / sin of float64 and carries, per stored value and per
component (real, imaginary), a bound e on |fp32 value - float64 value|.  The inputs are exact (e = 0).  One butterfly, b and w its float64
operands, p = b w, m.x = |b.x w.x| + |b.y w.y|, m.y = |b.x w.y| + |b.y w.x|:
    the incoming bound of b through the product          |w.x| e_b.x + |w.y| e_b.y   (and |w.y| e_b.x + |w.x| e_b.y)
    each term b.x w.x, b.y w.y: its twiddle component    2 u m                       2 roundings per term, at the terms' magnitude
        rounded once, the product rounded once
    the terms' sum, rounded once                         u |p|                       1 rounding at the magnitude of the result
    each output a +- p: the incoming bounds and one sum  e_a + e_p + u |a +- p|      1 rounding
so e_p = (through the product) + 2 u m + u |p|, and each output adds u of its own magnitude: per component two roundings on every term of
the product, one on their sum, one on the output sum.  Where the table entry is exact -- (1, 0) and (0, -1), j = 0 and j = half / 2 -- the
twiddle has no rounding and the products by 0 and +-1 and their sum are exact: only the output sums count.  The split adds one rounding per
component (the sum; the halving is exact):
(e_z + e_c + u |z +- c|) / 2.  The column pass starts from the row pass's bounds.  At the end E = sqrt(e.x^2 + e.y^2) * SECOND_ORDER: the
magnitudes above are the float64 network's where the kernel's own differ from them by e, so each stage under-counts by at most 5 u e, which
over 24 stages is 2^-17 of E, far inside the 2^-10 the other bounds in the twins allow for second-order terms.  Last, the float64 side's
own error: np.fft.fft2 and the float64 network are each a tree of log2(H W) levels over the samples, at most 8 roundings a level at a magnitude
of at most sum |x|: 16 log2(H W) 2^-53 sum |x| is added, 2^-29 of E's own scale.  Nothing here is tuned: FFT_TERM_ROUNDINGS and the 1 per sum
are the counts above.
"""
import math

import numpy as np

import _beauty_twin as bt
import _dataset_twin as dtwin

U = 2.0 ** -24
F = np.float32
SECOND_ORDER = 1.0 + 2.0 ** -10
MAX_N = 4096                        # spectrum_kernels.hip SP_MAX_N
FFT_TERM_ROUNDINGS = 2              # per term b.x w.x, b.y w.y of a product component: the twiddle component's and the product's
F64_ROUNDINGS = 16                  # per level of the float64 side: 8 for np.fft.fft2, 8 for the float64 network, at sum |x|


# ------------------------------------------------------------------------------------------------------------------------------ tables
def twiddles():
    """fp32 (2048, 2): exp(-2 pi i k / 4096) as spectrum.hip's twiddles() builds it"""
    step = 2.0 * 3.14159265358979323846 / float(MAX_N)
    t = np.array([(math.cos(step * k), -math.sin(step * k)) for k in range(MAX_N // 2)], np.float64).astype(F)
    t[0] = (1.0, 0.0)
    t[MAX_N // 4] = (0.0, -1.0)
    return t


TW = twiddles()


def bits_of(n):
    b = int(n).bit_length() - 1
    if n != 1 << b or not 3 <= b <= 12:
        raise ValueError(f"a side must be a power of two in 8 .. 4096, got {n}")
    return b


def bitrev(n):
    """int64 (n,): sp_bitrev(i, log2 n)"""
    b, i = bits_of(n), np.arange(n)
    r = np.zeros(n, np.int64)
    for k in range(b):
        r |= ((i >> k) & 1) << (b - 1 - k)
    return r


# ------------------------------------------------------------------------------------------------------------------------------ fp32
def fft_axis_fp32(re, im, twiddle_index=None, table=None):
    """sp_fft_lds on fp32 (T, n) real and imaginary parts: T transforms of length n along the last axis, natural order in and out.
    twiddle_index(t, idx) -> idx and table let a test seed a wrong table index or entry (tests/test_spectrum_ops_cpu.py); None is the kernel."""
    table = TW if table is None else table
    T, n = re.shape
    bits, rev = bits_of(n), bitrev(n)
    sr, si = np.empty((T, n), F), np.empty((T, n), F)
    sr[:, rev], si[:, rev] = re, im
    for t in range(1, bits + 1):
        half = 1 << (t - 1)
        idx = np.arange(half) * (MAX_N >> t)
        if twiddle_index is not None:
            idx = twiddle_index(t, idx)
        wx, wy = table[idx, 0], table[idx, 1]
        vr, vi = sr.reshape(T, n >> t, 2, half), si.reshape(T, n >> t, 2, half)
        ax, ay, bx, by = vr[:, :, 0], vi[:, :, 0], vr[:, :, 1], vi[:, :, 1]
        br = bx * wx - by * wy
        bi = bx * wy + by * wx
        lo_r, lo_i, hi_r, hi_i = ax + br, ay + bi, ax - br, ay - bi
        vr[:, :, 0], vi[:, :, 0], vr[:, :, 1], vi[:, :, 1] = lo_r, lo_i, hi_r, hi_i
    assert sr.dtype == F and si.dtype == F
    return sr, si


def rows_fp32(x, twiddle_index=None, table=None):
    """sp_fft_rows_kernel: fp32 (H, W) -> (re, im) fp32 (H, W / 2 + 1), the half spectrum of every row"""
    x = np.ascontiguousarray(x, F)
    H, W = x.shape
    zr, zi = fft_axis_fp32(x[0::2], x[1::2], twiddle_index, table)
    k = np.arange(W // 2 + 1)
    c = (W - k) & (W - 1)
    half = F(0.5)
    re, im = np.empty((H, W // 2 + 1), F), np.empty((H, W // 2 + 1), F)
    re[0::2], im[0::2] = (zr[:, k] + zr[:, c]) * half, (zi[:, k] - zi[:, c]) * half
    re[1::2], im[1::2] = (zi[:, k] + zi[:, c]) * half, (zr[:, c] - zr[:, k]) * half
    return re, im


def cols_fp32(re, im, twiddle_index=None, table=None):
    """sp_fft_cols_kernel: the transform along H of every column of the row spectra"""
    fr, fi = fft_axis_fp32(np.ascontiguousarray(re.T), np.ascontiguousarray(im.T), twiddle_index, table)
    return np.ascontiguousarray(fr.T), np.ascontiguousarray(fi.T)


def as_complex(re, im):
    """complex64 (H, Wh) holding exactly the given fp32 parts"""
    out = np.empty(re.shape + (2,), F)
    out[..., 0], out[..., 1] = re, im
    return out.view(np.complex64)[..., 0]


def fft2_fp32(x):
    """complex64 (H, W / 2 + 1) (or (B, ...) of a batch): td_spectrum_fft2's half spectrum, every bit"""
    x = np.asarray(x, F)
    if x.ndim == 3:
        return np.stack([fft2_fp32(p) for p in x])
    return as_complex(*cols_fp32(*rows_fp32(x)))


def int_view(z):
    """int32 (..., 2) of a complex64 array: what the bit comparison compares"""
    return np.ascontiguousarray(z, np.complex64).view(F).reshape(z.shape + (2,)).view(np.int32)


def ulp_distance(a, b):
    """int64: the number of fp32 values between two fp32 arrays, position by position (the ordered-integer distance)"""
    def ordered(v):
        i = np.ascontiguousarray(v, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


# ------------------------------------------------------------------------------------------------------------------------------ the bound
def _fft_axis_bound(vr, vi, er, ei):
    """the float64 network on (T, n) with the running bounds (module docstring): (vr, vi, er, ei) in natural order"""
    T, n = vr.shape
    bits, rev = bits_of(n), bitrev(n)
    out = []
    for a in (vr, vi, er, ei):
        s = np.empty((T, n), np.float64)
        s[:, rev] = a
        out.append(s)
    sr, si, ser, sei = out
    for t in range(1, bits + 1):
        half = 1 << (t - 1)
        j = np.arange(half)
        ang = -2.0 * np.pi * j / float(1 << t)
        wx, wy = np.cos(ang), np.sin(ang)
        exact = (j * (MAX_N >> t)) % (MAX_N // 4) == 0      # table entries 0 and 1024: (1, 0) and (0, -1)
        wx[exact], wy[exact] = np.round(wx[exact]), np.round(wy[exact])
        awx, awy = np.abs(wx), np.abs(wy)
        rnd = np.where(exact, 0.0, 1.0)
        shape = (T, n >> t, 2, half)
        vr_, vi_, er_, ei_ = (a.reshape(shape) for a in (sr, si, ser, sei))
        ax, ay, bx, by = vr_[:, :, 0], vi_[:, :, 0], vr_[:, :, 1], vi_[:, :, 1]
        eax, eay, ebx, eby = er_[:, :, 0], ei_[:, :, 0], er_[:, :, 1], ei_[:, :, 1]
        px, py = bx * wx - by * wy, bx * wy + by * wx
        mx, my = np.abs(bx) * awx + np.abs(by) * awy, np.abs(bx) * awy + np.abs(by) * awx
        epx = awx * ebx + awy * eby + rnd * U * (FFT_TERM_ROUNDINGS * mx + np.abs(px))
        epy = awy * ebx + awx * eby + rnd * U * (FFT_TERM_ROUNDINGS * my + np.abs(py))
        lo_r, lo_i, hi_r, hi_i = ax + px, ay + py, ax - px, ay - py
        e_lo_r, e_lo_i = eax + epx + U * np.abs(lo_r), eay + epy + U * np.abs(lo_i)
        e_hi_r, e_hi_i = eax + epx + U * np.abs(hi_r), eay + epy + U * np.abs(hi_i)
        vr_[:, :, 0], vi_[:, :, 0], vr_[:, :, 1], vi_[:, :, 1] = lo_r, lo_i, hi_r, hi_i
        er_[:, :, 0], ei_[:, :, 0], er_[:, :, 1], ei_[:, :, 1] = e_lo_r, e_lo_i, e_hi_r, e_hi_i
    return sr, si, ser, sei


def fft2_network(x):
    """(F complex128 (H, W / 2 + 1), E float64 (H, W / 2 + 1)): the float64 run of the kernels' network and the bound on
    |F_fp32 - F64| per coefficient, as the module docstring derives it"""
    x = np.asarray(x, F).astype(np.float64)
    H, W = x.shape
    zero = np.zeros((H // 2, W))
    zr, zi, er, ei = _fft_axis_bound(x[0::2], x[1::2], zero, zero)
    k = np.arange(W // 2 + 1)
    c = (W - k) & (W - 1)
    Wh = W // 2 + 1
    re, im, ere, eim = (np.empty((H, Wh)) for _ in range(4))
    sums = ((0, zr[:, k] + zr[:, c], er, re, ere), (0, zi[:, k] - zi[:, c], ei, im, eim),
            (1, zi[:, k] + zi[:, c], ei, re, ere), (1, zr[:, c] - zr[:, k], er, im, eim))
    for row, s, e, val, err in sums:
        val[row::2] = 0.5 * s
        err[row::2] = 0.5 * (e[:, k] + e[:, c] + U * np.abs(s))
    fr, fi, efr, efi = _fft_axis_bound(*(np.ascontiguousarray(a.T) for a in (re, im, ere, eim)))
    E = np.sqrt(efr * efr + efi * efi).T * SECOND_ORDER + F64_ROUNDINGS * np.log2(H * W) * 2.0 ** -53 * np.abs(x).sum()
    return (fr + 1j * fi).T, E


def fft2_bound(x):
    """float64 (H, W / 2 + 1): E[r, k] >= |fft2_fp32(x)[r, k] - np.fft.fft2(x)[r, k]|"""
    return fft2_network(x)[1]


# ------------------------------------------------------------------------------------------------------------------------------ decode
def decode_fp32(low, res):
    """(out fp32 (H, W), nonpos int) of sp_decode_kernel on fp32 low (h, w) and res (H, W): every bit"""
    low, res = np.ascontiguousarray(low, F), np.ascontiguousarray(res, F)
    (h, w), (H, W) = low.shape, res.shape
    i0, i1, wy0, wy1 = dtwin.bilinear_taps(h, H)
    j0, j1, wx0, wx1 = dtwin.bilinear_taps(w, W)
    assert all(a.dtype == F for a in (wy0, wy1, wx0, wx1))
    wy0, wy1, wx0, wx1 = wy0[:, None], wy1[:, None], wx0[None], wx1[None]
    top, bot = low[i0], low[i1]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        up = wy0 * (wx0 * top[:, j0] + wx1 * top[:, j1]) + wy1 * (wx0 * bot[:, j0] + wx1 * bot[:, j1])
        d = res + up
        sq = d * d
        v = np.where(d > 0, sq, np.where(d < 0, -sq, d))
        nonpos = int((v <= 0).sum())
        out = np.where(v < 0, F(0), v)
    assert out.dtype == F
    return out, nonpos


# ------------------------------------------------------------------------------------------------------------------------------ planes
SIDES = tuple(1 << b for b in range(3, 13))
_KINDS = ("noise", "terrain", "cosine")


def new_planes():
    """{name: fp32 (H, W) or (B, H, W)}: the shapes beyond the committed cases (tests/_beauty_twin.SPECTRUM_CASES).  Every side 8 .. 4096 on each
    axis in thin shapes; 512 and 2048, which no committed case transforms, on both; batches whose column tiles cross a plane stride (two-column
    tiles at H = 4096, a last tile of one column at W = 8 and of 1 of 16 at W = 32) with unlike planes."""
    out = {}
    for i, n in enumerate(SIDES):
        out[f"thin_{n}x8"] = bt.plane(_KINDS[i % 3], n, 8, 100 + i)
        out[f"thin_8x{n}"] = bt.plane(_KINDS[(i + 1) % 3], 8, n, 120 + i)
    out["noise_512x16"] = bt.plane("noise", 512, 16, 140)
    out["terrain_16x2048"] = bt.plane("terrain", 16, 2048, 141)
    out["noise_2048x16"] = bt.plane("noise", 2048, 16, 142)
    out["batch3_4096x8"] = np.stack([bt.plane(k, 4096, 8, 150 + i) for i, k in enumerate(("noise", "terrain", "cosine"))])
    out["batch2_8x4096"] = np.stack([bt.plane(k, 8, 4096, 160 + i) for i, k in enumerate(("terrain", "noise"))])
    out["batch5_16x32"] = np.stack([bt.plane(k, 16, 32, 170 + i) for i, k in enumerate(("impulse", "cosine", "noise", "terrain", "flat"))])
    return out


def all_planes():
    """the committed spectrum cases and new_planes(), in one dict"""
    out = dict(bt.spectrum_planes())
    out.update(new_planes())
    return out


def single_planes(planes):
    """[(name, fp32 (H, W))]: every plane of the dict, the members of a batch as name[i]"""
    return [item for n, x in planes.items() for item in ([(n, x)] if x.ndim == 2 else [(f"{n}[{i}]", p) for i, p in enumerate(x)])]


# (name, (h, w), (H, W)): the score cases of tests/_beauty_twin.py come first in decode_cases()
DECODE_SHAPES = (("up_5x7_from_2x3", (2, 3), (5, 7)), ("up_1x2_from_1x1", (1, 1), (1, 2)), ("up_7x7_from_3x3", (3, 3), (7, 7)),
                 ("identity_300x257", (300, 257), (300, 257)), ("up_64x64_from_1x8", (1, 8), (64, 64)), ("up_64x64_from_8x1", (8, 1), (64, 64)))


def decode_cases():
    """{name: (low fp32 (h, w), res fp32 (H, W))}: the score cases, then DECODE_SHAPES with values in +-40 and the edge values placed by hand:
    -0.0 in both inputs, a residual that cancels the upsampled value exactly, a NaN in res and a NaN in low"""
    out = {c[0]: bt.score_inputs(c[0]) for c in bt.SCORE_CASES}
    for i, (name, (h, w), (H, W)) in enumerate(DECODE_SHAPES):
        low = ((bt.uniform(200 + i, h * w).reshape(h, w) - 0.5) * 80.0).astype(F)
        res = ((bt.uniform(220 + i, H * W).reshape(H, W) - 0.5) * 80.0).astype(F)
        out[name] = (low, res)
    low, res = out["identity_300x257"]                    # scale 1: the taps are the pixel itself with weights 1 and 0
    res[10, 20:40] = -low[10, 20:40]                      # d = 0.0 exactly
    low[200, 100:104] = F(-0.0)
    res[200, 101:103] = F(-0.0)                           # d = -0.0
    res[299, 256] = np.nan
    low[0, 0] = np.nan
    low, res = out["up_64x64_from_1x8"]
    low[0, 3:5] = F(-0.0)
    res[:, 28:36] = F(-0.0)                               # between two taps of -0.0 every product and sum is -0.0
    low[0, 7] = np.nan
    res[5, 9] = np.nan
    low, res = out["up_5x7_from_2x3"]
    low[:, 0] = 0.0
    res[:, 0] = 0.0                                       # d = 0.0 from zeros
    res[4, 6] = np.nan
    out["up_7x7_from_3x3"][0][1, 1] = np.nan              # the centre tap: a NaN that reaches a block of outputs through 0-weight-free taps
    out["up_1x2_from_1x1"] = (np.array([[2.5]], F), np.array([[-2.5, np.nan]], F))
    return out
