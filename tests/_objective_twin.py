"""Host restatement ("twin") of libtd_objective.so (include/td_objective.h, objective_csrc/objective_kernels.hip) and the rules its values are
held to.  Nothing here imports `terrain_diffusion_amd`.

Two forms, written from the header's definitions:
  NumPy fp32, bit for bit what the kernels store   add_noise32 (entry point 2), terrain_u8 (entry point 6): every product, sum and division
                  is one fp32 operation in the reference's order, which is what an element kernel built without contraction computes;
  float64         levels64 (1), logvar64 (3), sqerr64 (4), loss64 (5): the exact definition, with math.fsum for every sum.  levels64 rounds t to
                  fp32 FIRST and takes cos, sin and x_lv of that t32, as the header states.

The criterion against the reference's recorded values (tests/golden/objective.npz: DiffusionTrainer.train_step itself, the nested calc_loss of
noise_loss_curve.py, _normalize_and_process_terrain), as tests/_train_data_twin.py states it: the fixture stores a float64 companion F of every
recorded fp32 quantity R and e_ref = |R - F|, the reference's own error.  A twin value T that restates F differs from R by at most
e_ref + ulp32(R) (T rounded once).  Every LATER operation f is the same rounded fp32 operation on both sides, and
|fl(f(a)) - fl(f(b))| <= L |a - b| + ulp(result) for an L-Lipschitz f, rounding being monotone; equal inputs give equal results (d = 0 stays 0):
  noise_carry   |dc|, |ds| of the table through x = (c img + s nz) / sd and v = c nz - s img;
  sq_carry      |dv| through S = sum d^2: sum (2 |d| dv + dv^2), d in fp32 on both sides (+ ulp32(d) where dv > 0);
  loss_carry    |dS| and |dlv| through each form's formula, by its partial derivatives taken at the worse end of the interval.
Nothing in a bound is measured on the code under test.

The logvar head's bound E (logvar64) is the one tests/_emb_twin.py derives for a 'float' input row: the dot product of one wave,
(ceil(K / 64) + 7) u sum |w_k p_k| (lane l's sequential chain of ceil(K / 64) products, the 6-level xor butterfly, the product rounding), and the
cos feature, (2 TRIG_ULP + 1) u |p_k| carried through |w_k|; TRIG_ULP = 4 is that file's constant, the OpenCL full-profile limit -- a
specification, not a measurement.

VARIANTS names deliberately WRONG restatements; tests/test_objective_cpu.py must see each fail on the committed inputs.
"""
import math

import numpy as np

F = np.float32
D = np.float64
U = 2.0 ** -24
TRIG_ULP = 4.0          # tests/_emb_twin.py TRIG_ULP (asserted equal by the tests)
CAP = 2.0 ** -14        # tests/_emb_twin.py CAP
LEVEL_COLS = ("sigma", "t", "cos", "sin", "xlv", "std")
VARIANTS = ("cos_sin_swapped", "noise_unscaled", "v_sign", "biased_std", "mean_nhw", "logvar_not_added", "group_weighted", "range_not_floored")


def ulp32(x):
    """unit in the last place of fp32 in the binade the float64 x lies in (the subnormal spacing below 2^-126)"""
    a = np.abs(np.asarray(x, dtype=D))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.where(a > 0, np.maximum(e, -126.0), -126.0)
    return np.where(np.isfinite(a), 2.0 ** (e - 23.0), np.inf)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def within(got, want, tol):
    """|got - want| <= tol everywhere, NaN matching NaN"""
    got, want, tol = np.asarray(got, dtype=D), np.asarray(want, dtype=D), np.asarray(tol, dtype=D)
    both = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - want) <= tol
    return bool(np.all(ok | both))


def _f32(x):
    """the float64 value of the fp32 a Python scalar is cast to"""
    return float(F(x))


# ------------------------------------------------------------------------------------------------------------------------------ levels
def std64(images, channels, variant=None):
    """torch.std (unbiased) of images[n, channels] per item in float64: the mean, then the centred squares; one value gives NaN"""
    img = np.asarray(images, dtype=F)
    out = np.empty(img.shape[0], dtype=D)
    for n in range(img.shape[0]):
        v = [float(a) for a in img[n, list(channels)].reshape(-1)]
        M = len(v)
        mean = math.fsum(v) / M
        q = math.fsum((a - mean) * (a - mean) for a in v)
        den = M if variant == "biased_std" else M - 1
        out[n] = math.sqrt(q / den) if den > 0 and not math.isnan(q) else float("nan")
    return out


def levels64(values, mode, sigma_data, P_mean=0.0, P_std=1.0, images=None, channels=None, eps=0.05, variant=None):
    """dict of float64 columns sigma, t, cos, sin, xlv, std (t the float64 value of t32) and `table`, the (N, 6) fp32 table rounded once"""
    a = np.asarray(values, dtype=F).astype(D).reshape(-1)
    sd = _f32(sigma_data)
    std = np.zeros_like(a)
    with np.errstate(all="ignore"):
        if mode == "t":
            t32 = np.asarray(values, dtype=F).reshape(-1)
            sigma = np.tan(t32.astype(D)) * sd
        else:
            sigma = np.exp(a * _f32(P_std) + _f32(P_mean)) if mode == "draw" else a.copy()
            if mode == "draw" and channels is not None:
                std = std64(images, channels, variant)
                r = std / sd
                sigma = sigma * np.where(np.isnan(r), r, np.maximum(r, _f32(eps)))
            t32 = np.arctan(sigma / sd).astype(F)
        t = t32.astype(D)
        cols = dict(sigma=sigma, t=t, cos=np.cos(t), sin=np.sin(t), xlv=np.log(np.tan(t) / 8.0), std=std)
        cols["table"] = np.stack([cols[k] for k in LEVEL_COLS], axis=1).astype(F)
    return cols


# ------------------------------------------------------------------------------------------------------------------------------ noise
def add_noise32(images, noise, table, sigma_data, cond=None, variant=None):
    """(x, v) fp32, bit for bit the kernel's: nz = noise sd; x = (c img + s nz) / sd followed by cond; v = c nz - s img"""
    img, nz0, table = np.asarray(images, dtype=F), np.asarray(noise, dtype=F), np.asarray(table, dtype=F)
    sd = F(sigma_data)
    c, s = table[:, 2].reshape(-1, 1, 1, 1), table[:, 3].reshape(-1, 1, 1, 1)
    if variant == "cos_sin_swapped":
        c, s = s, c
    with np.errstate(all="ignore"):
        nz = nz0 if variant == "noise_unscaled" else nz0 * sd
        a = c * img
        b = s * nz
        xt = a + b
        x = xt / sd
        p = c * nz
        q = s * img
        v = q - p if variant == "v_sign" else p - q
    if cond is not None:
        x = np.concatenate([x, np.asarray(cond, dtype=F)], axis=1)
    return x.astype(F), v.astype(F)


def _step(d, result):
    """an error d carried through one rounded operation: + one ulp of the result where d > 0"""
    return np.where(d > 0, d + ulp32(result), 0.0)


def noise_carry(dc, ds, images, noise, sigma_data):
    """(bound on |x - x'|, bound on |v - v'|) for the image channels when cos t and sin t differ by at most dc, ds (N) between the two sides"""
    img, nz0 = np.asarray(images, dtype=F), np.asarray(noise, dtype=F)
    sd = F(sigma_data)
    dc, ds = (np.asarray(d, dtype=D).reshape(-1, 1, 1, 1) for d in (dc, ds))
    nz = (nz0 * sd).astype(D)
    img = img.astype(D)
    big = lambda d: np.broadcast_to(d, img.shape)
    c = 1.0                                                   # |cos|, |sin| <= 1: an ulp of a product is at most an ulp of its larger factor
    da = _step(big(dc) * np.abs(img), c * np.abs(img))
    db = _step(big(ds) * np.abs(nz), c * np.abs(nz))
    dxt = _step(da + db, np.abs(img) + np.abs(nz))
    dx = _step(dxt / float(sd), (np.abs(img) + np.abs(nz)) / float(sd))
    dp = _step(big(dc) * np.abs(nz), np.abs(nz))
    dq = _step(big(ds) * np.abs(img), np.abs(img))
    dv = _step(dp + dq, np.abs(img) + np.abs(nz))
    return dx, dv


# ------------------------------------------------------------------------------------------------------------------------------ logvar
def logvar64(xlv, freqs, phases, weight):
    """(logvar (N) float64, its bound E) from the fp32 column x_lv and the FOLDED fp32 weight (K): the argument fl32(fl32(x f) + p) is fp32 and
    exact to restate, the cosine, sqrt2 and the dot product are float64"""
    x, f, p, w = (np.asarray(a, dtype=F).reshape(-1) for a in (xlv, freqs, phases, weight))
    K = f.size
    with np.errstate(all="ignore"):
        y = ((x[:, None] * f[None, :]).astype(F) + p[None, :]).astype(F)
        feat = np.cos(y.astype(D)) * math.sqrt(2.0)
    terms = feat * w.astype(D)[None, :]
    lv = np.array([math.fsum(r) if np.all(np.isfinite(r)) else float("nan") for r in terms])
    E = (math.ceil(K / 64) + 7.0 + 2.0 * TRIG_ULP + 1.0) * U * np.abs(terms).sum(axis=1)
    return lv, E


# ------------------------------------------------------------------------------------------------------------------------------ sqerr, loss
def diff32(model_output, v, sigma_data):
    """d = fl32(fl32(-sd out) - v), as the reference forms pred_v_t - v_t"""
    with np.errstate(all="ignore"):
        pred = (-F(sigma_data)) * np.asarray(model_output, dtype=F)
        return (pred.astype(F) - np.asarray(v, dtype=F)).astype(F)


def sqerr64(model_output, v, sigma_data):
    """S (N, C) float64: the exactly rounded sum of the exact squares of d (a square of an fp32 is exact in float64)"""
    d = diff32(model_output, v, sigma_data).astype(D)
    N, Cn = d.shape[:2]
    S = np.empty((N, Cn), dtype=D)
    for n in range(N):
        for c in range(Cn):
            r = d[n, c].reshape(-1)
            S[n, c] = math.fsum(float(a) * float(a) for a in r) if np.all(np.isfinite(r)) else float(np.sum(r * r))
    return S


def sq_carry(model_output, v, dv, sigma_data):
    """bound on |S - S'| (N, C) when v differs by at most dv elementwise between the two sides"""
    d = np.abs(diff32(model_output, v, sigma_data).astype(D))
    dd = _step(np.asarray(dv, dtype=D), d + np.asarray(dv, dtype=D))
    return (2.0 * d * dd + dd * dd).sum(axis=(2, 3))


def loss64(S, HW, sigma_data, logvar=None, form="weighted", groups=None, variant=None):
    """(per-item losses (N), the scalar) in float64 from S (N, C)"""
    S = np.asarray(S, dtype=D)
    N, Cn = S.shape
    sd2 = _f32(sigma_data) ** 2
    items = np.empty(N, dtype=D)
    for n in range(N):
        if form == "grouped" and variant != "group_weighted":
            c, g = 0, []
            for k in groups:
                g.append(math.fsum(S[n, c:c + k]) / (k * HW) / sd2)
                c += k
            assert c == Cn
            items[n] = math.fsum(g) / len(g)
            continue
        m = math.fsum(S[n]) / ((1 if variant == "mean_nhw" else Cn) * HW)
        if form == "weighted":
            lv = float(logvar[n])
            items[n] = m / (math.exp(lv) * sd2) + (0.0 if variant == "logvar_not_added" else lv)
        else:
            items[n] = m / sd2
    return items, math.fsum(items) / N if np.all(np.isfinite(items)) else float(np.mean(items))


def loss_carry(S, dS, HW, sigma_data, logvar=None, dlv=None, form="weighted", groups=None):
    """bound on the scalar's change when S moves by at most dS (N, C) and logvar by at most dlv (N)"""
    S, dS = np.asarray(S, dtype=D), np.asarray(dS, dtype=D)
    N, Cn = S.shape
    sd2 = _f32(sigma_data) ** 2
    if form == "grouped":
        c, tot = 0, 0.0
        for k in groups:
            tot = tot + dS[:, c:c + k].sum(axis=1) / (k * HW) / sd2
            c += k
        return float(tot.sum() / len(groups) / N)
    dm = dS.sum(axis=1) / (Cn * HW)
    if form == "plain":
        return float(dm.sum() / sd2 / N)
    lv, dlv = np.asarray(logvar, dtype=D), np.asarray(dlv, dtype=D)
    m = (S + dS).sum(axis=1) / (Cn * HW)
    w = np.exp(-(lv - dlv)) / sd2                              # the largest 1 / (exp(lv) sd^2) over the interval
    return float((dm * w + dlv * (m * w + 1.0)).sum() / N)


# ------------------------------------------------------------------------------------------------------------------------------ terrain_u8
def terrain_u8(terrain, variant=None):
    """(uint8 (N, 3 C, H, W), the fp32 values before the clamp and the truncation) in the reference's order of fp32 operations"""
    x = np.asarray(terrain, dtype=F)
    with np.errstate(all="ignore"):
        bad = np.isnan(x).any(axis=(1, 2, 3), keepdims=True)
        lo = np.where(bad, F(np.nan), np.nanmin(np.where(np.isnan(x), F(np.inf), x), axis=(1, 2, 3), keepdims=True)).astype(F)
        hi = np.where(bad, F(np.nan), np.nanmax(np.where(np.isnan(x), F(-np.inf), x), axis=(1, 2, 3), keepdims=True)).astype(F)
        r0 = (hi - lo).astype(F)
        rng = r0 if variant == "range_not_floored" else np.where(np.isnan(r0), r0, np.maximum(r0, F(255.0))).astype(F)
        mid = ((lo + hi).astype(F) / F(2.0)).astype(F)
        pre = ((((x - mid).astype(F) / rng).astype(F) + F(0.5)).astype(F) * F(255.0)).astype(F)
        y = np.where(np.isnan(pre), F(0.0), np.clip(pre, F(0.0), F(255.0)))
    return np.tile(y.astype(np.int32).astype(np.uint8), (1, 3, 1, 1)), pre
