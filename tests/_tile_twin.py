"""Float64 twins of the tiling and composition kernels, their bounds, the committed cases and fp32 CPU emulations.

What is checked.  The kernels between the U-Net and the caller: the overlap blend (`blend_gather_kernel` through td_blend_windows, `regions_gather_kernel` through
td_gather_regions, `blend_normalize_kernel`), the separable resampler (`resample_rows_kernel` / `resample_cols_kernel` through td_resample2d), the elevation finish
(`residual_plus_kernel`, `elev_finish_kernel`), the climate finish (`climate_finish_kernel`) and the guided DDIM step (`ddim_cfg_step_kernel`).  Every case calls the
C entry point on fp32 inputs this file makes; `*_ref` evaluates the same operation in float64 on the stored fp32 operands together with a bound E per element.

The criterion, the same for every op, u = 2^-24:
  A, every element:  |hip - ref| <= E.  E counts the fp32 roundings of the kernel as it is spelled: one per fused multiply-add, one per separate add, multiply or
     divide (standard model, nothing here is near the subnormal range), times 1 + 2^-10 for the products of two roundings.  The engine library is built with
     contraction on; where the source leaves the fusing to the compiler the count is the unfused one (it contains the fused one), where the source spells the FMA
     (`__builtin_fmaf` in the two gather kernels) it is that.  The resampler's `acc += w * v` is held to u sum_k |s_k| as well, the fused count: that bound
     presumes the build's contraction (the gfx950 code of both passes is one v_fmac_f32 per tap).  The kernel source compiled for a CPU passes every case with
     contraction on and reaches 1.18 of this bound on the two-tap upsample with contraction off, so a build that stops fusing there fails A, on purpose.
     fp32 division is one rounding: HIP's default is the correctly rounded divide and the build passes no flag that turns it off (no -ffast-math, no
     -fhip-fp32-correctly-rounded-divide-sqrt=off / -fno-hip-fp32-correctly-rounded-divide-sqrt in __graft_entry__.py).
  Cap, per case:     median(E / |ref|) <= CAP[op], CAP[op] <= 2 x the largest median the committed cases reach (MEDIAN_RANGE[op], measured by the CPU test on the
     fp32 emulation's cases -- the median depends on ref and E only, so no GPU number enters): A cannot go vacuous.
  B, per case:       rms(hip - ref) / rms(ref) <= C_RMS[op] = 4 x the worst value the fp32 CPU emulation reaches on the same cases (re-measured and asserted by
     test_tile_ops_cpu.py: 4 worst <= C <= 4.2 worst).
     A case of one element (the 1x1 crop, n = 1) has that element's own relative error as its B: the 1x1 crop of elev_finish (2.46 u) sets C_RMS there, the
     larger crops reach 1.23 u.
  Non-finite values: wherever ref is NaN / +inf / -inf, hip is the same kind, and nowhere else; such elements are left out of A, B and the cap, and may be at most
     2 % of a case (asserted).  Only the cases that say so produce them.
  Exact zeros (an uncovered pixel, an empty region): ref = 0 with E = 0 asks for hip == 0; they are left out of the median of E / |ref|.

The ops (each quantity below is the float64 value; s_k are the partial sums in the kernel's order):
  blend / regions   acc = fma(x, w, acc) over the covering windows in ascending (row-window, col-window) order, the weight channel acc += w; w = a[y] a[x] is the
                    fp32 window of weight_window_host, recomputed here (`weight_window`; bit-checked against td_linear_weight_window on the GPU and against
                    oracle/tiling.py here).  E = u sum_k |s_k|: the first term is the rounding of the product (fma(x, w, 0) = fl(x w)); with accumulate = 1 the prior
                    canvas value is s_0, exact.  The weight channel's first add (0 + w) is exact and not counted.
  normalise         fl(fl(c / wsum) scale): E = u |r| (1 + [scale is no power of two]).
  resample          one pass: acc += w v over the taps in table order, zero weights skipped: E = u sum_k |s_k| (the first live tap is fl(w v)).  The composed call:
                    the column bound on the twin's row result plus sum_a |wy_a| E_row at the tapped rows (the fp32 store of the row pass is E_row's last term).
  residual_plus     q = p0 / p1 [u |q|]; r = q std + mean [unfused: u |q std| + u |r|]; out = r + low [u |out|].
  elev_finish       e = r + low [u |e|]; out = sign(e) e^2: E = 2 |e| E_e + E_e^2 + u e^2.  E_e^2 is kept: where r + low cancels to a few ulp E_e exceeds |e|, and a
                    computed e of the other sign is inside it too (|e'| + |e| <= E_e then).
  climate_finish    the coordinate chain u, g, unnormalise, clamp, floor, t is evaluated IN FP32, step by step, as oracle/compose.py:123-128 and torch's
                    grid_sampler_unnormalize / clip_coordinates spell it: that chain is the specification, not its real-number value.  From the fp32 (ty, tx): the
                    four weights in float64, 1 - t exact or one rounding (checked per pixel), each product one; the blend of the live corners (the far corner of a
                    clamped cell is skipped) with one rounding per product and per add; then f0 + f1 max(elev, 0) [u |f1 m| + u |out|].  One allowance: the build may
                    contract (g + 1) size - 1 into one FMA, so the coordinate may differ from the unfused chain by d = u |(g + 1) size| / 2; the bound adds
                    d_y max|D_y f| + d_x max|D_x f|, D the feature difference across the cell, over the neighbouring cell too when the coordinate is within d of
                    an integer.  A coordinate further off is a finding.
  ddim_cfg_step     e = u + g (c - u) [u |d|, u |g d|, u |e|]; x0 = (x - s1 e) / s2 [u |s1 e|, u |t|, u |x0|]; out = s3 x0 + s4 e [u |s3 x0|, u |s4 e|, u |out|]; a
                    product with 0 or a power of two and an add of an exact 0 are not counted (g = 0, 1; alpha_prev = 1).  s1..s4 are the host's sqrtf
                    (correctly rounded) of the fp32 alphas, taken as fp32.

The fp32 emulations (`*_emu`, numpy, each FMA formed in float64 and rounded once) follow the build: contraction on.  Where the compiler decides (resample is fixed by
the bound; elev, climate, ddim) the unfused variant is emulated too, must pass A as well, and the constants are the worst over both.  EMU_WORST_A records the worst
err / E per op: every one is above 0.5, so no bound is looser than its op needs, and nothing is added to any of them.

Broken emulations (`mutant=`) miss A by the factor test_tile_ops_cpu.py prints.  One candidate is an equivalent mutant and is asserted bit-identical instead:
"the far corner not skipped (index clamped instead)" multiplies the same cell's value by a weight that is exactly 0 on a clamped coordinate (t = 0), so for finite
features it changes no bit; the skip matters for memory safety, not for the value.
"""
import math

import numpy as np

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -10
MAX_EXCLUDED = 0.02
OPS = ("blend", "regions", "normalise", "resample", "residual_plus", "elev_finish", "climate", "ddim")
# measured by test_tile_ops_cpu.py::test_fp32_emulations_pass_and_set_the_constants on the committed cases (fp32 emulations, CPU):
EMU_WORST_A = {"blend": 0.996, "regions": 0.948, "normalise": 0.975, "resample": 0.837, "residual_plus": 0.818, "elev_finish": 0.603, "climate": 0.598, "ddim": 0.785}
# least and largest median E / |ref| in u over the op's cases; CAP in u = 1.5 x the largest; C_RMS in u = 4.05 x the emulation's worst B
MEDIAN_RANGE = {"blend": (1.0, 2.98), "regions": (1.0, 2.98), "normalise": (1.0, 2.0), "resample": (2.57, 18.97), "residual_plus": (2.83, 3.18), "elev_finish": (4.5, 8.27), "climate": (4.08, 18.34), "ddim": (2.22, 14.27)}
CAP = {"blend": 4.5, "regions": 4.5, "normalise": 3.0, "resample": 28.4, "residual_plus": 4.8, "elev_finish": 12.4, "climate": 27.5, "ddim": 21.4}
C_RMS = {"blend": 3.569, "regions": 3.569, "normalise": 2.53, "resample": 5.239, "residual_plus": 2.534, "elev_finish": 9.979, "climate": 5.662, "ddim": 6.078}


def f32(v):
    return np.asarray(v, dtype=np.float32)


def f64(v):
    return np.asarray(v, dtype=np.float64)


def _fma(a, b, c):
    """a * b is exact in float64 (2 x 24 bits), the sum is rounded to 53 bits and then once to 24"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (f64(a) * f64(b) + f64(c)).astype(np.float32)


def _exact_mul(s):
    """True when a product with the fp32 scalar s carries no rounding: 0 or a power of two"""
    s = abs(float(s))
    return s == 0.0 or math.frexp(s)[0] == 0.5


# ------------------------------------------------------------------------------------------------------------------ the criterion
def judge(got, ref, E):
    """figures of one case: dict(A, at, B, median, excluded, masks_ok, elements)"""
    got, ref, E = f64(got), f64(ref), f64(E) * 1.0
    assert got.shape == ref.shape == E.shape, (got.shape, ref.shape, E.shape)
    fin = np.isfinite(ref)
    kind = lambda a: np.where(np.isnan(a), 2, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), -1, 0)))
    masks_ok = bool(np.array_equal(kind(got), kind(ref)))
    st = {"elements": int(ref.size), "excluded": float(1.0 - fin.mean()), "masks_ok": masks_ok}
    g, r, e = got[fin], ref[fin], E[fin]
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(g - r)
        ratio = np.where(err == 0, 0.0, err / e)
        ratio = np.where(np.isfinite(g), ratio, np.inf)
        med = (e / np.abs(r))[~((e == 0) & (r == 0))]          # exact zeros are held exactly and say nothing about the bound's size
    st["A"] = float(ratio.max()) if ratio.size else 0.0
    st["at"] = tuple(int(v) for v in np.argwhere(fin)[int(np.argmax(ratio))]) if ratio.size else ()
    den = float(np.sqrt(np.mean(r ** 2))) if r.size else 0.0
    num = float(np.sqrt(np.mean(np.where(np.isfinite(err), err, 0.0) ** 2))) if r.size else 0.0
    st["B"] = 0.0 if num == 0.0 else (num / den if den > 0 else float("inf"))
    st["median"] = float(np.median(med)) if med.size else 0.0
    if not masks_ok:
        st["A"] = float("inf")
    return st


def verdict(op, st):
    """what the case violates (empty: passes A, B, the cap and the non-finite rule)"""
    v = []
    if not st["masks_ok"]:
        v.append("non-finite masks differ")
    if not st["A"] <= 1.0:
        v.append(f"A: err / E = {st['A']:.3g} at {st['at']}")
    if not st["B"] <= C_RMS[op] * U:
        v.append(f"B: {st['B'] / U:.3f} u > {C_RMS[op]:.3f} u")
    if not st["median"] <= CAP[op] * U:
        v.append(f"cap: median E / |ref| = {st['median'] / U:.2f} u > {CAP[op]:.2f} u")
    if not st["excluded"] <= MAX_EXCLUDED:
        v.append(f"{100 * st['excluded']:.2f} % non-finite > 2 %")
    return v


def line(op, name, shape, st):
    return (f"{op} | {name} | {shape}: worst err / E {st['A']:.3f}, B {st['B'] / U:.3f} u (<= {C_RMS[op]:.3f}), median E / |ref| {st['median'] / U:.2f} u "
            f"(cap {CAP[op]:.2f}), non-finite {100 * st['excluded']:.2f} %")


# ------------------------------------------------------------------------------------------------------------------ blend and regions
def weight_window(size, mutant=None):
    """weight_window_host in numpy fp32: a[i] = 1 - fl(0.999) clamp(|i - mid| / mid), w = a[y] a[x]"""
    mid = np.float32(size / 2.0) if mutant == "mid = size / 2" else np.float32((size - 1) / 2.0)
    k = np.float32(1 - 1e-3)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs(np.arange(size, dtype=np.float32) - mid) / mid
    d = np.minimum(np.maximum(d, np.float32(0)), np.float32(1))
    a = (np.float32(1) - k * d).astype(np.float32)
    return (a[:, None] * a[None, :]).astype(np.float32)


def _add_window(acc, Es, xw, ww, oy, ox, size, emu, *, no_weight=False, skip_rows=None, swap=False, le=False):
    """one window into acc (C + 1, H, W) at offset (oy, ox): float64 with the running sum of |s_k| in Es, or fp32 (emu).  Reads are by flat offset, as the kernels'."""
    C, H, W = acc.shape[0] - 1, acc.shape[1], acc.shape[2]
    ext = size + (1 if le else 0)
    ys, xs = np.arange(max(0, oy), min(H, oy + ext)), np.arange(max(0, ox), min(W, ox + ext))
    if skip_rows is not None:
        ys = ys[~skip_rows[ys]]
    if not ys.size or not xs.size:
        return
    ly, lx = (ys - oy)[:, None], (xs - ox)[None, :]
    if swap:
        ly, lx = lx, ly
    sl = np.ix_(ys, xs)
    wv = np.take(ww.reshape(-1), ly * size + lx, mode="wrap")
    for c in range(C):
        xv = np.take(xw.reshape(-1), (c * size + ly) * size + lx, mode="wrap")
        if emu:
            acc[c][sl] = _fma(xv, wv, acc[c][sl])
        else:
            acc[c][sl] += f64(xv) * f64(wv)
            Es[c][sl] += np.abs(acc[c][sl])
    if no_weight:
        return
    if emu:
        acc[C][sl] = acc[C][sl] + wv
    else:
        prev = acc[C][sl]
        acc[C][sl] = prev + f64(wv)
        Es[C][sl] += np.where(prev != 0, np.abs(acc[C][sl]), 0.0)


class Refused(Exception):
    """what the C entry point answers with an error code"""


def _rowmap(n, starts, size):
    m = np.full((n, 4), -1, np.int64)
    for ic, s in enumerate(starts):
        for y in range(max(0, s), min(n, s + size)):
            k = int(np.count_nonzero(m[y] >= 0))
            if k == 4:
                raise Refused("more than 4 windows cover a canvas row / column")
            m[y, k] = ic
    return m


def _blend(tiles, C, Hc, Wc, size, row_starts, col_starts, wi, wj, accumulate, prior, emu, mutant=None):
    if C + 1 > 8:
        raise Refused("C + 1 must be <= 8")
    rowmap = _rowmap(Hc, row_starts, size)
    _rowmap(Wc, col_starts, size)
    tile_of = {}
    for i, (a, b) in enumerate(zip(wi, wj)):
        if not (0 <= a < len(row_starts) and 0 <= b < len(col_starts)):
            raise Refused("window index out of range")
        tile_of[(int(a), int(b))] = i
    dt = np.float32 if emu else np.float64
    acc = np.zeros((C + 1, Hc, Wc), dt)
    if accumulate and mutant != "accumulate ignores the prior canvas":
        acc[:] = prior
    Es = None if emu else np.zeros_like(acc)
    ww = weight_window(size, mutant)
    first = True
    for ic, rs in enumerate(row_starts):
        skip = (rowmap[:, 3] == ic) if mutant == "fourth covering row-window dropped" else None
        for jc, cs in enumerate(col_starts):
            slot = tile_of.get((ic, jc), -1)
            if slot < 0:
                continue
            oy, ox = int(rs), int(cs)
            if mutant == "overhang clamped, not cropped":
                oy, ox = min(max(oy, 0), Hc - size), min(max(ox, 0), Wc - size)
            _add_window(acc, Es, tiles[slot], ww, oy, ox, size, emu, no_weight=first and mutant == "weight channel misses one window", skip_rows=skip,
                        swap=mutant == "ly / lx swapped")
            first = False
    return acc if emu else (acc, Es * U * SECOND_ORDER)


def blend_ref(tiles, C, Hc, Wc, size, row_starts, col_starts, wi, wj, accumulate=0, prior=None):
    """float64 td_blend_windows on fp32 tiles (n, C, size, size) -> (canvas (C + 1, Hc, Wc), E)"""
    return _blend(f32(tiles), C, Hc, Wc, size, row_starts, col_starts, wi, wj, accumulate, prior, False)


def blend_emu(tiles, C, Hc, Wc, size, row_starts, col_starts, wi, wj, accumulate=0, prior=None, mutant=None):
    return _blend(f32(tiles), C, Hc, Wc, size, row_starts, col_starts, wi, wj, accumulate, prior, True, mutant)


def _regions(wins, desc, C, size, h, w, emu, mutant=None):
    if C + 1 > 8:
        raise Refused("C + 1 must be <= 8")
    desc = np.asarray(desc)
    if np.any(desc[..., 0] >= len(wins)):
        raise Refused("window slot out of range")
    n = desc.shape[0]
    out = np.zeros((n, C + 1, h, w), np.float32 if emu else np.float64)
    Es = None if emu else np.zeros_like(out)
    ww = weight_window(size, mutant)
    for r in range(n):
        first = True
        for slot, oy, ox in desc[r]:
            if slot < 0:
                if mutant == "terminator ignored":
                    continue
                break
            _add_window(out[r], None if emu else Es[r], f32(wins[slot]), ww, int(oy), int(ox), size, emu, swap=mutant == "ly / lx swapped",
                        le=mutant == "bounds test <= size", no_weight=first and mutant == "weight channel misses one window")
            first = False
    return out if emu else (out, Es * U * SECOND_ORDER)


def regions_ref(wins, desc, C, size, h, w):
    """float64 td_gather_regions: wins = list of (C, size, size) fp32, desc (n, maxk, 3) = (slot, y, x of the window's first row / column in the region)"""
    return _regions(wins, desc, C, size, h, w, False)


def regions_emu(wins, desc, C, size, h, w, mutant=None):
    return _regions(wins, desc, C, size, h, w, True, mutant)


def _rs(seed):
    return np.random.RandomState(seed)


def tile_starts(length, tile, stride):
    """training/evaluation/__init__.py:_tile_starts (oracle/tiling.py restates it; asserted equal in the CPU test)"""
    if length <= tile:
        return [0]
    s = list(range(0, max(1, length - tile + 1), max(1, stride)))
    if s[-1] != length - tile:
        s.append(length - tile)
    return s


def blend_cases():
    """name -> dict(C, Hc, Wc, size, rows, cols, tiles (n, C, size, size), launches [(window indices into the grid list, accumulate)], prior)"""
    def case(seed, C, Hc, Wc, size, rows, cols, launches=None, prior=None):
        grid = [(i, j) for i in range(len(rows)) for j in range(len(cols))]
        tiles = (_rs(seed).standard_normal((len(grid), C, size, size)) * 1.5 + 0.3).astype(np.float32)
        return dict(C=C, Hc=Hc, Wc=Wc, size=size, rows=list(rows), cols=list(cols), grid=grid, tiles=tiles, launches=launches or [(list(range(len(grid))), 0)], prior=prior)
    c = {}
    c["regular size 16 stride 8, 40x40, C 5"] = case(1, 5, 40, 40, 16, tile_starts(40, 16, 8), tile_starts(40, 16, 8))
    c["stride size/4: 16 live terms, size 16, 28x28, C 7"] = case(2, 7, 28, 28, 16, [0, 4, 8, 12], [0, 4, 8, 12])
    c["ragged tile_starts, last window pulled back, 37x29, C 1"] = case(3, 1, 37, 29, 16, tile_starts(37, 16, 8), tile_starts(29, 16, 8))
    c["overhang on all four sides, size 8, 11x13, C 2"] = case(4, 2, 11, 13, 8, [-3, 1, 6], [-5, 0, 7])
    c["subset of the grid with an uncovered pixel, odd size 5, 12x9, C 3"] = case(5, 3, 12, 9, 5, [0, 3, 7], [0, 4], launches=[([0, 3, 4], 0)])
    prior = np.concatenate([_rs(60).standard_normal((4, 21, 17)), _rs(61).uniform(0.1, 3.0, (1, 21, 17))]).astype(np.float32)
    c["accumulate over a non-zero canvas made by the test, size 8, 21x17, C 4"] = case(6, 4, 21, 17, 8, tile_starts(21, 8, 4), tile_starts(17, 8, 4),
                                                                                   launches=[(list(range(0, 20, 2)), 1)], prior=prior)
    c["two launches, the second accumulates on the first, size 8, 21x17, C 4"] = case(7, 4, 21, 17, 8, tile_starts(21, 8, 4), tile_starts(17, 8, 4),
                                                                                  launches=[(list(range(0, 20, 2)), 0), (list(range(1, 20, 2)), 1)])
    c["size 2 stride 1, 5x7, C 1"] = case(8, 1, 5, 7, 2, [0, 1, 2, 3], [0, 1, 2, 3, 4, 5])
    return c


def run_blend_case(cs, launch):
    """runs the case's launches through launch(tiles_subset, wi, wj, accumulate, prior) -> fp32 canvas; returns [(got, ref, E)] per launch.  The prior of a later
    launch is what the earlier one STORED (fp32), as on the GPU."""
    out, prior = [], cs["prior"]
    for idx, accumulate in cs["launches"]:
        wi, wj = [cs["grid"][i][0] for i in idx], [cs["grid"][i][1] for i in idx]
        tiles = np.ascontiguousarray(cs["tiles"][idx])
        got = launch(tiles, wi, wj, accumulate, prior)
        ref, E = blend_ref(tiles, cs["C"], cs["Hc"], cs["Wc"], cs["size"], cs["rows"], cs["cols"], wi, wj, accumulate, prior)
        out.append((got, ref, E))
        prior = f32(got)
    return out


def regions_cases():
    """name -> dict(C, size, h, w, wins [list of (C, size, size)], desc (n, maxk, 3))"""
    c = {}
    wins = [w for w in (_rs(20).standard_normal((1, 2, 8, 8)) + 0.2).astype(np.float32)]
    c["maxk 1, negative offsets, 6x9"] = dict(C=2, size=8, h=6, w=9, wins=wins, desc=np.array([[[0, -1, -2]]], np.int32))
    wins = [w for w in (_rs(21).standard_normal((5, 3, 8, 8)) * 2 - 0.4).astype(np.float32)]
    h, w = 17, 19
    T = [-1, 0, 0]
    desc = np.array([
        [[0, -3, -2], [1, -3, 6], [2, 5, -2], [3, 5, 6], [4, 9, 11], T],                    # four windows around a corner and one further in
        [[0, 0, 0], T, [2, 1, 1], [3, 2, 2], [4, 3, 3], [1, 4, 4]],                         # a terminator in the middle: what follows looks live and is ignored
        [T, [0, 0, 0], T, T, T, T],                                                         # empty list: zeros, weight 0
        [[0, -8, 0], [1, h, 0], [2, 0, -8], [3, 0, w], [4, -7, -7], [0, h - 1, w - 1]],     # one past the region on each side (touch nothing); one pixel each
        [[1, 4, 5], [1, 4, 9], [3, 8, 5], [3, 8, 9], T, T],                                 # the same window twice: shared within a region too
    ], np.int32)
    c["five regions sharing five windows, 17x19, maxk 6"] = dict(C=3, size=8, h=h, w=w, wins=wins, desc=desc)
    b = blend_cases()["stride size/4: 16 live terms, size 16, 28x28, C 7"]
    desc = np.array([[[k, b["rows"][i], b["cols"][j]] for k, (i, j) in enumerate(b["grid"])]], np.int32)
    c["the stride size/4 blend geometry as one region, 28x28, maxk 16"] = dict(C=7, size=16, h=28, w=28, wins=[t for t in b["tiles"]], desc=desc)
    return c


# ------------------------------------------------------------------------------------------------------------------ normalise
def normalise_ref(canvas, scale):
    c = f64(f32(canvas))
    s = float(np.float32(scale))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = c[:-1] / c[-1:] * s
    return r, U * np.abs(r) * (1 if _exact_mul(s) else 2) * SECOND_ORDER


def normalise_emu(canvas, scale, mutant=None):
    c = f32(canvas)
    den = c[0:1] if mutant == "divided by channel 0" else c[-1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((c[:-1] / den).astype(np.float32) * np.float32(scale)).astype(np.float32)


def normalise_cases():
    c = {}
    for k, (name, scale) in enumerate((("scale 1", 1.0), ("scale 2 = 1 / 0.5", 1 / 0.5), ("scale 1 / 0.3", 1 / 0.3), ("scale 0.18215", 0.18215))):
        rs = _rs(30 + k)
        wsum = rs.uniform(1e-3, 4.0, (1, 13, 23))
        c[f"{name}, 13x23, C 3"] = dict(canvas=np.concatenate([rs.standard_normal((3, 13, 23)) * wsum, wsum]).astype(np.float32), scale=scale)
    rs = _rs(35)
    wsum = rs.uniform(1e-3, 4.0, (1, 19, 15))
    cv = np.concatenate([rs.standard_normal((5, 19, 15)) * wsum, wsum]).astype(np.float32)
    cv[:, 3, 4] = 0.0                                   # uncovered: 0 / 0 -> NaN in every channel
    cv[:, 18, 14] = 0.0
    cv[-1, 7, 7] = 0.0                                  # a weight of 0 under a value: +-inf
    c["uncovered pixels (0 / 0) and x / 0, scale 1 / 0.3, 19x15, C 5"] = dict(canvas=cv, scale=1 / 0.3)
    return c


# ------------------------------------------------------------------------------------------------------------------ resample
def _pass_ref(x, idx, wts, axis):
    """one pass along `axis` of x (C, H, W) float64: returns (sum, sum_k |s_k|) in table order, zero weights skipped"""
    idx, wts = np.asarray(idx), f64(f32(wts))
    s = E = None
    for b in range(idx.shape[1]):
        live = wts[:, b] != 0
        v = np.take(x, idx[:, b], axis=axis)
        shp = [1, 1, 1]
        shp[axis] = -1
        lv, wv = live.reshape(shp), wts[:, b].reshape(shp)
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.where(lv, np.where(lv, v, 0.0) * wv, 0.0)
        s = t if s is None else s + t
        E = np.where(lv, np.abs(s), 0.0) if E is None else E + np.where(lv, np.abs(s), 0.0)
    return s, E


def resample_ref(x, taps_y, taps_x):
    """float64 td_resample2d on fp32 x (C, Hin, Win): rows pass (along x) first, then columns -> (out, E)"""
    (iy, wy), (ix, wx) = taps_y, taps_x
    row, Er = _pass_ref(f64(f32(x)), ix, wx, 2)
    out, Ec = _pass_ref(row, iy, wy, 1)
    prop = np.zeros_like(out)
    for a in range(np.asarray(iy).shape[1]):
        prop += np.abs(f64(f32(wy))[:, a])[None, :, None] * np.take(Er * U, np.asarray(iy)[:, a], axis=1)
    return out, (Ec * U + prop) * SECOND_ORDER


def identity_taps(n):
    return np.arange(n, dtype=np.int32)[:, None].copy(), np.ones((n, 1), np.float32)


def _pass_emu(x, idx, wts, axis, mutant=None):
    idx, wts = np.asarray(idx), f32(wts)
    K = idx.shape[1]
    acc = None
    for b in range(K - 1 if mutant == "last tap dropped" else K):
        if mutant == "table row stride K - 1":
            o = np.arange(idx.shape[0]) * (K - 1) + b
            ib, wb = idx.reshape(-1)[o], wts.reshape(-1)[o]
        else:
            ib, wb = idx[:, b], wts[:, b]
        shp = [1, 1, 1]
        shp[axis] = -1
        live = (wb != 0).reshape(shp) | (mutant == "zero weights not skipped")
        v = np.take(x, ib, axis=axis)
        if acc is None:
            acc = np.zeros(v.shape, np.float32)
        acc = np.where(live, _fma(wb.reshape(shp), v, acc), acc).astype(np.float32)
    return acc


def resample_emu(x, taps_y, taps_x, mutant=None):
    if mutant == "tables swapped":
        taps_y, taps_x = taps_x, taps_y
    row = _pass_emu(f32(x), taps_x[0], taps_x[1], 2, mutant)
    return _pass_emu(row, taps_y[0], taps_y[1], 1, mutant)


def resample_cases():
    """name -> dict(x (C, Hin, Win), ty, tx) with ty / tx = (index, weight) tables; built from the product's table functions and by hand"""
    from terrain_diffusion_amd import composition as cp
    c = {}

    def x(seed, C, H, W):
        return (_rs(seed).standard_normal((C, H, W)) * 3 + 1).astype(np.float32)
    c["rows only: upsample 5 -> 37, 11 rows, C 3"] = dict(x=x(40, 3, 11, 5), ty=identity_taps(11), tx=cp.bilinear_taps(5, 37))
    c["columns only: upsample 8 -> 64, 7 columns, C 1"] = dict(x=x(41, 1, 8, 7), ty=cp.bilinear_taps(8, 64), tx=identity_taps(7))
    c["rows only: AA shrink 64 -> 9, 5 rows, C 1"] = dict(x=x(42, 1, 5, 64), ty=identity_taps(5), tx=cp.bilinear_aa_taps(64, 9))
    c["columns only: AA shrink 37 -> 5, 21 columns, C 3"] = dict(x=x(43, 3, 37, 21), ty=cp.bilinear_aa_taps(37, 5), tx=identity_taps(21))
    c["rows only: Gaussian sigma 5 on n 12, 9 rows, C 1"] = dict(x=x(44, 1, 9, 12), ty=identity_taps(9), tx=cp.gaussian_taps(12, 5))
    c["columns only: Gaussian sigma 5 on n 12, 31 columns, C 3"] = dict(x=x(45, 3, 12, 31), ty=cp.gaussian_taps(12, 5), tx=identity_taps(31))
    c["composed: upsample 5x8 -> 37x64, C 3"] = dict(x=x(46, 3, 5, 8), ty=cp.bilinear_taps(5, 37), tx=cp.bilinear_taps(8, 64))
    c["composed: AA shrink 64x37 -> 9x5, C 1"] = dict(x=x(47, 1, 64, 37), ty=cp.bilinear_aa_taps(64, 9), tx=cp.bilinear_aa_taps(37, 5))
    c["composed: Gaussian sigma 5, 12x13, C 3"] = dict(x=x(48, 3, 12, 13), ty=cp.gaussian_taps(12, 5), tx=cp.gaussian_taps(13, 5))
    c["composed: up 5 -> 37 in y, AA 64 -> 9 in x, C 1"] = dict(x=x(49, 1, 5, 64), ty=cp.bilinear_taps(5, 37), tx=cp.bilinear_aa_taps(64, 9))
    rs = _rs(50)                                                         # hand-made, 12 -> 12 in both axes: negative weights in y, the Gaussian in x
    iy = rs.randint(0, 12, (12, 4)).astype(np.int32)
    wy = (rs.standard_normal((12, 4)) * 0.7).astype(np.float32)
    c["composed: hand-made table with negative weights in y, Gaussian in x, 12x12, C 3"] = dict(x=x(51, 3, 12, 12), ty=(iy, wy), tx=cp.gaussian_taps(12, 5))
    xx = x(52, 1, 6, 7)
    xx[0, 2, 3], xx[0, 4, 1], xx[0, 0, 6] = np.inf, np.nan, -np.inf
    bad_col = np.array([3, 1, 6], np.int32)
    ix = rs.randint(0, 7, (9, 3)).astype(np.int32)
    wx = rs.uniform(0.1, 1.0, (9, 3)).astype(np.float32)
    iy = rs.randint(0, 6, (8, 3)).astype(np.int32)
    wy = rs.uniform(0.1, 1.0, (8, 3)).astype(np.float32)
    hit = np.isin(ix, bad_col)
    wx[hit] = 0.0                                                        # every tap at a column that holds a non-finite value has weight 0 ...
    ix[0], wx[0] = bad_col, 0.0                                          # ... and one output has nothing but such taps: 0
    ix[1, 1], wx[1, 1] = 3, 0.0
    c["zero-weight taps on inf / NaN cells, 6x7 -> 8x9, C 1"] = dict(x=xx, ty=(iy, wy), tx=(ix, wx), finite_out=True)
    return c


# ------------------------------------------------------------------------------------------------------------------ residual_plus / elev_finish
def elev_ref(packed, low, mean, std, crop=None):
    """float64 td_residual_plus (crop None) or td_elev_finish (crop = (oi, oj, h, w)) on fp32 packed (2, Hp, Wp), low (Hp, Wp) -> (out, E)"""
    p, low = f64(f32(packed)), f64(f32(low))
    mean, std = float(np.float32(mean)), float(np.float32(std))
    q = p[0] / p[1]
    qs = q * std
    r = qs + mean
    Er = abs(std) * U * np.abs(q) + U * np.abs(qs) + U * np.abs(r)
    e = r + low
    Ee = Er + U * np.abs(e)
    if crop is None:
        return e, Ee * SECOND_ORDER
    oi, oj, h, w = crop
    if oi < 0 or oj < 0 or oi + h > p.shape[1] or oj + w > p.shape[2]:
        raise Refused("crop outside the window")
    e, Ee = e[oi:oi + h, oj:oj + w], Ee[oi:oi + h, oj:oj + w] * SECOND_ORDER
    return np.sign(e) * e * e, (2 * np.abs(e) * Ee + Ee * Ee + U * e * e) * SECOND_ORDER


def elev_emu(packed, low, mean, std, crop=None, fused=True, mutant=None):
    p, low = f32(packed), f32(low)
    mean, std = np.float32(mean), np.float32(std)
    Hp, Wp = low.shape
    if mutant == "std / mean swapped":
        mean, std = std, mean
    if crop is None:
        p0, p1, lo = p[0], p[1], low
    else:
        oi, oj, h, w = crop
        if mutant == "oi / oj swapped":
            oi, oj = oj, oi
        flat = ((np.arange(h) + oi)[:, None] * Wp + (np.arange(w) + oj)[None, :])
        plane = h * w if mutant == "plane stride from the crop" else Hp * Wp
        p0, p1, lo = np.take(p.reshape(-1), flat, mode="wrap"), np.take(p.reshape(-1), plane + flat, mode="wrap"), np.take(low.reshape(-1), flat, mode="wrap")
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (p0 / (p0 if mutant == "divided by p0" else p1)).astype(np.float32)
    r = _fma(q, std, mean) if fused else ((q * std).astype(np.float32) + mean).astype(np.float32)
    e = (r + lo).astype(np.float32)
    if crop is None:
        return e
    sign = np.float32(1) if mutant == "sign lost" else np.sign(e).astype(np.float32)
    return (sign * (e * e).astype(np.float32)).astype(np.float32)


ELEV_HP, ELEV_WP = 19, 23
ELEV_CROPS = {"offset 0": (0, 0, 7, 9), "far corner": (8, 9, 11, 14), "1x1": (5, 17, 1, 1), "full window": (0, 0, 19, 23), "interior, oi != oj": (3, 11, 13, 10)}


def elev_inputs(stats):
    """(packed, low, mean, std) on the 19x23 window: decoder weights 0.2 .. 1.7; in the low band a block that cancels r + low to a few ulp, a block where it is exactly 0
    and negative sums everywhere else at random"""
    mean, std = stats
    rs = _rs(70 + int(abs(mean) * 10))
    p1 = rs.uniform(0.2, 1.7, (ELEV_HP, ELEV_WP)).astype(np.float32)
    p0 = (rs.standard_normal((ELEV_HP, ELEV_WP)) * 4 * p1).astype(np.float32)
    low = (rs.standard_normal((ELEV_HP, ELEV_WP)) * 6 - 1).astype(np.float32)
    packed = np.stack([p0, p1])
    r = elev_emu(packed, np.zeros_like(low), mean, std)                  # fl32(r) of the fused build
    k = rs.randint(-3, 4, (4, 6))
    near = -r[4:8, 10:16]
    for _ in range(3):
        near = np.where(k > 0, np.nextafter(near, np.float32(np.inf)), np.where(k < 0, np.nextafter(near, np.float32(-np.inf)), near)).astype(np.float32)
        k = k - np.sign(k)
    low[4:8, 10:16] = near                                              # r + low within 3 ulp of 0, both signs, and 0
    packed[0, 12:15, 2:6] = 0.0                                          # q = 0: r = mean exactly ...
    low[12:15, 2:6] = -np.float32(mean)                                  # ... and r + low == 0 exactly, in fp32 and in float64
    return packed, low, mean, std


ELEV_STATS = ((0.0, 1.1678), (-2.37, 1.1678))


# ------------------------------------------------------------------------------------------------------------------ climate
def climate_coords(n_src, first, count, S, c1):
    """the fp32 chain along one axis: (coordinate clamped, unclamped, d = allowance for the contracted (g + 1) size - 1), all from fp32 steps"""
    o = np.float32
    ii = (np.int64(first) + np.arange(count, dtype=np.int64)).astype(np.float32)          # (float)(i1 + r): int -> fp32, round to nearest even
    u = (((ii + o(0.5)) / o(S)) - o(c1)) + o(0.5)
    g = (((u + o(0.5)) * o(2)) / o(n_src)) - o(1)
    a = (g + o(1)).astype(np.float32)
    prod = (a * o(n_src)).astype(np.float32)
    y = ((prod - o(1)) / o(2)).astype(np.float32)
    d = U * np.abs(f64(a) * n_src) / 2
    return np.minimum(np.maximum(y, o(0)), o(n_src - 1)).astype(np.float32), y, d, g.astype(np.float32), a


def _climate_fused_coords(n_src, first, count, S, c1):
    yc, y, d, g, a = climate_coords(n_src, first, count, S, c1)
    y = (_fma(a, np.float32(n_src), np.float32(-1)) / np.float32(2)).astype(np.float32)
    return np.minimum(np.maximum(y, np.float32(0)), np.float32(n_src - 1)).astype(np.float32)


def climate_blend64(feats, y, x):
    """the five blended features in float64 from fp32 clamped coordinates y (h,), x (w,): (f (5, h, w), corner weights, corner indices, liveness)"""
    F = f64(feats)
    Hs, Ws = F.shape[1:]
    y0, x0 = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)
    ty, tx = f64(y) - y0, f64(x) - x0
    y1, x1 = y0 + 1, x0 + 1
    ly, lx = y1 < Hs, x1 < Ws
    y1c, x1c = np.minimum(y1, Hs - 1), np.minimum(x1, Ws - 1)
    W = [np.outer(1 - ty, 1 - tx), np.outer(1 - ty, tx), np.outer(ty, 1 - tx), np.outer(ty, tx)]        # nw, ne, sw, se
    P = [F[:, y0][:, :, x0], F[:, y0][:, :, x1c], F[:, y1c][:, :, x0], F[:, y1c][:, :, x1c]]
    L = [np.ones((y.size, x.size), bool), np.outer(np.ones_like(ly), lx), np.outer(ly, np.ones_like(lx)), np.outer(ly, lx)]
    f = sum(np.where(l, p * w, 0.0) for p, w, l in zip(P, W, L))
    return f, W, P, L, (ty, tx, y0, x0)


def climate_ref(feats, elev, Hs, Ws, i1, j1, h, w, S, ci1, cj1):
    """float64 td_climate_finish on fp32 feats (5, Hs, Ws), elev (h, w) -> (out (5, h, w), E)"""
    F = f64(f32(feats))
    y, yu, dy, _, _ = climate_coords(Hs, i1, h, S, ci1)
    x, xu, dx, _, _ = climate_coords(Ws, j1, w, S, cj1)
    f, W, P, L, (ty, tx, y0, x0) = climate_blend64(F, y, x)
    # weights: 1 - t exact or one rounding, the product one
    ry = (f64((np.float32(1) - f32(ty)).astype(np.float32)) != 1 - ty).astype(np.float64)
    rx = (f64((np.float32(1) - f32(tx)).astype(np.float32)) != 1 - tx).astype(np.float64)
    one_y, one_x = np.ones_like(ry), np.ones_like(rx)
    nr = [np.add.outer(ry, rx) + 1, np.add.outer(ry, 0 * rx) + 1, np.add.outer(0 * ry, rx) + 1, np.add.outer(0 * one_y, 0 * one_x) + 1]
    E = np.zeros_like(f)
    s = np.zeros_like(f)
    started = np.zeros(f.shape[1:], bool)
    for p, wgt, l, n in zip(P, W, L, nr):
        t = np.where(l, p * wgt, 0.0)
        E += np.where(l, np.abs(p) * (n * U * np.abs(wgt)) + U * np.abs(t), 0.0)      # the weight's roundings carried by |p|, the product's own
        s = s + t
        E += np.where(l & started, U * np.abs(s), 0.0)                                 # an add after the first live term
        started = started | l
    # contraction allowance: d x the largest feature difference across the cell (and its neighbour when the coordinate is within d of an integer)
    dy = np.where((f64(yu) < -dy) | (f64(yu) > Hs - 1 + dy), 0.0, dy)
    dx = np.where((f64(xu) < -dx) | (f64(xu) > Ws - 1 + dx), 0.0, dx)
    Dy = np.zeros((5, Hs, Ws))
    Dx = np.zeros((5, Hs, Ws))
    Dy[:, :-1, :] = np.abs(np.diff(F, axis=1))
    Dx[:, :, :-1] = np.abs(np.diff(F, axis=2))
    cell_y = np.maximum(Dy, np.concatenate([Dy[:, :, 1:], Dy[:, :, -1:]], axis=2))     # both columns of the cell (y0 .. y0 + 1, x0 .. x0 + 1)
    cell_x = np.maximum(Dx, np.concatenate([Dx[:, 1:, :], Dx[:, -1:, :]], axis=1))
    sy, sx = np.zeros_like(f), np.zeros_like(f)
    for oy in (-1, 0, 1):
        my = (oy == 0) | ((oy < 0) & (ty <= dy)) | ((oy > 0) & (1 - ty <= dy))
        yy = np.clip(y0 + oy, 0, Hs - 1)
        for ox in (-1, 0, 1):
            mx = (ox == 0) | ((ox < 0) & (tx <= dx)) | ((ox > 0) & (1 - tx <= dx))
            xx = np.clip(x0 + ox, 0, Ws - 1)
            m = np.outer(my, mx)
            sy = np.maximum(sy, np.where(m, cell_y[:, yy][:, :, xx], 0.0))
            sx = np.maximum(sx, np.where(m, cell_x[:, yy][:, :, xx], 0.0))
    E = E + dy[None, :, None] * sy + dx[None, None, :] * sx
    m = np.maximum(f64(f32(elev)), 0.0)
    fm = f[1] * m
    t0 = f[0] + fm
    out = np.stack([t0, f[2], f[3], f[4], f[1]])
    E0 = E[0] + m * E[1] + U * np.abs(fm) + U * np.abs(t0)
    return out, np.stack([E0, E[2], E[3], E[4], E[1]]) * SECOND_ORDER


def climate_emu(feats, elev, Hs, Ws, i1, j1, h, w, S, ci1, cj1, fused=False, mutant=None):
    """climate_finish_kernel in numpy fp32; fused: (g + 1) size - 1 and the blend's adds contracted.  Out-of-range reads wrap (flat offsets), as memory would give something"""
    o = np.float32
    F = f32(feats)
    if mutant == "ci1 truncated towards zero":
        ci1, cj1 = int(i1 / S), int(j1 / S)

    def axis(n, first, count, c1):
        if mutant in ("align_corners=True", "no +0.5 in u", "no border clamp"):
            ii = (np.int64(first) + np.arange(count, dtype=np.int64)).astype(np.float32)
            u = (((ii + o(0.5)) / o(S)) - o(c1)) + (o(0) if mutant == "no +0.5 in u" else o(0.5))
            g = (((u + o(0.5)) * o(2)) / o(n)) - o(1)
            yv = ((g + o(1)) / o(2) * o(n - 1)).astype(np.float32) if mutant == "align_corners=True" else (((g + o(1)) * o(n) - o(1)) / o(2)).astype(np.float32)
            return yv if mutant == "no border clamp" else np.minimum(np.maximum(yv, o(0)), o(n - 1)).astype(np.float32)
        return _climate_fused_coords(n, first, count, S, c1) if fused else climate_coords(n, first, count, S, c1)[0]
    y, x = axis(Hs, i1, h, ci1), axis(Ws, j1, w, cj1)
    y0f, x0f = np.floor(y), np.floor(x)
    y0, x0 = y0f.astype(np.int64), x0f.astype(np.int64)
    ty, tx = (y - y0f).astype(np.float32), (x - x0f).astype(np.float32)
    wnw, wne = np.outer(o(1) - ty, o(1) - tx).astype(np.float32), np.outer(o(1) - ty, tx).astype(np.float32)
    wsw, wse = np.outer(ty, o(1) - tx).astype(np.float32), np.outer(ty, tx).astype(np.float32)
    if mutant == "wne / wsw swapped":
        wne, wsw = wsw, wne
    y1, x1 = y0 + 1, x0 + 1
    iy1, ix1 = np.outer(y1 < Hs, np.ones(w, bool)), np.outer(np.ones(h, bool), x1 < Ws)
    iy0 = ix0 = np.ones((h, w), bool)
    if mutant == "no border clamp":                                  # corners outside the map are skipped (anything else would be an out-of-bounds read)
        iy0, ix0 = np.outer(y0 >= 0, np.ones(w, bool)) & np.outer(y0 < Hs, np.ones(w, bool)), np.outer(np.ones(h, bool), x0 >= 0) & np.outer(np.ones(h, bool), x0 < Ws)
        iy1, ix1 = iy1 & np.outer(y1 >= 0, np.ones(w, bool)), ix1 & np.outer(np.ones(h, bool), x1 >= 0)
    if mutant == "far corner clamped, not skipped":
        y1, x1 = np.minimum(y1, Hs - 1), np.minimum(x1, Ws - 1)
        iy1 = ix1 = np.ones((h, w), bool)
    flat = F.reshape(5, -1)
    g = lambda yy, xx: np.take(flat, (yy[:, None] * Ws + xx[None, :]), axis=1, mode="wrap")
    live = [iy0 & ix0, iy0 & ix1, iy1 & ix0, iy1 & ix1]
    f = None
    for p, wgt, l in zip((g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1)), (wnw, wne, wsw, wse), live):
        if f is None:
            f = np.where(l, (p * wgt).astype(np.float32), o(0)).astype(np.float32)
        else:
            t = _fma(p, wgt, f) if fused else (f + (p * wgt).astype(np.float32)).astype(np.float32)
            f = np.where(l, t, f).astype(np.float32)
    m = f32(elev) if mutant == "max(elev, 0) dropped" else np.maximum(f32(elev), o(0))
    t0 = _fma(f[1], m, f[0]) if fused else (f[0] + (f[1] * m).astype(np.float32)).astype(np.float32)
    planes = [f[2], f[3], f[4], f[1]]
    if mutant == "planes 1-4 rotated":
        planes = planes[1:] + planes[:1]
    return np.stack([t0] + planes).astype(np.float32)


def climate_cases():
    """name -> dict(feats (5, Hs, Ws), elev (h, w), Hs, Ws, i1, j1, h, w, S, ci1, cj1).  ci1 / cj1 are the call's own arguments: the cases move them off
    floor(i1 / S) to push the request over each border of the feature map"""
    c = {}

    def case(seed, Hs, Ws, S, i1, j1, h, w, di=0, dj=0, steep=False):
        rs = _rs(seed)
        base = rs.uniform(-5, 30, (Hs, Ws))
        beta = rs.uniform(-0.012, -0.001, (Hs, Ws))
        elev = rs.standard_normal((h, w)) * 1500 + 400
        elev[rs.uniform(size=(h, w)) < 0.1] = 0.0
        if steep:                                                       # lapse rate against baseline: plane 0 cancels; a large step across one cell
            base = rs.uniform(20, 30, (Hs, Ws))
            base[Hs // 2:, :] += 2000.0
            elev = base.mean() / 0.0065 * (1 + 0.05 * rs.standard_normal((h, w)))
            beta = np.full((Hs, Ws), -0.0065) * (1 + 0.01 * rs.standard_normal((Hs, Ws)))
        feats = np.stack([base, beta, rs.standard_normal((Hs, Ws)) * 10, rs.uniform(0, 3000, (Hs, Ws)), rs.standard_normal((Hs, Ws)) * 0.3]).astype(np.float32)
        return dict(feats=feats, elev=elev.astype(np.float32), Hs=Hs, Ws=Ws, i1=i1, j1=j1, h=h, w=w, S=float(S), ci1=i1 // S + di, cj1=j1 // S + dj)
    c["S 256, 6x7, rows cross a cell, columns straddle the origin, 48x80"] = case(80, 6, 7, 256, 100, -40, 48, 80)
    c["S 96, 5x6, rows straddle the origin (i1 -20), 48x80"] = case(81, 5, 6, 96, -20, 60, 48, 80)
    c["S 96, 6x7, far origin i1 -1000003 j1 999983, 48x80"] = case(82, 6, 7, 96, -1000003, 999983, 48, 80)
    c["S 256, 6x7, far origin i1 1000121 j1 -999871, 40x64"] = case(83, 6, 7, 256, 1000121, -999871, 40, 64)
    c["S 96, 4x5, clamps at the low border in y and x, 48x80"] = case(84, 4, 5, 96, 10, 30, 48, 80, di=1, dj=1)
    c["S 96, 3x3, clamps at the high border in y and x (y1 == Hs skipped), 48x80"] = case(85, 3, 3, 96, 10, 30, 48, 80, di=-1, dj=-1)
    c["S 256, 3x4, low border in y, high border in x, 48x80"] = case(86, 3, 4, 256, 100, 90, 48, 80, di=1, dj=-2)
    c["S 96, Hs 1, 1x4, 33x47"] = case(87, 1, 4, 96, -7, 50, 33, 47)
    c["S 96, Ws 1, 3x1, 33x47"] = case(88, 3, 1, 96, 40, -13, 33, 47)
    c["S 96, 6x7, steep features, plane 0 cancels, 48x80"] = case(89, 6, 7, 96, 200, -300, 48, 80, steep=True)
    return c


def climate_args(cs):
    return tuple(cs[k] for k in ("Hs", "Ws", "i1", "j1", "h", "w", "S", "ci1", "cj1"))


# ------------------------------------------------------------------------------------------------------------------ ddim
def ddim_scalars(alpha_t, alpha_prev):
    """the four host sqrtf values, fp32: sqrt(1 - a_t), sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev)"""
    a, p, one = np.float32(alpha_t), np.float32(alpha_prev), np.float32(1)
    if not (0 < a <= 1 and 0 < p <= 1):
        raise Refused("alpha outside (0, 1]")
    return np.sqrt(one - a), np.sqrt(a), np.sqrt(p), np.sqrt(one - p)


def ddim_ref(x, uncond, cond, g, alpha_t, alpha_prev):
    s1, s2, s3, s4 = (float(v) for v in ddim_scalars(alpha_t, alpha_prev))
    x, un, co = (f64(f32(a)) for a in (x, uncond, cond))
    g = float(np.float32(g))
    ab = np.abs
    d = co - un
    gd = g * d
    e = un + gd
    Ee = 0.0 * e if g == 0 else abs(g) * U * ab(d) + (0.0 if _exact_mul(g) else U * ab(gd)) + U * ab(e)
    p = s1 * e
    Ep = s1 * Ee + (0.0 if _exact_mul(s1) else U * ab(p))
    t = x - p
    Et = Ep + (0.0 if s1 == 0 else U * ab(t))
    x0 = t / s2
    Ex0 = Et / s2 + (0.0 if _exact_mul(s2) else U * ab(x0))
    a_, b_ = s3 * x0, s4 * e
    Ea = s3 * Ex0 + (0.0 if _exact_mul(s3) else U * ab(a_))
    Eb = s4 * Ee + (0.0 if _exact_mul(s4) else U * ab(b_))
    out = a_ + b_
    return out, (Ea + Eb + (0.0 if s4 == 0 else U * ab(out))) * SECOND_ORDER


def ddim_emu(x, uncond, cond, g, alpha_t, alpha_prev, fused=True, mutant=None):
    s1, s2, s3, s4 = ddim_scalars(alpha_t, alpha_prev)
    if mutant == "s1 / s4 swapped":
        s1, s4 = s4, s1
    x, un, co, g = f32(x), f32(uncond), f32(cond), np.float32(g)
    r = lambda v: np.asarray(v).astype(np.float32)
    if mutant == "g applied to cond only":
        e = r(un + r(g * co))
    else:
        e = _fma(g, r(co - un), un) if fused else r(un + r(g * r(co - un)))
    x0 = r((_fma(-s1, e, x) if fused else r(x - r(s1 * e))) / s2)
    return _fma(s3, x0, r(s4 * e)) if fused else r(r(s3 * x0) + r(s4 * e))


def ddim_cases():
    c = {}
    k = 0
    for n, g, a_t, a_prev in ((1, 7.5, 0.6, 0.8), (257, 1.0, 0.9991, 0.99951), (257, 0.0, 0.0047, 0.0291), (4 * 24 * 24, 7.5, 0.0047, 0.0291), (4 * 24 * 24, 7.5, 0.37, 0.52),
                              (257, 7.5, 0.9991, 1.0), (4 * 24 * 24, 1.0, 0.5, 1.0), (4 * 24 * 24, 3.0, 0.001, 0.0047)):
        rs = _rs(90 + k)
        k += 1
        un = rs.standard_normal(n)
        cs = dict(x=rs.standard_normal(n).astype(np.float32), uncond=un.astype(np.float32), cond=(un + 0.2 * rs.standard_normal(n)).astype(np.float32))
        if n == 1:      # one element is no sample of anything: written out, without a cancellation, so that its B and median (that element's own) say something
            cs = dict(x=np.float32([0.7]), uncond=np.float32([-0.3]), cond=np.float32([-0.2]))
        c[f"n {n}, g {g}, alpha_t {a_t}, alpha_prev {a_prev}"] = dict(cs, g=g, alpha_t=a_t, alpha_prev=a_prev)
    return c


# ------------------------------------------------------------------------------------------------------------------ every case through one door
def all_cases(run):
    """Runs every committed case through `run`: run(op, name, case, **what) -> fp32 result of the engine (or of an emulation).  Yields (op, name, shape, got, ref, E)."""
    for name, cs in blend_cases().items():
        res = run_blend_case(cs, lambda tiles, wi, wj, acc, prior: run("blend", name, cs, tiles=tiles, wi=wi, wj=wj, accumulate=acc, prior=prior))
        for k, (got, ref, E) in enumerate(res):
            yield "blend", name + (f" [launch {k + 1}]" if len(res) > 1 else ""), ref.shape, got, ref, E
    for name, cs in regions_cases().items():
        ref, E = regions_ref(cs["wins"], cs["desc"], cs["C"], cs["size"], cs["h"], cs["w"])
        yield "regions", name, ref.shape, run("regions", name, cs), ref, E
    for name, cs in normalise_cases().items():
        ref, E = normalise_ref(cs["canvas"], cs["scale"])
        yield "normalise", name, ref.shape, run("normalise", name, cs), ref, E
    for name, cs in resample_cases().items():
        ref, E = resample_ref(cs["x"], cs["ty"], cs["tx"])
        yield "resample", name, ref.shape, run("resample", name, cs), ref, E
    for stats in ELEV_STATS:
        packed, low, mean, std = elev_inputs(stats)
        cs = dict(packed=packed, low=low, mean=mean, std=std)
        ref, E = elev_ref(packed, low, mean, std)
        yield "residual_plus", f"mean {mean} std {std}, 19x23", ref.shape, run("residual_plus", "", cs), ref, E
        for cname, crop in ELEV_CROPS.items():
            ref, E = elev_ref(packed, low, mean, std, crop)
            yield "elev_finish", f"mean {mean} std {std}, crop {cname} {crop}", ref.shape, run("elev_finish", cname, cs, crop=crop), ref, E
    for name, cs in climate_cases().items():
        ref, E = climate_ref(cs["feats"], cs["elev"], *climate_args(cs))
        yield "climate", name, ref.shape, run("climate", name, cs), ref, E
    for name, cs in ddim_cases().items():
        ref, E = ddim_ref(cs["x"], cs["uncond"], cs["cond"], cs["g"], cs["alpha_t"], cs["alpha_prev"])
        yield "ddim", name, ref.shape, run("ddim", name, cs), ref, E


def emulate(op, name, cs, fused=True, mutant=None, **kw):
    """the fp32 emulation of any op, in the signature `all_cases` calls"""
    if op == "blend":
        return blend_emu(kw["tiles"], cs["C"], cs["Hc"], cs["Wc"], cs["size"], cs["rows"], cs["cols"], kw["wi"], kw["wj"], kw["accumulate"], kw["prior"], mutant)
    if op == "regions":
        return regions_emu(cs["wins"], cs["desc"], cs["C"], cs["size"], cs["h"], cs["w"], mutant)
    if op == "normalise":
        return normalise_emu(cs["canvas"], cs["scale"], mutant)
    if op == "resample":
        return resample_emu(cs["x"], cs["ty"], cs["tx"], mutant)
    if op == "residual_plus":
        return elev_emu(cs["packed"], cs["low"], cs["mean"], cs["std"], None, fused, mutant)
    if op == "elev_finish":
        return elev_emu(cs["packed"], cs["low"], cs["mean"], cs["std"], kw["crop"], fused, mutant)
    if op == "climate":
        return climate_emu(cs["feats"], cs["elev"], *climate_args(cs), fused=fused, mutant=mutant)
    if op == "ddim":
        return ddim_emu(cs["x"], cs["uncond"], cs["cond"], cs["g"], cs["alpha_t"], cs["alpha_prev"], fused, mutant)
    raise KeyError(op)
