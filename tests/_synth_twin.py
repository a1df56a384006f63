"""Float64 twin of the synthetic conditioning map (`perlin_map_kernel` in csrc/compose_kernels.hip through td_perlin_map), its bound, the committed cases and an
fp32 CPU emulation.  Layout and criterion are those of tests/_tile_twin.py (A on every element, B and the cap per case); `judge` is that file's.

The specification.  What is exact or an fp32 chain of the kernel is taken as it is spelled, everything else is evaluated in float64 and its roundings are counted:
  coordinates   x = fl(fl(i1 + r) frequency), y = fl(fl(j1 + c) frequency) (int -> fp32, then one product), then x = fl(x lacunarity) per octave (exact for a power of
                two): this fp32 chain IS the coordinate.  floor, (int) and the wrapped 32-bit hash h = (seed ^ xp ^ yp) * 0x27d4eb2d, h ^= h >> 15, h & 127 are exact.
  amplitudes    bound = 1 + |g| + |g|^2 + ... and amp = fl(1 / bound), amp = fl(amp g) in fp32 as spelled (the divide is HIP's correctly rounded one).
  gradient      the angle is a = fl(k c1 + c2), k = h & 127, c1 = fl(2 pi) / 128, c2 = fl(pi) / 128: ONE rounding.  The source spells a product and a sum; the build
                contracts them (the gfx950 code of the loop is v_fmamk_f32 v, k, 0x3d490fdb, c2, then v_mul_f32 by 1 / (2 pi), then v_cos_f32 / v_sin_f32; read once from
                `hipcc --offload-arch=gfx950 -O3 -S`), and tests/sincos_probe.hip, built with the same flags, returns these angles bit for bit on the device
                (asserted by the GPU test).  A build that stops fusing there moves 30 of the 128 angles by an ulp and fails, on purpose.
                The gradient is (cos a, sin a) in float64.  The kernel calls the device's fast __cosf / __sinf, whose absolute error is neither derivable nor documented:
                it is MEASURED, exhaustively, by the probe kernel at the 128 angles against float64: EPS_SINCOS = 3.93e-7 (cos 3.62e-7 at k = 109, sin 3.93e-7 at
                k = 123; tests/golden/sincos_gfx950.npz keeps the returned table, the GPU test measures again and prints).  E uses SINCOS_MARGIN = 2 x that value, the
                margin for a different lowering by a later compiler.
  noise         xd0 = x - floor(x) [one rounding unless exact, checked per element], xd1 = xd0 - 1 [one], the quintic fade, four dots, three lerps, the scale
                1.4247691 and sum += n amp: every product and every add one rounding u |result| on top of the propagated operand errors (the unfused count; it
                contains the fused one).  The first octave's add to 0 is exact.  On a lattice point xd0 = yd0 = 0 every term of the bound is 0: the noise is exactly 0.
  transfer      np.interp(sum, src, dst) with clamped ends, continuous and piecewise linear, so a sum the kernel has within E_sum of the twin's gives
                |out - ref| <= max |slope| E_sum + roundings over the intervals [s - E_sum, s + E_sum] touches: the larger adjacent slope when the sum is within E_sum
                of a knot; 0 beyond an end knot by more than E_sum (dst[0] / dst[-1] exactly); within E_sum of an end knot either branch is inside the bound.
                Roundings of dst[lo] + (s - src[lo]) ((dst[hi] - dst[lo]) / (src[hi] - src[lo])): one for s - src[lo], three relative in the slope, the product, the sum.

Constants below are measured by test_synth_ops_cpu.py on the fp32 emulation (`fbm_emu`: numpy fp32 in the kernel's order with the recorded device table for the
gradients, fused as the build fuses and unfused; the worst of both) and asserted there.
"""
import os

import numpy as np

from _tile_twin import SECOND_ORDER, U, _fma, f32, f64, judge  # noqa: F401  (judge is re-exported: one criterion)

OP = "synth"
EPS_SINCOS = 3.93e-7          # measured on the MI355X by tests/sincos_probe.hip (see above); the GPU test measures again and asserts SINCOS_MARGIN x it is not exceeded
SINCOS_MARGIN = 2.0
MAX_EXCLUDED = 0.0            # nothing here is non-finite
# measured by test_synth_ops_cpu.py::test_fp32_emulations_pass_and_set_the_constants
EMU_WORST_A = 0.776
MEDIAN_RANGE = (0.0, 1466.86)     # least and largest median E / |ref| in u over the cases
CAP = 2200.0                     # u
C_RMS = 198.7                   # u

PX, PY = 501125321, 1136930381
HASH = 0x27d4eb2d
C1 = np.float32(6.283185307179586) / np.float32(128)
C2 = np.float32(3.141592653589793) / np.float32(128)
SCALE = np.float32(1.4247691104677813)
GOLDEN_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sincos_gfx950.npz")


def _i32(x):
    return (np.asarray(x, dtype=np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31


def angles(fused=True):
    """the 128 fp32 gradient angles: fl(k c1 + c2) (the build) or fl(fl(k c1) + c2)"""
    k = np.arange(128, dtype=np.float32)
    return _fma(k, C1, C2) if fused else ((k * C1).astype(np.float32) + C2).astype(np.float32)


def device_table():
    """(cos, sin) fp32 as the MI355X returned them for `angles()` (recorded by the probe)"""
    t = np.load(GOLDEN_TABLE)
    return t["cos"], t["sin"]


def libm_table(fused=True):
    a = angles(fused)
    return np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)


def amplitudes(octaves, gain):
    g = np.float32(gain)
    bound, a = np.float32(1), np.abs(g)
    for _ in range(1, octaves):
        bound = np.float32(bound + a)
        a = np.float32(a * np.abs(g))
    amp = [np.float32(np.float32(1) / bound)]
    for _ in range(1, octaves):
        amp.append(np.float32(amp[-1] * g))
    return amp


def coordinates(first, count, frequency, octaves, lacunarity):
    """the fp32 coordinate of every octave along one axis"""
    v = ((np.int64(first) + np.arange(count, dtype=np.int64)).astype(np.float32) * np.float32(frequency)).astype(np.float32)
    out = [v]
    for _ in range(1, octaves):
        out.append((out[-1] * np.float32(lacunarity)).astype(np.float32))
    return out


def hash_index(seed, fx, fy, px=PX, py=PY):
    """k = h & 127 at the four corners of the cell (fx, fy) (fp32 floors, broadcast): dict (dx, dy) -> k"""
    x0, y0 = _i32(fx.astype(np.int64) * px), _i32(fy.astype(np.int64) * py)
    x1, y1 = _i32(x0 + px), _i32(y0 + py)
    out = {}
    for dx, xp in ((0, x0), (1, x1)):
        for dy, yp in ((0, y0), (1, y1)):
            h = _i32(_i32(_i32(seed) ^ xp ^ yp) * HASH)
            h = h ^ (h >> 15)
            out[(dx, dy)] = (h & 127).astype(np.int64)
    return out


# ------------------------------------------------------------------------------------------------------------------ float64 with a running bound
def _add(a, b):
    v = a[0] + b[0]
    return v, a[1] + b[1] + U * np.abs(v)


def _sub(a, b):
    return _add(a, (-b[0], b[1]))


def _mul(a, b):
    v = a[0] * b[0]
    return v, np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1] + U * np.abs(v)


def _k(c):
    return (float(c), 0.0)


def _frac(v32):
    """xd0 = x - floor(x) and xd1 = xd0 - 1 with their bounds (fp32 in: the coordinate chain)"""
    fl = np.floor(v32)
    d = f64(v32) - f64(fl)
    exact = f64((v32 - fl).astype(np.float32)) == d
    d0 = (d, np.where(exact, 0.0, U * np.abs(d)))
    return fl, d0, _sub(d0, _k(1))


def _fade(t):
    inner = _add(_mul(t, _sub(_mul(t, _k(6)), _k(15))), _k(10))
    return _mul(_mul(_mul(t, t), t), inner)


def fbm_sum(rows, cols, i1, j1, seed, frequency, octaves, lacunarity, gain):
    """(sum, E_sum) in float64 on the (rows, cols) window"""
    xs_, ys_ = coordinates(i1, rows, frequency, octaves, lacunarity), coordinates(j1, cols, frequency, octaves, lacunarity)
    amp = amplitudes(octaves, gain)
    a32 = f64(angles())
    cs, sn = np.cos(a32), np.sin(a32)
    et = SINCOS_MARGIN * EPS_SINCOS
    total = None
    for o in range(octaves):
        fx, xd0, xd1 = _frac(xs_[o][:, None])
        fy, yd0, yd1 = _frac(ys_[o][None, :])
        k = hash_index(int(_i32(seed + o)), fx, fy)
        g = lambda key, xd, yd: _add(_mul(xd, (cs[k[key]], et)), _mul(yd, (sn[k[key]], et)))
        a, b, c, d = g((0, 0), xd0, yd0), g((1, 0), xd1, yd0), g((0, 1), xd0, yd1), g((1, 1), xd1, yd1)
        fxs, fys = _fade(xd0), _fade(yd0)
        xf0 = _add(a, _mul(fxs, _sub(b, a)))
        xf1 = _add(c, _mul(fxs, _sub(d, c)))
        n = _mul(_add(xf0, _mul(fys, _sub(xf1, xf0))), _k(SCALE))
        t = _mul(n, _k(amp[o]))
        total = t if total is None else _add(total, t)
    shape = (rows, cols)
    return np.broadcast_to(total[0], shape).copy(), np.broadcast_to(total[1], shape) * SECOND_ORDER


def transfer_ref(s, Es, src, dst):
    """np.interp(s, src, dst) with clamped ends in float64 on the fp32 tables, and the bound for a sum within Es of s"""
    src, dst = f64(f32(src)), f64(f32(dst))
    out = np.interp(s, src, dst)
    slope = np.diff(dst) / np.diff(src)
    smax, rmax = np.zeros_like(s), np.zeros_like(s)
    for k in range(len(src) - 1):
        touched = (s + Es >= src[k]) & (s - Es <= src[k + 1])
        d = np.minimum(np.abs(np.clip(s, src[k], src[k + 1]) - src[k]) + Es, src[k + 1] - src[k])
        p = np.abs(slope[k]) * d
        v = np.abs(dst[k] + slope[k] * (np.clip(s, src[k], src[k + 1]) - src[k])) + np.abs(slope[k]) * Es
        R = U * p + 3 * U * p + U * p + U * v
        smax = np.where(touched, np.maximum(smax, np.abs(slope[k])), smax)
        rmax = np.where(touched, np.maximum(rmax, R), rmax)
    return out, (smax * Es + rmax) * SECOND_ORDER


def fbm_ref(rows, cols, i1, j1, seed, frequency, octaves, lacunarity, gain, src, dst):
    """float64 td_perlin_map -> (out, E, dict(sum, E_sum))"""
    s, Es = fbm_sum(rows, cols, i1, j1, seed, frequency, octaves, lacunarity, gain)
    out, E = transfer_ref(s, Es, src, dst)
    return out, E, dict(sum=s, E_sum=Es)


# ------------------------------------------------------------------------------------------------------------------ the fp32 emulation
def fbm_emu(rows, cols, i1, j1, seed, frequency, octaves, lacunarity, gain, src, dst, fused=True, table=None, mutant=None):
    """perlin_map_kernel in numpy fp32, thread by thread (flat index i, r = i / cols, c = i % cols); table = (cos, sin) fp32 at the 128 angles (default: the device's)"""
    o32 = np.float32
    r = lambda v: np.asarray(v).astype(np.float32)
    cs, sn = device_table() if table is None else table
    fma = _fma if fused else (lambda a, b, c: r(r(a * b) + c))
    i = np.arange(rows * cols, dtype=np.int64)
    if mutant == "rows / cols transposed":
        rr, cc = i % rows, i // rows
    else:
        rr, cc = i // cols, i % cols
    x = r(r(i1 + rr) * o32(frequency))
    y = r(r((i1 if mutant == "i1 added to the column" else j1) + cc) * o32(frequency))
    amp = amplitudes(octaves, gain)
    if mutant == "amplitude not divided by the bound":
        amp = [o32(a / amp[0]) for a in amp]
    if mutant == "lacunarity applied before the first octave":
        x, y = r(x * o32(lacunarity)), r(y * o32(lacunarity))
    px, py = (PY, PX) if mutant == "coordinate primes swapped" else (PX, PY)
    total = np.zeros(rows * cols, np.float32)
    for o in range(octaves):
        fx, fy = (np.trunc(x), np.trunc(y)) if mutant == "trunc for floor" else (np.floor(x), np.floor(y))
        xd0, yd0 = r(x - fx), r(y - fy)
        xd1, yd1 = r(xd0 - o32(1)), r(yd0 - o32(1))
        if mutant == "smoothstep fade":
            fade = lambda t: r(r(t * t) * r(o32(3) - r(o32(2) * t)))
        else:
            fade = lambda t: r(r(r(t * t) * t) * fma(t, fma(t, o32(6), o32(-15)), o32(10)))
        k = hash_index(int(_i32(seed if mutant == "seed not advanced per octave" else seed + o)), fx, fy, px, py)
        g = lambda key, xd, yd: fma(yd, sn[k[key]], r(xd * cs[k[key]]))
        a, b, c, d = g((0, 0), xd0, yd0), g((1, 0), xd1, yd0), g((0, 1), xd0, yd1), g((1, 1), xd1, yd1)
        fxs, fys = fade(xd0), fade(yd0)
        xf0, xf1 = fma(fxs, r(b - a), a), fma(fxs, r(d - c), c)
        n = r(fma(fys, r(xf1 - xf0), xf0) * SCALE)
        total = fma(n, amp[o], total)
        x, y = r(x * o32(lacunarity)), r(y * o32(lacunarity))
    src, dst = f32(src), f32(dst)
    nq = len(src)
    hi = np.clip(np.searchsorted(src, total, side="right"), 1, nq - 1)      # the binary search: the last knot <= sum
    lo = hi - 1
    ls, hs = (np.clip(lo + 1, 0, nq - 2), np.clip(hi + 1, 1, nq - 1)) if mutant == "slope from the neighbouring interval" else (lo, hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = r(r(dst[hs] - dst[ls]) / r(src[hs] - src[ls]))
    v = fma(r(total - src[lo]), slope, dst[lo])
    v = np.where(total <= src[0], dst[0], np.where(total >= src[-1], dst[nq - 2] if mutant == "right clamp returns dst[nq - 2]" else dst[-1], v))
    return r(v).reshape(rows, cols)


# ------------------------------------------------------------------------------------------------------------------ the cases
def identity_table(nq):
    t = np.linspace(-1.0, 1.0, nq).astype(np.float32)
    return t, t.copy()


FACTORY_PARAMS = [(0.05 * m, o, 2.0, 0.5) for m, o in ((1.5, 4), (3, 2), (3, 4), (3, 4), (3, 4))]   # today's test: frequency_mult (1.5, 3, 3, 3, 3)
_STATS = {}


def default_stats():
    """the factory's default statistics, made on the CPU: its data tables as they are, its noise tables the way it measures them (the stride-32 call, seeds 1 .. 5,
    synthetic_map.py:_build_quantiles) on 256 x 256 samples of the emulation.  -> [(src, dst)] fp32 per channel"""
    if not _STATS:
        from terrain_diffusion_amd.synthetic_map import _build_quantiles, _default_targets
        ident = identity_table(64)
        tabs = []
        for ch, ((f, o, l, g), tgt) in enumerate(zip(FACTORY_PARAMS, _default_targets())):
            raw = fbm_emu(256, 256, 0, 0, ch + 1, np.float32(f * 32), o, l, g, *ident)
            tabs.append((_build_quantiles(raw.ravel(), 64, 1e-4).astype(np.float32), np.asarray(tgt).astype(np.float32)))
        _STATS["t"] = tabs
    return _STATS["t"]


def knot_table(args):
    """an identity-like table with three knots moved onto sums of the case's own float64 twin (rounded to fp32, the table's type)"""
    s, _ = fbm_sum(*args)
    src = np.linspace(-1.0, 1.0, 64).astype(np.float32)
    picks = np.sort(s.ravel()[[5, s.size // 2, s.size - 7]].astype(np.float32))
    for p in picks:
        j = int(np.argmin(np.abs(src - p)))
        src[j] = p
    src = np.unique(src)
    assert len(src) == 64 and np.all(np.diff(src) > 0)
    dst = (np.cumsum(np.linspace(0.5, 3.0, 64)) - 30.0).astype(np.float32)
    return src, dst, picks


def cases():
    """name -> dict(args = (rows, cols, i1, j1, seed, frequency, octaves, lacunarity, gain), src, dst)"""
    c = {}
    st = default_stats()

    def case(name, rows, cols, i1, j1, seed, freq, octaves, lac, gain, table):
        c[name] = dict(args=(rows, cols, i1, j1, seed, freq, octaves, lac, gain), src=table[0], dst=table[1])
    case("1x1 at (13, -5), f 0.05, 4 octaves, identity 64", 1, 1, 13, -5, 11, 0.05, 4, 2.0, 0.5, identity_table(64))
    case("1x257 at (0, 0), f 0.075, 2 octaves, identity 65", 1, 257, 0, 0, 12, 0.075, 2, 2.0, 0.5, identity_table(65))
    case("3x300 straddling 0 at (-3, -3), f 0.05, 4 octaves, identity 64", 3, 300, -3, -3, 13, 0.05, 4, 2.0, 0.5, identity_table(64))
    for ch, (f, o, l, g) in enumerate(FACTORY_PARAMS):
        case(f"50x70 at (-37, 1200), default stats channel {ch}, f {f:g}, {o} octaves", 50, 70, -37, 1200, 78 + ch, f, o, l, g, st[ch])
    case("20x70 at (2^20, -2^20), f 0.05, 4 octaves, identity 64", 20, 70, 2 ** 20, -2 ** 20, 14, 0.05, 4, 2.0, 0.5, identity_table(64))
    case("20x70 at (-2^20, 2^20), f 0.05, 6 octaves, gain 0.35, identity 64", 20, 70, -2 ** 20, 2 ** 20, 15, 0.05, 6, 2.0, 0.35, identity_table(64))
    case("30x40 at (0, 0), f 1.6 (the stride-32 call), 4 octaves, identity 64", 30, 40, 0, 0, 1, 1.6, 4, 2.0, 0.5, identity_table(64))
    case("9x11 at (-3, -3), f 0.5, 2 octaves: lattice and half points, default stats channel 1", 9, 11, -3, -3, 16, 0.5, 2, 2.0, 0.5, st[1])
    case("9x11 at (-3, -3), f 1.0, 4 octaves: every point on the lattice, default stats channel 0", 9, 11, -3, -3, 17, 1.0, 4, 2.0, 0.5, st[0])
    case("17x33 at (-37, 1200), f 0.075, 1 octave, nq 2", 17, 33, -37, 1200, 18, 0.075, 1, 2.0, 0.5, identity_table(2))
    case("17x33 at (5, -40), f 0.075, 2 octaves, nq 3", 17, 33, 5, -40, 19, 0.075, 2, 2.0, 0.5, (np.float32([-1, 0.1, 1]), np.float32([-5, 0, 20])))
    case("23x37 at (-3, -3), f 0.05, 4 octaves, lacunarity 2.5, gain 0.35, identity 64", 23, 37, -3, -3, 20, 0.05, 4, 2.5, 0.35, identity_table(64))
    narrow = np.linspace(-0.1, 0.1, 64).astype(np.float32)
    case("40x60 at (-37, 1200), f 0.075, 4 octaves, source range narrower than the noise", 40, 60, -37, 1200, 21, 0.075, 4, 2.0, 0.5, (narrow, st[0][1]))
    wide = np.linspace(-2.0, 2.0, 64).astype(np.float32)
    case("40x60 at (-37, 1200), f 0.075, 4 octaves, source range wider than the noise", 40, 60, -37, 1200, 21, 0.075, 4, 2.0, 0.5, (wide, st[0][1]))
    args = (24, 50, -12, 7, 22, 0.075, 4, 2.0, 0.5)
    src, dst, _ = knot_table(args)
    case("24x50 at (-12, 7), f 0.075, 4 octaves, three knots on sums of the twin", *args, (src, dst))
    return c


N_CASES = 19


def run_cases(run):
    """run(name, case) -> fp32 map; yields (name, shape, got, ref, E, info)"""
    for name, cs in cases().items():
        ref, E, info = fbm_ref(*cs["args"], cs["src"], cs["dst"])
        yield name, ref.shape, run(name, cs), ref, E, info


def verdict(st):
    v = []
    if not st["masks_ok"]:
        v.append("non-finite masks differ")
    if not st["A"] <= 1.0:
        v.append(f"A: err / E = {st['A']:.3g} at {st['at']}")
    if not st["B"] <= C_RMS * U:
        v.append(f"B: {st['B'] / U:.3f} u > {C_RMS:.3f} u")
    if not st["median"] <= CAP * U:
        v.append(f"cap: median E / |ref| = {st['median'] / U:.2f} u > {CAP:.2f} u")
    if not st["excluded"] <= MAX_EXCLUDED:
        v.append(f"{100 * st['excluded']:.2f} % non-finite")
    return v


def line(name, shape, st):
    return (f"{OP} | {name} | {shape}: worst err / E {st['A']:.3f}, B {st['B'] / U:.3f} u (<= {C_RMS:.3f}), median E / |ref| {st['median'] / U:.2f} u "
            f"(cap {CAP:.2f}), non-finite {100 * st['excluded']:.2f} %")
