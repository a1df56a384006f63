"""Float64 twin of score scaling in the solver step and of the overlap blend with a caller's window; the criterion they are held to.

Score scaling (`scale_score`, csrc/td_device.h; the reference's `_scale_score`): in step i the guided-or-plain model output f becomes, at the current sample x,
      v = -sd f;  x0 = x c - v s;  np = x s + v c;  x0a = x + alpha (x0 - x);  va = np c - x0a s;  f' = va / (-sd)
in fp32, one rounding per operation (the kernel turns contraction off), with (c, s) = (cos t_i, sin t_i) fp32 scalars from the host.  `score_ref` evaluates the six
lines in float64 from the stored fp32 operands together with a bound E per element; u = 2^-24 per rounding, each with the modulus of its own term, so that the
cancellation in x0 - x at large sigma (x ~ sigma, x0 ~ sd) is covered by the terms that cancel and not by the small result:
      v   = nsd f                          E(v)   = |nsd| E(f) + u |v|                                  (nsd = -sd; E(f): the guide mix's bound, 0 without a guide)
      x0  = x c - v s                      E(x0)  = u |x c| + |s| E(v) + u |v s| + u |x0|
      np  = x s + v c                      E(np)  = u |x s| + |c| E(v) + u |v c| + u |np|
      d   = x0 - x                         E(d)   = E(x0) + u |d|
      x0a = x + alpha d                    E(x0a) = |alpha| E(d) + u |alpha d| + u |x0a|
      va  = np c - x0a s                   E(va)  = |c| E(np) + u |np c| + |s| E(x0a) + u |x0a s| + u |va|
      f'  = va / nsd                       E(f')  = E(va) / |nsd| + u |f'|
14 roundings.  Everything is multiplied by 1 + 2^-10 for the products of two roundings; a build that contracted a product into the following add would round once
where two are counted and stays inside.  E(f') then enters the solver step: tests/_sampler_twin.py's `step_ref` is evaluated on the float64 f' without a guide (its
own E(f) = 0), and the linear carry of E(f') through dpm_update, `carry(k)` (the coefficients E(f) has in step_ref's lines), is added.  test_sampler_args_cpu.py
checks `carry` against step_ref's own guided bound, so the two cannot drift apart.

Criterion A, every element of x_new and of the new m1: |hip - ref| <= E.  The fp32 emulation (`emulate`, numpy, no contraction in the score lines, dpm_update as
_sampler_twin.emulate_update spells it) reaches EMU_WORST_A of the bound.
Cap, per step: median(E / scale) <= CAP_SS.  The project's cap for the plain step is 16 u = one u per rounding on the longest path of dpm_update with a guide (guide
mix 3, m0 2, base 2, d10 2, d11 2, dd 1, d1 1, d2 1, x_new 2); the score lines add 14 roundings in front of it: (16 + 14) u = 30 u by the rounding count.  That
count assumes that no rounding is amplified, and the scaled step is ill-conditioned by construction in two places.  (1) At large sigma |x| ~ sigma >> |x0| ~ sd, so
in x0a = x + alpha (x0 - x) the roundings that carry |x|-sized terms land on a result of size |1 - alpha| |x|: relative (2 |alpha| + |1 - alpha|) / |1 - alpha| u
(23 u at alpha 1.1), which f' ~ x0a s / sd and m0 ~ c_out f' inherit: the float64 bound's median E / |m0| reaches 35.3 u on the CPU emulation's cases.  (2) A scaled
trajectory overshoots (m0 ~ (1 - alpha) x + alpha x0), so a x - b0 m0 itself cancels in some steps (order 1, alpha 1.3, sigma 24 -> 5.8: median E / |x_new| = 129 u
with every element inside A and the emulation at 0.6 of the bound).  So 30 u would refuse the twin's own bound, and no count of roundings caps (2).  The cap
therefore follows tests/_tile_twin.py's rule instead: scale = |m0| for the new m1 and |a x| + |b0 m0| (the two terms of dpm_update's `base`) for x_new, and
CAP_SS = 1.5 x the largest median the float64 bound has over the CPU test's cases (re-measured and asserted there): it keeps A from going vacuous, which is its job.
Criterion B, per step: rms(hip - ref) / rms(ref) <= C_RMS_SS (C_RMS_SS_GUIDED with a guide) = 4 x the worst value the emulation gives over the CPU test's cases
(test_sampler_args_cpu.py re-measures and asserts 4 worst <= C <= 4.2 worst).  Never taken from a GPU kernel.
Exact hand-offs: those of tests/_sampler_twin.py, unchanged (check_step is reused), which includes xin[..., C:Cin] == RNE_T(cond_img) in the main and the guide plan.

Blend with a caller's window: `blend_ref` is tests/_tile_twin.py's float64 blend (its `_add_window`, same order, same bound E = u sum_k |s_k|) with the stored fp32
window in place of the recomputed linear one, judged by that file's `judge` / `verdict("blend", .)`: A, B, the cap and the exact zeros as stated there.

Measured on the committed goldens (tests/golden/make_sampler_args_golden.py, CPU): rel-RMS of the reference's own fp32 run against its float64 run, e_ref =
5.96e-7 plain, 6.65e-7 guided 1.5, 5.42e-7 alpha 1.1, 8.70e-7 alpha 1.3, 5.86e-7 guided 1.5 with alpha 1.1: the new cases are as well conditioned as the plain one
and keep the project's 1e-5 fp32-mode bound.  On the MI355X the engine's fp32 mode is 9.2e-7 / 9.9e-7 / 6.6e-7 / 5.3e-7 / 7.6e-7 from those goldens; bf16 mode, end to end
(printed by test_sampler_args_gpu.py, only the guided alpha = 1 case asserted, < 3e-2): 6.96e-3 plain, 6.93e-3 guided, 4.09e-3 alpha 1.1, 2.98e-3 alpha 1.3, 5.19e-3
guided with alpha 1.1.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_twin as tw   # noqa: E402
import _tile_twin as tt      # noqa: E402

U = tw.U
SECOND_ORDER = tw.SECOND_ORDER
ROUNDINGS_SS = 14
# measured by test_sampler_args_cpu.py::test_fp32_emulation_passes_and_sets_the_constants on its cases (fp32 emulation, CPU):
EMU_WORST_A = 0.991         # worst |emulation - ref| / E
MEDIAN_WORST = 57.78 * U    # largest median E / scale over the steps of those cases
CAP_SS = 86.7 * U          # 1.5 x MEDIAN_WORST
C_RMS_SS = 95.5 * U         # 4 x 23.76 u, worst per-step rel-RMS without a guide (order 1, alpha 1.3, the cancelling step)
C_RMS_SS_GUIDED = 89.8 * U  # 4 x 22.34 u with a guide
ALPHAS = (0.8, 1.1, 1.3)


def score_table(sigmas, sigma_data):
    """the package's own (cos t_i, sin t_i) table: (n_steps, 2) fp32"""
    from terrain_diffusion_amd.sampling import score_scaling_table
    return score_scaling_table(sigmas, sigma_data)


def guide_mix_ref(F, Fg, gscale):
    """float64 f = g + s (F - g) with step_ref's bound for it (tests/_sampler_twin.py, `guide mix`)"""
    F = np.asarray(F, np.float64)
    if Fg is None:
        return F, np.zeros_like(F)
    g, s = np.asarray(Fg, np.float64), float(np.float32(gscale))
    sd = s * (F - g)
    f = g + sd
    return f, 2 * U * np.abs(sd) + U * np.abs(f)


def score_ref(alpha, c, s, sigma_data, x, f, Ef=0.0):
    """float64 scale_score on fp32 operands; alpha, c, s, sigma_data are taken as the fp32 values the kernel gets.  Returns (f', E(f')) -- E first order, NOT yet
    multiplied by 1 + 2^-10 (the caller does, once, after the carry through the step)."""
    ab = np.abs
    alpha, c, s, nsd = (float(np.float32(v)) for v in (alpha, c, s, -np.float32(sigma_data)))
    x, f = np.asarray(x, np.float64), np.asarray(f, np.float64)
    v = nsd * f
    Ev = ab(nsd) * Ef + U * ab(v)
    xc, vs, xs, vc = x * c, v * s, x * s, v * c
    x0 = xc - vs
    E0 = U * ab(xc) + ab(s) * Ev + U * ab(vs) + U * ab(x0)
    npr = xs + vc
    En = U * ab(xs) + ab(c) * Ev + U * ab(vc) + U * ab(npr)
    d = x0 - x
    Ed = E0 + U * ab(d)
    ad = alpha * d
    x0a = x + ad
    Ea = ab(alpha) * Ed + U * ab(ad) + U * ab(x0a)
    p1, p2 = npr * c, x0a * s
    va = p1 - p2
    Eva = ab(c) * En + U * ab(p1) + ab(s) * Ea + U * ab(p2) + U * ab(va)
    out = va / nsd
    return out, Eva / ab(nsd) + U * ab(out)


def carry(k):
    """(coefficient of E(f) in step_ref's E_x, in its E_m0) for the coefficient row k: the lines of step_ref that carry E(f), read off term by term"""
    ab = abs
    g0 = ab(k["c_out"])
    gb = ab(k["b0"]) * g0
    order = int(k["order"])
    if order == 1:
        return gb, g0
    if order == 2:
        return ab(0.5 * k["b0"]) * ab(k["inv_r0"]) * g0 + gb, g0
    g10 = ab(k["inv_r0"]) * g0
    g1 = ab(k["f01"]) * g10 + g10
    g2 = ab(k["inv_r01"]) * g10
    return ab(k["c2"]) * g2 + ab(k["c1"]) * g1 + gb, g0


def step_ss_ref(k, ss, x, F, m1, m2, Fg=None, gscale=None):
    """float64 guide mix -> scale_score -> dpm_update on fp32 operands.  ss = (alpha, c, s, sigma_data).  Returns dict(x, m0, E_x, E_m0, f)"""
    f, Ef = guide_mix_ref(F, Fg, gscale)
    fp, Efp = score_ref(ss[0], ss[1], ss[2], ss[3], x, f, Ef)
    r = tw.step_ref(k, x, fp, m1, m2)
    gx, gm = carry(k)
    scale_x = np.abs(k["a"] * np.asarray(x, np.float64)) + np.abs(r["terms"]["b0 m0"])
    return dict(x=r["x"], m0=r["m0"], E_x=r["E_x"] + gx * Efp * SECOND_ORDER, E_m0=r["E_m0"] + gm * Efp * SECOND_ORDER, f=fp, scale_x=scale_x)


def emulate_score(alpha, c, s, sigma_data, x, f, mutant=None):
    """scale_score in numpy fp32, one rounding per operation.  `mutant` breaks one thing (test_sampler_args_cpu.py)."""
    f32 = np.float32
    alpha, c, s, nsd = f32(alpha), f32(c), f32(s), -f32(sigma_data)
    if mutant == "c and s swapped":
        c, s = s, c
    x, f = np.asarray(x, f32), np.asarray(f, f32)
    v = (-nsd if mutant == "sign of v" else nsd) * f
    x0 = x * c - v * s
    npr = x * s + v * c
    if mutant == "alpha on the noise prediction":
        npr = x + alpha * (npr - x)
        x0a = x0
    else:
        x0a = x + alpha * (x0 - x)
    va = npr * c - x0a * s
    return (va / nsd).astype(f32)


def emulate(k, ss, x, F, m1, m2, Fg=None, gscale=None, mutant=None):
    """the scaled step in numpy fp32: (x_new, m0)"""
    f32 = np.float32
    x, F = np.asarray(x, f32), np.asarray(F, f32)
    if mutant == "scaled before the guide mix" and Fg is not None:
        F2 = emulate_score(ss[0], ss[1], ss[2], ss[3], x, F)
        g2 = emulate_score(ss[0], ss[1], ss[2], ss[3], x, np.asarray(Fg, f32))
        f = g2 + f32(gscale) * (F2 - g2)
    else:
        f = F if Fg is None else (np.asarray(Fg, f32) + f32(gscale) * (F - np.asarray(Fg, f32)))
        f = emulate_score(ss[0], ss[1], ss[2], ss[3], x, f, mutant)
    return tw.emulate_update(k, x, f, m1, m2)


def judge_step(k, ss, pre, post, Fg=None, gscale=None):
    """figures of one step from the states before / after it (arrays of one shape: x, m1, m2 before; F (and Fg) consumed; x, m1 after)"""
    r = step_ss_ref(k, ss, pre["x"], post["F"], pre["m1"], pre["m2"], Fg, gscale)
    st = {"order": int(k["order"]), "guided": Fg is not None, "elements": int(r["x"].size), "alpha": float(ss[0])}
    for what, got, ref, E, scale in (("x", post["x"], r["x"], r["E_x"], r["scale_x"]), ("m0", post["m1"], r["m0"], r["E_m0"], np.abs(r["m0"]))):
        err = np.abs(np.asarray(got, np.float64) - ref)
        ratio = err / np.maximum(E, 1e-300)
        st[f"A_{what}"] = float(np.max(ratio)) if np.all(np.isfinite(got)) else float("inf")
        st[f"B_{what}"] = float(np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(ref ** 2)))
        st[f"median_{what}"] = float(np.median(E / np.maximum(scale, 1e-300)))
    return st


def verdict(st):
    v = []
    cmax = C_RMS_SS_GUIDED if st["guided"] else C_RMS_SS
    for what in ("x", "m0"):
        if not st[f"A_{what}"] <= 1.0:
            v.append(f"A({what}): err / E = {st[f'A_{what}']:.3g}")
        if not st[f"B_{what}"] <= cmax:
            v.append(f"B({what}): {st[f'B_{what}'] / U:.2f} u > {cmax / U:.2f} u")
        if not st[f"median_{what}"] <= CAP_SS:
            v.append(f"cap({what}): median E / scale = {st[f'median_{what}'] / U:.1f} u > {CAP_SS / U:.1f} u")
    return v


def emu_cases():
    """the CPU test's cases: (name, sigma ladder, solver order, alpha, guided).  x0 = sigma_0 noise, toy models of tests/_sampler_twin.py; n 3, C 5, 8 x 8"""
    from oracle import schedule
    out = []
    for order in (1, 2, 3):
        for alpha in ALPHAS:
            for guided in (False, True):
                out.append((f"order {order}, alpha {alpha}" + (", guided 1.3" if guided else ""), schedule.karras_sigmas(6)[0].numpy(), order, alpha, guided))
    return out


def run_emu_case(sig, order, alpha, guided, mutant=None, sd=0.5, n=3, C=5, HW=64, seed=5):
    """chains the emulation over the ladder; every step is judged against step_ss_ref on the emulation's own stored operands.  Returns the list of step figures."""
    table = tw.engine_table(sig, sd, order, True)
    cs = score_table(sig, sd)
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((n, HW, C)) * float(sig[0])).astype(np.float32)
    m1 = m2 = np.zeros_like(x)
    model, guide = tw.toy_model(C, 3), tw.toy_model(C, 4, strength=0.8)
    stats = []
    for i in range(table.shape[0]):
        k = tw.row(table, i)
        c_in = np.float32(1.0) / np.sqrt(np.float32(sig[i]) ** 2 + np.float32(sd) ** 2)
        xin = (x * c_in).astype(np.float32)
        F = model(xin, i)
        Fg = guide(xin, i) if guided else None
        ss = (alpha, cs[i][0], cs[i][1], sd)
        xn, m0 = emulate(k, ss, x, F, m1, m2, Fg, 1.3 if guided else None, mutant)
        st = judge_step(k, ss, dict(x=x, m1=m1, m2=m2), dict(x=xn, m1=m0, F=F), Fg, 1.3 if guided else None)
        st["step"] = i
        stats.append(st)
        x, m1, m2 = xn, m0, (m1 if order == 3 else m2)
    return stats


# ------------------------------------------------------------------------------------------------------------------ blend with a stored window
def blend_ref(tiles, window, C, Hc, Wc, size, row_starts, col_starts, wi, wj, accumulate=0, prior=None):
    """float64 td_blend_windows_w on fp32 tiles (n, C, size, size) and the stored fp32 window (size, size) -> (canvas (C + 1, Hc, Wc), E): tests/_tile_twin.py's
    blend (its _add_window in ascending (row, col) window order, E = u sum_k |s_k|) with the caller's window in place of the recomputed linear one"""
    tiles, ww = tt.f32(tiles), tt.f32(window).reshape(size, size)
    tt._rowmap(Hc, row_starts, size)
    tt._rowmap(Wc, col_starts, size)
    tile_of = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(wi, wj))}
    acc = np.zeros((C + 1, Hc, Wc), np.float64)
    if accumulate:
        acc[:] = prior
    Es = np.zeros_like(acc)
    for ic, rs in enumerate(row_starts):
        for jc, cs in enumerate(col_starts):
            slot = tile_of.get((ic, jc), -1)
            if slot >= 0:
                tt._add_window(acc, Es, tiles[slot], ww, int(rs), int(cs), size, False)
    return acc, Es * U * SECOND_ORDER
