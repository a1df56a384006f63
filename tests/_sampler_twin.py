"""Float64 twin of the solver step and of the sampler's hand-offs, and the criterion they are held to.

What is checked.  One DPM-Solver++ step of the engine is `dpm_update` (csrc/td_device.h), run either by `dpm_step_kernel` or by the EPI_DPM_STEP branch of the conv
epilogue, on fp32 operands the engine keeps: the sample x, the histories m1 / m2, the model output F (and the guide's) and 13 fp32 scalars per step that the host
derives from the sigma ladder (`dpm_coefs`, read through td_dpm_coefs).  With the engine option "sampler_stop_after" = k the state after k steps of an n-step run can be
read back ("@x", "@m1", "@m2", "@xin", "out_conv"), so two runs (k and k + 1) give every input and every output of step k.  `step_ref` evaluates the same update in
float64 from those stored fp32 operands, term by term, together with a bound E per element.

Criterion A, every element of x_new and of the new m1:   |hip - ref| <= E.
  E counts the fp32 roundings of dpm_update as it is spelled, u = 2^-24 per rounding, one rounding per fused multiply-add (standard model fl(a op b) =
  (a op b)(1 + d), |d| <= u; nothing here is near the subnormal range).  Each quantity below is the float64 value, E(.) the bound of its computed counterpart:
      guide mix   f = g + s (F - g):  d = F - g [u|d|], s d [u|s d|], g + s d [u|f|]              E(f)  = 2 u |s d| + u |f|        (0 without a guide; a compiler
                                                                                                  that fuses the last two roundings stays inside)
      m0   = fma(c_skip, x, c_out f)      E(m0)   = |c_out| E(f) + u |c_out f| + u |m0|
      base = fma(a, x, -(b0 m0))          E(base) = |b0| E(m0) + u |b0 m0| + u |base|
      order 1: x_new = base
      order 2: q = inv_r0 (m0 - m1)       E(q)    = |inv_r0| (E(m0) + u |m0 - m1|) + u |q|
               x_new = fma(-0.5 b0, q, base)      E = |0.5 b0| E(q) + E(base) + u |x_new|         (0.5 b0 is exact)
      order 3: d10 = inv_r0 (m0 - m1)     E(d10)  = |inv_r0| (E(m0) + u |m0 - m1|) + u |d10|
               d11 = inv_r1 (m1 - m2)     E(d11)  = |inv_r1| u |m1 - m2| + u |d11|
               dd  = d10 - d11            E(dd)   = E(d10) + E(d11) + u |dd|
               d1  = fma(f01, dd, d10)    E(d1)   = |f01| E(dd) + E(d10) + u |d1|
               d2  = inv_r01 dd           E(d2)   = |inv_r01| E(dd) + u |d2|
               x_new = fma(-c2, d2, fma(c1, d1, base))   E = |c2| E(d2) + |c1| E(d1) + E(base) + u |fma(c1, d1, base)| + u |x_new|
  These are first-order counts; every E is multiplied by 1 + 2^-10 for the products of two roundings (each is below u times a first-order term).  The fp32 CPU emulation
  of dpm_update (`emulate_update`, FMAs formed in float64 and rounded once) reaches EMU_WORST_A of the bound, so it is tight, and nothing is added to it.
  Cap, asserted per step: median(E / |ref|) <= CAP = 16 u.  The emulation's cases give MEDIAN_RANGE: A cannot go vacuous.

Criterion B, per step:   rms(hip - ref) / rms(ref) <= C_RMS_STEP (C_RMS_STEP_GUIDED with a guide model) = 4 x the worst value the emulation gives over the CPU
  test's unguided (guided) cases (test_sampler_ops_cpu.py re-measures and asserts 4 worst <= C <= 4.2 worst).  Never taken from a GPU kernel.

Exact hand-offs (torch.equal, every storage type T):  history shift m2_new == m1_old (order-3 runs; otherwise m2 stays as it was); after a non-last step
  xin[..., :C] == RNE_T(fl32(x_new c_in_next)) from the engine's own stored x_new; xin[..., C:Cin] == RNE_T(cond_img); xin[..., Cin] == 1; channels above Cin == 0; after
  the last step xin is what it was; the guide plan's xin equals the main plan's; at k = 0 xin[..., :C] == RNE_T(fl32(x c_in0)), m1 == m2 == 0.

Coefficient table: `coef_ref` restates dpmsolver.py's formulae (as oracle/schedule.py spells them) in float64 on the fp32 sigma ladder and gives every float a relative
  tolerance from its formula: lambda = -logf(sigma) carries 1 ulp of the host libm (<= 2 u |lambda|), h = lambda_t - lambda_s therefore e_h = 2 u (|lambda_t| +
  |lambda_s|) + u |h|; every later field is G(h_hat) evaluated with local roundings, so its error is |G'(h)| e_h plus the local roundings amplified by what follows them
  (c2 divides the roundings of expf(-h) - 1 + h by h^2 and ends near -h / 6: that is the 1 / h^2 amplification).  Cap: <= 2^-14 relative for n_steps <= 20.

Consistency sampler: x_t = cos t x + sin t (z sd) and out = cos t x_t - (sin t sd)(-F): one rounding per product and per add, each product term with its modulus, plus
  1 ulp (<= 2 u) of the host's cosf / sinf on each term that carries one; xin == RNE_T(fl32(x_t / sd)) exactly.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -10
CAP = 16 * U
# measured by test_sampler_ops_cpu.py::test_fp32_emulation_passes_and_sets_the_constants on the committed cases (fp32 emulation, CPU):
EMU_WORST_A = 0.996           # worst |emulation - ref| / E
MEDIAN_RANGE = (1.0, 7.9, 10.9)   # median E / |ref| in u over the steps of those cases: least, largest without a guide (order 3), largest with one
C_RMS_STEP = 4.85 * U         # 4 x 1.21 u (order 3; orders 1 and 2 reach 0.85 u and 1.10 u)
C_RMS_STEP_GUIDED = 6.41 * U  # 4 x 1.60 u: the guide mix adds three roundings in front of everything else
FIELDS = ("c_skip", "c_out", "a", "b0", "inv_r0", "inv_r1", "f01", "inv_r01", "c1", "c2", "c_in_next", "order", "last")
TORCH_T = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CHUNK = {"fp32": 32, "bf16": 64, "fp16": 64}


def rne(v, T):
    """fp32 array -> storage type T (round to nearest even) -> fp32"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    return v if T == "fp32" else torch.from_numpy(v).to(TORCH_T[T]).float().numpy()


def engine_table(sigmas, sigma_data, solver_order, lower_order_final=True):
    """the engine's own coefficient table (td_dpm_coefs: host code, needs no GPU): (n_steps, 13) fp32"""
    from terrain_diffusion_amd.engine import dpm_coefs
    return dpm_coefs(sigmas, sigma_data, solver_order, lower_order_final)


def row(table, i):
    return {f: float(table[i][j]) for j, f in enumerate(FIELDS)}


# ------------------------------------------------------------------------------------------------------------------ the step twin
def step_ref(k, x, F, m1, m2, Fg=None, gscale=None):
    """float64 dpm_update on fp32 operands (arrays of one shape) with the coefficient row k (dict of the fp32 values); returns dict(x, m0, E_x, E_m0, terms)"""
    x, F, m1, m2 = (np.asarray(a, dtype=np.float64) for a in (x, F, m1, m2))
    ab = np.abs
    if Fg is not None:
        g, s = np.asarray(Fg, dtype=np.float64), float(np.float32(gscale))
        sd = s * (F - g)
        f = g + sd
        Ef = 2 * U * ab(sd) + U * ab(f)
    else:
        f, Ef = F, 0.0
    cf = k["c_out"] * f
    m0 = k["c_skip"] * x + cf
    E0 = ab(k["c_out"]) * Ef + U * ab(cf) + U * ab(m0)
    bm = k["b0"] * m0
    base = k["a"] * x - bm
    Eb = ab(k["b0"]) * E0 + U * ab(bm) + U * ab(base)
    order = int(k["order"])
    terms = {"c_out f": cf, "b0 m0": bm, "base": base}
    if order == 1:
        xn, Ex = base, Eb
    elif order == 2:
        d = m0 - m1
        q = k["inv_r0"] * d
        Eq = ab(k["inv_r0"]) * (E0 + U * ab(d)) + U * ab(q)
        xn = base - 0.5 * k["b0"] * q
        Ex = ab(0.5 * k["b0"]) * Eq + Eb + U * ab(xn)
        terms["0.5 b0 q"] = 0.5 * k["b0"] * q
    else:
        da, db = m0 - m1, m1 - m2
        d10, d11 = k["inv_r0"] * da, k["inv_r1"] * db
        E10 = ab(k["inv_r0"]) * (E0 + U * ab(da)) + U * ab(d10)
        E11 = ab(k["inv_r1"]) * U * ab(db) + U * ab(d11)
        dd = d10 - d11
        Edd = E10 + E11 + U * ab(dd)
        d1 = d10 + k["f01"] * dd
        E1 = ab(k["f01"]) * Edd + E10 + U * ab(d1)
        d2 = k["inv_r01"] * dd
        E2 = ab(k["inv_r01"]) * Edd + U * ab(d2)
        inner = base + k["c1"] * d1
        xn = inner - k["c2"] * d2
        Ex = ab(k["c2"]) * E2 + ab(k["c1"]) * E1 + Eb + U * ab(inner) + U * ab(xn)
        terms.update({"c1 d1": k["c1"] * d1, "c2 d2": k["c2"] * d2})
    return dict(x=xn, m0=m0, E_x=Ex * SECOND_ORDER, E_m0=E0 * SECOND_ORDER, terms=terms)


def chain_float64(sig, orders, x, model, sigma_data=0.5):
    """the twin chained without rounding on float64 coefficients (`coef_ref`): what oracle/schedule.py computes in fp32.  model(x_in, i) -> F"""
    ref = coef_ref(sig, sigma_data, orders=orders)
    x = np.asarray(x, dtype=np.float64)
    m1 = m2 = np.zeros_like(x)
    out = []
    for i in range(len(orders)):
        k = {f: ref["val"][i][j] for j, f in enumerate(FIELDS)}
        c_in = 1.0 / math.sqrt(float(sig[i]) ** 2 + sigma_data ** 2)
        r = step_ref(k, x, model(x * c_in, i), m1, m2)
        x, m1, m2 = r["x"], r["m0"], m1
        out.append(x)
    return out


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation (CPU)
def _fma(a, b, c):
    """a * b is exact in float64 (2 x 24 bits), the sum is rounded to 53 bits and then once to 24"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def emulate_update(k, x, F, m1, m2, Fg=None, gscale=None, mutant=None):
    """dpm_update + the guide mix in numpy fp32, operation by operation as td_device.h / small_kernels.hip spell them.  k: coefficient row (dict);
    returns (x_new, m0).  `mutant` breaks one thing (test_sampler_ops_cpu.py)."""
    f32 = np.float32
    c = {n: f32(v) for n, v in k.items()}
    if mutant == "bf16 coefficient":
        c["b0"] = f32(rne(np.array([c["b0"]]), "bf16")[0])
    x, F, m1, m2 = (np.asarray(a, dtype=f32) for a in (x, F, m1, m2))
    f = F
    if Fg is not None:
        g = np.asarray(Fg, dtype=f32)
        f = (F + f32(gscale) * (g - F)) if mutant == "guide swapped" else (g + f32(gscale) * (F - g))
    m0 = _fma(c["c_skip"], x, c["c_out"] * f)
    base = _fma(c["a"], x, -(c["b0"] * m0))
    order = int(k["order"])
    if mutant == "order 2 for 3" and order == 3:
        order = 2
    elif mutant == "order 3 for 2" and order == 2:
        order = 3
    if order == 1:
        return base, m0
    if order == 2:
        prev = m2 if mutant == "difference against m2" else m1
        half = f32(1.0) if mutant == "half dropped" else f32(0.5)
        return _fma(-(half * c["b0"]), c["inv_r0"] * (m0 - prev), base), m0
    d10, d11 = c["inv_r0"] * (m0 - m1), c["inv_r1"] * (m1 - m2)
    dd = d10 - d11
    d1, d2 = _fma(c["f01"], dd, d10), c["inv_r01"] * dd
    return _fma(-c["c2"], d2, _fma(c["c1"], d1, base)), m0


class EmuSampler:
    """sample_edm_lane in numpy: the buffers and index arithmetic of prep_input_kernel, write_cond_img_kernel and dpm_step_kernel (planar fp32 x / m1 / m2
    [N][C][HW], NHWC xin [N][HW][chunk] in T, NHWC F [N][HW][8]), with emulate_update per element.  run(k) returns what the engine's read-back labels return after
    "sampler_stop_after" = k.  model(xin_nhwc fp32 view, step) -> F [N][HW][C]; `mutant` breaks one thing."""

    def __init__(self, table, T, n, C, Cin, H, W, x0, c_in0, model, cond_img=None, guide=None, gscale=None, solver_order=3, mutant=None, mutant_table=None):
        self.tab, self.T, self.n, self.C, self.Cin, self.H, self.W = table, T, n, C, Cin, H, W
        self.x0, self.c_in0, self.model, self.cond_img, self.guide, self.gscale = np.asarray(x0, np.float32), np.float32(c_in0), model, cond_img, guide, gscale
        self.has_m2, self.mutant, self.chunk = solver_order == 3, mutant, CHUNK[T]
        self.run_tab = table if mutant_table is None else mutant_table          # the table the (broken) sampler runs with; the checker keeps `table`

    def _planar(self, n, c, p):
        C, HW = self.C, self.H * self.W
        if self.mutant == "H and W swapped":
            y, xx = divmod(p, self.W)
            p = xx * self.H + y
        return ((n * (8 if self.mutant == "batch offset n * 8" else C) + c) * HW + p)

    def run(self, k):
        n, C, Cin, H, W, ch = self.n, self.C, self.Cin, self.H, self.W, self.chunk
        HW = H * W
        idx = np.array([[[self._planar(i, c, p) for p in range(HW)] for c in range(C)] for i in range(n)])      # [n][C][HW] -> flat offset
        size = n * 8 * HW
        x, m1, m2 = np.zeros(size, np.float32), np.zeros(size, np.float32), np.zeros(size, np.float32)
        x[:n * C * HW] = self.x0.reshape(-1)                                  # the caller's tensor is copied in as it is laid out
        xin = np.zeros((n, HW, ch), np.float32)
        if self.cond_img is not None:                                         # write_cond_img_kernel
            xin[:, :, C:Cin] = rne(np.asarray(self.cond_img, np.float32).reshape(n, Cin - C, HW).transpose(0, 2, 1), self.T)
        plain = np.arange(n * C * HW).reshape(n, C, HW)                       # prep_input_kernel reads x with the plain index
        xin[:, :, :C] = rne(x[plain] * self.c_in0, self.T).transpose(0, 2, 1)
        xin[:, :, C if self.mutant == "ones channel at C" else Cin] = 1.0
        F = Fg = None
        steps = self.tab.shape[0]
        for i in range(min(k, steps)):
            kr = row(self.run_tab, i)
            F = np.asarray(self.model(xin, i), np.float32)                    # [n][HW][C]
            Fg = np.asarray(self.guide(xin, i), np.float32) if self.guide else None
            cs = C - 1 if self.mutant == "last channel skipped" else C
            for c in range(cs):
                o = idx[:, c, :]
                xn, m0 = emulate_update(kr, x[o], F[:, :, c], m1[o], m2[o], None if Fg is None else Fg[:, :, c], self.gscale, self.mutant)
                x[o] = xn
                if self.has_m2 and self.mutant != "history not shifted":
                    m2[o] = m1[o]
                m1[o] = m0
                if not kr["last"] or self.mutant == "last step writes xin":
                    xin[:, :, c] = rne(xn * np.float32(kr["c_in_next"]), self.T)
        pl = lambda a: a[:n * C * HW].reshape(n, C, H, W).copy()
        nchw = lambda a: None if a is None else np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(n, -1, H, W)
        return dict(x=pl(x), m1=pl(m1), m2=pl(m2), xin=nchw(xin), F=nchw(F), Fg=nchw(Fg), xin_g=nchw(xin) if self.guide else None)


# ------------------------------------------------------------------------------------------------------------------ the criterion
WHERE = {}      # name of an exact hand-off -> description of the first element that missed it (for the failure message)


def _exact(bad, name, got, want):
    if got.shape != want.shape:
        bad[name] = bad.get(name, 0) + max(got.size, 1)
        return None
    ne = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    d = int(np.count_nonzero(ne))
    if not d:
        return None
    bad[name] = bad.get(name, 0) + d
    at = tuple(int(v) for v in np.argwhere(ne)[0])
    WHERE[name] = f"first at {at}: stored {float(got[at])!r}, expected {float(want[at])!r}"
    return ne


def check_xin_static(bad, xin, T, C, Cin, cond_img):
    """the part of the model input no step may touch: conditioning image, ones channel, zero padding"""
    if Cin > C:
        _exact(bad, "xin cond_img", xin[:, C:Cin], rne(cond_img, T))
    _exact(bad, "xin ones", xin[:, Cin], np.ones_like(xin[:, Cin]))
    _exact(bad, "xin padding", xin[:, Cin + 1:], np.zeros_like(xin[:, Cin + 1:]))


def check_start(S0, x0, c_in0, T, C, Cin, cond_img=None):
    """state at sampler_stop_after = 0; returns {name: differing elements}"""
    bad = {}
    _exact(bad, "x at k=0", S0["x"], np.asarray(x0, np.float32))
    _exact(bad, "m1 at k=0", S0["m1"], np.zeros_like(S0["m1"]))
    _exact(bad, "m2 at k=0", S0["m2"], np.zeros_like(S0["m2"]))
    _exact(bad, "xin sample", S0["xin"][:, :C], rne(np.asarray(x0, np.float32) * np.float32(c_in0), T))
    check_xin_static(bad, S0["xin"], T, C, Cin, cond_img)
    if S0.get("xin_g") is not None:
        _exact(bad, "guide xin", S0["xin_g"], S0["xin"])
    return bad


def check_step(k, pre, post, T, C, Cin, has_m2, cond_img=None, gscale=None):
    """step described by coefficient row k: `pre` = state before it, `post` = state after it (with the F / Fg the step consumed).  Returns the figures; judge them with
    `verdict`."""
    r = step_ref(k, pre["x"], post["F"][:, :C], pre["m1"], pre["m2"], None if post.get("Fg") is None else post["Fg"][:, :C], gscale)
    st = {"order": int(k["order"]), "last": int(k["last"]), "elements": int(r["x"].size), "guided": post.get("Fg") is not None}
    for what, got, ref, E in (("x", post["x"], r["x"], r["E_x"]), ("m0", post["m1"], r["m0"], r["E_m0"])):
        err = np.abs(got.astype(np.float64) - ref)
        ratio = err / np.maximum(E, 1e-300)
        st[f"A_{what}"] = float(np.nanmax(np.where(np.isfinite(ratio), ratio, np.inf))) if np.all(np.isfinite(got)) else float("inf")
        st[f"at_{what}"] = tuple(int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        st[f"B_{what}"] = float(np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(ref ** 2)))
        st[f"median_{what}"] = float(np.median(E / np.maximum(np.abs(ref), 1e-300)))
        st[f"rne_{what}"] = float(np.mean(got == ref.astype(np.float32)))
    bad = {}
    _exact(bad, "m2 shift" if has_m2 else "m2 untouched", post["m2"], pre["m1"] if has_m2 else pre["m2"])
    if k["last"]:
        _exact(bad, "xin after the last step", post["xin"], pre["xin"])
    else:
        ne = _exact(bad, "xin sample", post["xin"][:, :C], rne(post["x"] * np.float32(k["c_in_next"]), T))
        if ne is not None and T != "fp32":       # say what the stored values are instead: the product rounded ONCE to T (a multiply fused with the conversion)?
            once = torch.from_numpy(post["x"].astype(np.float64) * float(np.float32(k["c_in_next"]))).to(TORCH_T[T]).float().numpy()
            at = tuple(int(v) for v in np.argwhere(ne)[0])
            WHERE["xin sample"] += (f"; x_new {float(post['x'][at])!r} * c_in_next {float(np.float32(k['c_in_next']))!r}; {int(np.count_nonzero(post['xin'][:, :C][ne] == once[ne]))} of "
                                    f"{int(ne.sum())} differing elements equal the product rounded once to {T}")
    check_xin_static(bad, post["xin"], T, C, Cin, cond_img)
    if post.get("xin_g") is not None:
        _exact(bad, "guide xin", post["xin_g"], post["xin"])
    st["exact_bad"] = bad
    return st


def verdict(st):
    """list of what the step violates (empty: passes A, B, the cap and the exact hand-offs)"""
    v = []
    cmax = C_RMS_STEP_GUIDED if st["guided"] else C_RMS_STEP
    for what in ("x", "m0"):
        if not st[f"A_{what}"] <= 1.0:
            v.append(f"A({what}): err / E = {st[f'A_{what}']:.3g} at {st[f'at_{what}']}")
        if not st[f"B_{what}"] <= cmax:
            v.append(f"B({what}): {st[f'B_{what}'] / U:.2f} u > {cmax / U:.2f} u")
        if not st[f"median_{what}"] <= CAP:
            v.append(f"cap({what}): median E / |ref| = {st[f'median_{what}'] / U:.1f} u > 16 u")
    v += [f"exact {n}: {c} elements differ ({WHERE.get(n, '')})" for n, c in st["exact_bad"].items()]
    return v


def check_trajectory(run, table, T, C, Cin, has_m2, x0, c_in0, cond_img=None, gscale=None, ks=None):
    """run(k) -> state after k steps (EmuSampler.run / the engine with sampler_stop_after = k).  Checks k = 0 and every step; returns (stats per step, violations)."""
    n_steps = table.shape[0]
    S = run(0)
    viol = [f"k=0 exact {n}: {c} elements differ" for n, c in check_start(S, x0, c_in0, T, C, Cin, cond_img).items()]
    stats = []
    for i in range(n_steps):
        S1 = run(i + 1)
        st = check_step(row(table, i), S, S1, T, C, Cin, has_m2, cond_img, gscale)
        st["step"] = i
        stats.append(st)
        viol += [f"step {i} (order {st['order']}): {m}" for m in verdict(st)]
        S = S1
    return stats, viol


def miss_factor(stats, viol):
    """how far a broken sampler misses: worst err / E over the steps, and the exact hand-off elements that differ"""
    a = max(max(s["A_x"], s["A_m0"]) for s in stats)
    ex = sum(sum(s["exact_bad"].values()) for s in stats) + sum("k=0" in v for v in viol)
    return a, ex


def line(name, stats, wall=None):
    a = max(max(s["A_x"], s["A_m0"]) for s in stats)
    b = max(max(s["B_x"], s["B_m0"]) for s in stats)
    med = max(s["median_x"] for s in stats)
    rn = min(s["rne_x"] for s in stats)
    orders = "".join(str(s["order"]) for s in stats)
    return (f"{name}: {len(stats)} steps (orders {orders}), {stats[0]['elements']} elements per step; worst err / E {a:.3f}, B {b / U:.2f} u (<= {(C_RMS_STEP_GUIDED if stats[0]['guided'] else C_RMS_STEP) / U:.2f}), "
            f"max median E / |ref| {med / U:.1f} u (cap 16), x == RNE_32(ref) on >= {100 * rn:.1f} %" + (f"; {wall:.1f} s" if wall is not None else ""))


# ------------------------------------------------------------------------------------------------------------------ the coefficient table
def coef_ref(sig, sigma_data=0.5, solver_order=3, lower_order_final=True, orders=None):
    """float64 restatement of dpmsolver.py's coefficients (the formulae of oracle/schedule.py: step_coefficients, precondition_*, solver_orders) on the fp32 ladder
    `sig`, and a relative tolerance per float for an fp32 evaluation of the same formulae (derivation: module docstring).  Returns dict(val, tol): (n_steps, 13)."""
    from oracle import schedule
    sig = [float(np.float32(s)) for s in np.asarray(sig).reshape(-1)]
    n = len(sig) - 1
    if orders is None:
        orders = schedule.solver_orders(n, solver_order=solver_order, lower_order_final=lower_order_final)
    sd = float(sigma_data)
    val, tol = np.zeros((n, len(FIELDS))), np.zeros((n, len(FIELDS)))
    lam = lambda s: -math.log(s)
    e_lam = lambda s: 2 * U * abs(lam(s))
    for i in range(n):
        s, st, last = sig[i], sig[i + 1], i == n - 1
        v = dict.fromkeys(FIELDS, 0.0)
        t = dict.fromkeys(FIELDS, 0.0)
        v["c_skip"], t["c_skip"] = sd * sd / (s * s + sd * sd), 4 * U             # sd^2, s^2 + sd^2 (two products, one add, all positive), the division
        v["c_out"], t["c_out"] = s * sd / math.sqrt(s * s + sd * sd), 4 * U       # s sd; (s^2 + sd^2: 2 u) halved by the root, the root, the division
        v["order"], v["last"] = float(orders[i]), float(last)
        if last:
            assert st == 0.0
            v["a"], v["b0"], v["c_in_next"] = 0.0, -1.0, 0.0                      # st = 0: a = 0, h = +inf, expf(-inf) - 1 = -1: exact
        else:
            v["a"], t["a"] = st / s, U
            v["c_in_next"], t["c_in_next"] = 1.0 / math.sqrt(st * st + sd * sd), 3 * U
            h = lam(st) - lam(s)
            e_h = e_lam(st) + e_lam(s) + U * abs(h)
            ex = math.exp(-h)
            v["b0"] = ex - 1.0
            e_b0_local = 2 * U * ex + U * abs(v["b0"])                             # expf at 1 ulp, the subtraction
            t["b0"] = (ex * e_h + e_b0_local) / abs(v["b0"])
            if orders[i] >= 2:
                h0 = lam(s) - lam(sig[i - 1])
                e_h0 = e_lam(s) + e_lam(sig[i - 1]) + U * abs(h0)
                r0, rho0 = h0 / h, e_h / abs(h) + e_h0 / abs(h0) + U
                v["inv_r0"], t["inv_r0"] = 1.0 / r0, rho0 + U
                if orders[i] == 3:
                    h1 = lam(sig[i - 1]) - lam(sig[i - 2])
                    e_h1 = e_lam(sig[i - 1]) + e_lam(sig[i - 2]) + U * abs(h1)
                    r1, rho1 = h1 / h, e_h / abs(h) + e_h1 / abs(h1) + U
                    rhos = max(rho0, rho1) + U                                     # r0 + r1, both positive
                    v["inv_r1"], t["inv_r1"] = 1.0 / r1, rho1 + U
                    v["f01"], t["f01"] = r0 / (r0 + r1), rho0 + rhos + U
                    v["inv_r01"], t["inv_r01"] = 1.0 / (r0 + r1), rhos + U
                    q = (ex - 1.0) / h
                    v["c1"] = q + 1.0
                    g1 = (1.0 - ex - h * ex) / (h * h)                             # d/dh of (e^-h - 1) / h + 1
                    t["c1"] = (abs(g1) * e_h + e_b0_local / h + U * abs(q) + U * abs(v["c1"])) / abs(v["c1"])
                    num = ex - 1.0 + h
                    Q = num / (h * h)
                    v["c2"] = Q - 0.5
                    g2 = ((1.0 - ex) * h - 2.0 * num) / h ** 3                     # d/dh of (e^-h - 1 + h) / h^2 - 1/2
                    t["c2"] = (abs(g2) * e_h + (e_b0_local + U * abs(num)) / (h * h) + 2 * U * abs(Q) + U * abs(v["c2"])) / abs(v["c2"])
        val[i] = [v[f] for f in FIELDS]
        tol[i] = [t[f] * SECOND_ORDER for f in FIELDS]
    return dict(val=val, tol=tol)


def check_table(table, ref):
    """(worst |got - ref| / (tol |ref|) per field, exact-column mismatches): orders / last / zeros exact, floats within their tolerance"""
    worst, bad = {}, []
    for j, f in enumerate(FIELDS):
        got, val, tol = table[:, j].astype(np.float64), ref["val"][:, j], ref["tol"][:, j]
        ex = tol == 0.0
        if np.any(got[ex] != val[ex]):
            bad.append((f, [int(i) for i in np.nonzero(ex & (got != val))[0]]))
        r = np.abs(got[~ex] - val[~ex]) / (tol[~ex] * np.abs(val[~ex]))
        worst[f] = float(r.max()) if r.size else 0.0
    return worst, bad


# ------------------------------------------------------------------------------------------------------------------ consistency sampler
def consistency_ref(t, sd, sample, z, xt_stored, F):
    """float64 x_t / out of consistency_pre_kernel / consistency_post_kernel with their bounds; cos / sin of the fp32 t in float64 (the host's cosf / sinf: 1 ulp <= 2 u)"""
    t = float(np.float32(t))
    ct, sn, sd = math.cos(t), math.sin(t), float(np.float32(sd))
    sample, z, xs, F = (np.asarray(a, np.float64) for a in (sample, z, xt_stored, F))
    a1, a2 = ct * sample, sn * (z * sd)
    xt = a1 + a2
    E_xt = (U * (np.abs(a1) + 2 * np.abs(a2) + np.abs(xt)) + 2 * U * (np.abs(a1) + np.abs(a2))) * SECOND_ORDER      # cos x | z sd, sin (.) | the add | cosf, sinf
    b1, b2 = ct * xs, (sn * sd) * (-F)
    out = b1 - b2
    E_out = (U * (np.abs(b1) + 2 * np.abs(b2) + np.abs(out)) + 2 * U * (np.abs(b1) + np.abs(b2))) * SECOND_ORDER     # cos x_t | sin sd, (.) F | the subtraction | libm
    return dict(xt=xt, E_xt=E_xt, out=out, E_out=E_out)


def emulate_consistency(t, sd, sample, z, F, mutant=None):
    """the two kernels in numpy fp32 without contraction; returns (xt, xin_scaled fp32, out)"""
    f32 = np.float32
    ct, sn, sd = f32(math.cos(float(f32(t)))), f32(math.sin(float(f32(t)))), f32(sd)
    sample, z, F = (np.asarray(a, f32) for a in (sample, z, F))
    xt = ct * sample + sn * (z * sd)
    if mutant == "sin and cos swapped":
        xt = sn * sample + ct * (z * sd)
    out = ct * xt - sn * sd * (-F)
    if mutant == "sign of F":
        out = ct * xt - sn * sd * F
    return xt, xt / sd, out


def check_consistency(t, sd, sample, z, got_xt, got_xin, F, got_out, T, C, Cin, cond_img=None):
    r = consistency_ref(t, sd, sample, z, got_xt, F)
    st = {"elements": int(r["xt"].size)}
    for what, got, ref, E in (("xt", got_xt, r["xt"], r["E_xt"]), ("out", got_out, r["out"], r["E_out"])):
        err = np.abs(np.asarray(got, np.float64) - ref)
        st[f"A_{what}"] = float((err / np.maximum(E, 1e-300)).max())
        st[f"B_{what}"] = float(np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(ref ** 2)))
        st[f"median_{what}"] = float(np.median(E / np.maximum(np.abs(ref), 1e-300)))
    bad = {}
    _exact(bad, "xin sample", got_xin[:, :C], rne(np.asarray(got_xt, np.float32) / np.float32(sd), T))
    check_xin_static(bad, got_xin, T, C, Cin, cond_img)
    st["exact_bad"] = bad
    return st


def verdict_consistency(st):
    v = [f"A({w}): err / E = {st[f'A_{w}']:.3g}" for w in ("xt", "out") if not st[f"A_{w}"] <= 1.0]
    v += [f"cap({w}): median E / |ref| = {st[f'median_{w}'] / U:.1f} u" for w in ("xt", "out") if not st[f"median_{w}"] <= CAP]
    return v + [f"exact {n}: {c} elements differ" for n, c in st["exact_bad"].items()]


# ------------------------------------------------------------------------------------------------------------------ shared inputs
def toy_model(C, seed, strength=1.0):
    """a cheap stand-in for the U-Net on the CPU: F depends on the model input the way a denoiser's does (F correlated with x), plus a channel mix"""
    rs = np.random.RandomState(seed)
    mix = (rs.standard_normal((C, C)) / math.sqrt(C)).astype(np.float32)

    def model(xin, i):
        xs = np.asarray(xin, np.float32)[:, :, :C]
        return (strength * (np.tanh(0.3 * xs) - 0.6 * xs @ mix) - np.float32(0.2 * math.cos(0.37 * i))).astype(np.float32)
    return model


def noise_model(C, seed):
    """white-noise F, independent of x"""
    def model(xin, i):
        return np.random.RandomState(seed + i).standard_normal(np.asarray(xin).shape[:2] + (C,)).astype(np.float32)
    return model
