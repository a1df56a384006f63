"""Host model ("twin") of the embedding and modulation kernels (csrc/small_kernels.hip: emb_kernel; cvec_kernel, cvec_mfma_kernel<1>, cvec_mfma_kernel<4>;
cvec_norm_kernel) in plain torch float64, the element-wise criterion they are held to, and a float32 emulation of their arithmetic on the CPU that the constants
of the statistical condition rest on.  Nothing here imports `terrain_diffusion_amd`; torch shares no code with the engine.

Operands (`operands`).  Exactly the fp32 tensors the engine is handed: `_conv_twin.fold_host(w, gain)` (pinned bit for bit to the host's fold by
  tests/test_conv_ops_cpu.py), gain = the fp32 `emb_gain` for a block's `emb_linear`, 1 otherwise; freqs / phases as stored; the input weights as the fp32 values
  the config struct holds; inv_norm = fp32(1 / sqrt(1 + sum_i weight_i^2)), formed in double as `finalize` (engine.hip) forms it.

Rows (`row_index`).  row = step * n_tiles + tile: t depends on the step only, the conditional inputs on the tile only.  A sampler call writes n_steps * N rows, a
  forward with one t n rows; a forward with differing t writes the n * n cross product and then copies the diagonal rows (i, i) = row i * n + i over rows 1 .. n - 1
  (emb and cvec alike), which is the table the conv stack reads.  "@emb:rows" / "@cvec:rows" return all of it.

Embedding op (`embedding`), one row from t, cond and the weights:
    y_k = fl32(t * f_k)                         one IEEE fp32 multiply: restated in fp32, reproduces exactly
    p   = sqrt2 * (sin y, cos y)                float64
    e_0 = W_noise p
    tensor input i:  e_i = mp_silu(W_i x)       float input i:  y = fl32(fl32(x * f) + ph) (the kernel spells __fmul_rn / __fadd_rn: fp32, exact),
                                                                e_i = W_i (sqrt2 cos y), NO mp_silu
    emb = mp_silu((e_0 + sum_i weight_i e_i) * inv_norm)                                                     mp_silu(z) = z / (1 + exp(-z)) / 0.596, all float64
Modulation op (`modulation`), from the rows the ENGINE stored (@emb:rows), not from the twin's embedding, so that an error cannot hide behind the op in front:
    c = E W_b^T + 1 per block b;     out = c / sqrt(mean_b(c^2) + 1e-8)

Condition A, every element, nothing skipped, masked or averaged:   |hip - ref| <= E.   E is a worst-case deterministic bound (K <= 768: no sqrt(K) model);
  u = 2^-24:
    dot product of length K        (ceil(K / 64) + 7) u sum_k |w_k x_k|: one lane's sequential chain of ceil(K / 64) products, the 6-level xor butterfly, the product
                                   rounding.  The matrix-core form (four products per accumulate step, interleaved chains) is given the same allowance.
    a sin / cos feature            (2 TRIG_ULP + 1) u |p_k| (TRIG_ULP ulps of 2 u each, the multiply by sqrt2), carried through |w_k|
    weighted sum                   a += weight_i * e_i: 2 u (|weight_i e_i| + |a|) per input (the product, the sum, the second order of both)
    * inv_norm                     u |z|
    mp_silu                        the error d of its argument as sup |silu(z') - silu(z)| over |z' - z| <= d (`_conv_twin._through_silu`: not linearised), plus
                                   (EXP_ULP |z| + 4) u |silu| for expf, 1 + e, the division and the constant
    + 1                            u |c|
    the norm                       E_c / rms + |ref| rms_b(E_c) / rms + (ceil(cout / 256) + 12) u |ref|: an element's own error, the relative error of the rms (the rms
                                   of the block's element errors over the rms), and the sum of squares (cout / 256 per thread, butterfly, four partial sums),
                                   the division by cout, + 1e-8, sqrtf, the reciprocal, the multiply
    TRIG_ULP = 4, EXP_ULP = 3      the OpenCL full-profile limits for sin, cos (4 ulp) and exp (3 ulp), which the device math library is written to meet.  They are a
                                   SPECIFICATION, not a measurement: nobody has measured sinf, cosf or expf on the MI355X.  The engine is built without fast-math
                                   (__graft_entry__.py: -O3 and nothing else), so sinf / cosf / expf are the library's full-range functions.
    sampler cases only             the engine forms t = atanf(sigma / sigma_d) on the host and the test cannot rely on the same last bit: + ulp32(t) |d ref / d t|, the
                                   derivative in float64 from the formula (`embedding(..., t_slack=True)`).
  Cap (asserted by `check`: it keeps A from being vacuous): per case the median over elements of E / |ref| is <= CAP = 2^-14 = 1024 u, for the embedding rows and per
  block for the modulation rows.  If a case exceeds it the model is tightened, the cap stays.
Condition B, per case:   rms(hip - ref) / rms(ref) <= C_RMS_EMB (embedding rows), C_RMS_CVEC (modulation rows) = 4 x the worst value `emulate` gives over the
  CPU cases (tests/test_emb_ops_cpu.py prints them and asserts the constants below against them).  4: the device's sinf / cosf / expf may be 3 - 4 ulp where the
  CPU's are about 1, and the matrix core's summation order is not the CPU's.
Honesty, per case:   any two rows of ref that belong to different (step, tile) pairs differ in at least one element by more than 1000 E, else a wrong-row read could
  pass.  (Rows 1 .. n - 1 of a differing-t forward ARE copies of other rows; a model without conditional inputs has one row per step whatever the tile: those
  pairs are equal by construction and are left out, the second being a limit of such a case: it cannot see a wrong tile.)

`emulate`: the same ops in fp32 with the kernels' summation shapes -- 64 lanes with stride-64 chains and the xor butterfly 32 .. 1 (emb_kernel, cvec_kernel); the k
  order 16 m + 4 g + t with four products (g = 0 .. 3) per accumulate step (cvec_mfma_kernel: MFMA t of super-step m); the two-level sum of cvec_norm_kernel
  (thread stride 256, butterfly per wave, four partial sums in order); the diagonal copy.  `mutate` builds the deliberately broken kernels of the CPU test.

Constants, from tests/test_emb_ops_cpu.py (torch 2.10 CPU, the 21 cases of `gpu_cases()`), none from a GPU kernel:
    rms(emulation - ref) / rms(ref), embedding rows     1.46 .. 2.54 u (worst: emb_channels 16)                            x 4 -> C_RMS_EMB  = 10.2 u
    rms(emulation - ref) / rms(ref), modulation rows    1.03 .. 2.47 u (worst: emb_channels 768, 192 accumulate steps)     x 4 -> C_RMS_CVEC = 9.9 u
                                                         (the only check there was, on 2 embedding rows: 5e-6 = 84 u)
    worst |emulation - ref| / E                          embedding 0.41, modulation 0.26
    median E / (u |ref|)                                 embedding 46 .. 296, modulation rows (largest block of a case) 35 .. 331 (cap 1024)
What the MI355X showed is in DESIGN.md, "How the embedding and modulation kernels are checked".
"""
import math

import torch

from oracle.unet import build_plan, synth_state_dict, tiny_config
from oracle import rng

import _conv_twin as ct

U = 2.0 ** -24
TRIG_ULP, EXP_ULP = 4.0, 3.0
CAP = 2.0 ** -14
C_RMS_EMB, C_RMS_CVEC = 10.2 * U, 9.9 * U
HONEST = 1000.0
SQRT2_32 = float(torch.tensor(1.41421356237309515, dtype=torch.float32))
F32, F64 = torch.float32, torch.float64


def ulp32(x):
    """unit in the last place of fp32 in the binade the float64 x lies in"""
    e = ((x.abs().contiguous().view(torch.int64) >> 52) & 0x7FF) - 1023
    return ((e.clamp_min(-126) - 23 + 1023) << 52).view(F64)


def arm_of(cfg):
    """which kernel compute_cvecs (engine.hip) launches for the product: '<4>', '<1>' (cvec_mfma_kernel<U>) or 'scalar' (cvec_kernel)"""
    plan = build_plan(cfg)
    blocks = [b for b in plan["enc"] + plan["dec"] if b["kind"] != "conv"]
    c16 = plan["emb_channels"] % 16 == 0 and sum(b["cout"] for b in blocks) % 4 == 0 and all(b["cout"] % 16 == 0 for b in plan["enc"] + plan["dec"])
    return "<4>" if c16 and plan["emb_channels"] % 64 == 0 else ("<1>" if c16 else "scalar")


# ------------------------------------------------------------------------------------------------ operands
def operands(cfg, sd):
    """the fp32 tensors the engine holds after load_state_dict(fold='reference') + finalize"""
    plan = build_plan(cfg)
    ops = dict(emb_ch=plan["emb_channels"], freqs=sd["noise_fourier.freqs"].to(F32), w_noise=ct.fold_host(torch.as_tensor(sd["noise_linear.weight"]), 1), conds=[], blocks=[])
    wsq = 1.0
    for i, (typ, dim, wt) in enumerate(cfg.get("conditional_inputs", [])):
        w32 = float(torch.tensor(float(wt), dtype=F32))
        pre = f"conditional_layers.{i}"
        if typ == "tensor":
            ops["conds"].append(dict(type="tensor", dims=dim, weight=w32, w=ct.fold_host(torch.as_tensor(sd[pre + ".weight"]), 1)))
        else:
            ops["conds"].append(dict(type="float", dims=dim, weight=w32, w=ct.fold_host(torch.as_tensor(sd[pre + ".1.weight"]), 1),
                                     freqs=sd[pre + ".0.freqs"].to(F32), phases=sd[pre + ".0.phases"].to(F32)))
        wsq += w32 * w32
    ops["inv_norm"] = float(torch.tensor(1.0 / math.sqrt(wsq), dtype=F32))
    off = 0
    for b in plan["enc"] + plan["dec"]:
        if b["kind"] == "conv":
            continue
        w = ct.fold_host(torch.as_tensor(sd[b["name"] + ".emb_linear.weight"]), torch.as_tensor(sd[b["name"] + ".emb_gain"]).to(F32))
        ops["blocks"].append(dict(name=b["name"], cout=b["cout"], off=off, w=w))
        off += b["cout"]
    ops["c_total"] = off
    return ops


# ------------------------------------------------------------------------------------------------ rows
def row_index(n_steps, n_tiles, diagonal=False):
    """(step, tile) of every stored row; diagonal: the forward with differing t (n_steps == n_tiles), rows 1 .. n - 1 overwritten by the rows (i, i)"""
    r = torch.arange(n_steps * n_tiles)
    step, tile = r // n_tiles, r % n_tiles
    if diagonal:
        assert n_steps == n_tiles
        for i in range(1, n_tiles):
            step[i], tile[i] = i, i
    return step, tile


def make_case(name, kind, n, cfg_kw=None, seed=77, cfg=None):
    """kind 'forward' (n distinct t: n * n rows with the diagonal copy), 'uniform' (one t, n rows), 'edm' (5 sigmas x n tiles), 'consistency' (one t, n tiles).
    t from 1e-3 to 1.5705, float inputs reaching +-4 (|x f| passes 40), tensor inputs standard normal."""
    cfg = cfg or tiny_config(64, 1, **(cfg_kw or {}))
    sd = synth_state_dict(cfg, seed=seed)
    cond = []
    for i, (typ, dim, _w) in enumerate(cfg.get("conditional_inputs", [])):
        if typ == "tensor":
            cond.append(torch.from_numpy(rng.standard_normal(8 + i, (n, dim))).to(F32))
        else:
            x = torch.from_numpy(rng.standard_normal(8 + i, (n,))).to(F32) * 1.6
            x[0] = 4.0 - 0.25 * i
            if n > 1:
                x[n - 1] = -4.0 + 0.125 * i
            cond.append(x)
    case = dict(name=name, kind=kind, n=n, cfg=cfg, sd=sd, cond=cond, diagonal=False, t_slack=False)
    if kind == "forward":
        t = torch.linspace(1e-3, 1.5705, n, dtype=F32) if n > 1 else torch.tensor([0.7853], dtype=F32)
        case.update(t=t, diagonal=n > 1)
    elif kind == "uniform":
        case.update(t=torch.tensor([1.1], dtype=F32))
    elif kind == "consistency":
        case.update(t=torch.tensor([1.5705], dtype=F32))
    elif kind == "edm":
        sig = torch.tensor([80.0, 9.5, 1.3, 0.11, 0.002, 0.0], dtype=F32)
        case.update(sigmas=sig, sigma_data=0.5, t=torch.atan(sig[:5] / torch.tensor(0.5, dtype=F32)), t_slack=True)
    else:
        raise ValueError(kind)
    case["step"], case["tile"] = row_index(case["t"].numel(), n, case["diagonal"])
    return case


MIXED8 = [["tensor", 58, 1.0], ["float", 64, 0.2], ["tensor", 300, 0.7], ["float", 7, 0.5], ["tensor", 1, 0.3], ["float", 1, 1.5], ["tensor", 64, 0.0], ["float", 300, 0.25]]
FLOAT5 = [["float", 64, 0.2]] * 5


def gpu_cases():
    """(name, kind, n, config overrides) of every case tests/test_emb_ops_gpu.py runs; tests/test_emb_ops_cpu.py runs the emulation on the same list"""
    c = []
    for n in (1, 8, 9, 17):
        c.append((f"forward n{n} emb256 tensor58", "forward", n, {}))
    c.append(("uniform n8 emb256 tensor58", "uniform", 8, {}))
    for e in (768, 80, 16, 100, 37):
        c.append((f"forward n17 emb{e} tensor58", "forward", 17, dict(emb_channels=e)))
    c += [("forward n9 emb256 no cond", "forward", 9, dict(conditional_inputs=[])),
          ("forward n9 emb37 no cond noise6", "forward", 9, dict(emb_channels=37, conditional_inputs=[], noise_emb_dims=6)),
          ("forward n9 emb256 5 floats", "forward", 9, dict(conditional_inputs=FLOAT5)),
          ("forward n9 emb100 5 floats", "forward", 9, dict(emb_channels=100, conditional_inputs=FLOAT5)),
          ("forward n17 emb256 mixed8", "forward", 17, dict(conditional_inputs=MIXED8)),
          ("forward n9 emb80 mixed8", "forward", 9, dict(emb_channels=80, conditional_inputs=MIXED8)),
          ("forward n9 emb100 mixed8 noise6", "forward", 9, dict(emb_channels=100, conditional_inputs=MIXED8, noise_emb_dims=6)),
          ("forward n9 emb16 noise200", "forward", 9, dict(emb_channels=16, noise_emb_dims=200)),
          ("forward n9 emb256 noise200", "forward", 9, dict(noise_emb_dims=200)),
          ("edm 5 steps N3 emb256 tensor58", "edm", 3, {}),
          ("consistency N3 emb256 tensor58", "consistency", 3, {})]
    return c


# ------------------------------------------------------------------------------------------------ the reference and the bound
def _silu(z):
    return z / (1.0 + torch.exp(-z)) / 0.596


def _dsilu(z):
    s = torch.sigmoid(z)
    return s * (1.0 + z * (1.0 - s)) / 0.596


def _silu_bound(z, d):
    """(silu(z), what an argument error d and the evaluation itself may add)"""
    f = _silu(z)
    return f, ct._through_silu(z, d, f) + (EXP_ULP * z.abs() + 4.0) * U * f.abs()


def _dot(w, x, extra=0.0):
    """x (R, K) . w (J, K) in float64 and its allowance ((ceil(K / 64) + 7 + extra) u sum |w x|)"""
    K = w.shape[1]
    w, x = w.double(), x.double()
    return x @ w.T, (math.ceil(K / 64) + 7.0 + extra) * U * (x.abs() @ w.abs().T)


def embedding(ops, t, cond, step, tile, t_slack=False, trig=F64):
    """float64 embedding rows (R, emb_ch) for rows (step, tile) and the bound E of condition A.  t: fp32 (n_steps,); cond: the model call's list (per tile).
    trig = float32 takes sin / cos (and their sqrt2) in fp32, as oracle.unet.OracleUnet does in every dtype: only for the comparison with it."""
    t = t.to(F32)[step]
    y32 = t[:, None] * ops["freqs"][None, :]                                       # fl32(t f_k)
    y = y32.double()
    p = (torch.cat([y32.to(trig).sin(), y32.to(trig).cos()], 1) * math.sqrt(2.0)).double()
    a, E = _dot(ops["w_noise"], p, 2.0 * TRIG_ULP + 1.0)
    da = None
    if t_slack:                                                                     # d / dt of the noise part (float64, from the formula)
        f = ops["freqs"].double()[None, :]
        da = (torch.cat([f * y.cos(), -f * y.sin()], 1) * math.sqrt(2.0)) @ ops["w_noise"].double().T
    for c, x in zip(ops["conds"], cond):
        x = x.to(F32)[tile]
        if c["type"] == "tensor":
            b, eb = _dot(c["w"], x.reshape(-1, c["dims"]))
            g, eg = _silu_bound(b, eb)
        else:
            yy = ((x.reshape(-1, 1) * c["freqs"][None, :]) + c["phases"][None, :]).to(trig)     # two fp32 operations, separately rounded
            g, eg = _dot(c["w"], (yy.cos() * math.sqrt(2.0)).double(), 2.0 * TRIG_ULP + 1.0)
        a = a + c["weight"] * g
        E = E + abs(c["weight"]) * eg + 2.0 * U * (abs(c["weight"]) * g.abs() + a.abs())
    z = a * ops["inv_norm"]
    ref, Ee = _silu_bound(z, E * ops["inv_norm"] + U * z.abs())
    if t_slack:
        Ee = Ee + ulp32(t.double())[:, None] * (_dsilu(z) * ops["inv_norm"] * da).abs()
    return ref, Ee


def modulation(ops, emb_stored):
    """float64 modulation rows (R, c_total) from the STORED embedding rows (fp32 values) and the bound E of condition A"""
    ref, E = [], []
    for b in ops["blocks"]:
        c, ec = _dot(b["w"], emb_stored)
        c = c + 1.0
        ec = ec + U * c.abs()
        rms = torch.sqrt((c * c).mean(1, keepdim=True) + 1e-8)
        r = c / rms
        ref.append(r)
        E.append(ec / rms + r.abs() * (torch.sqrt((ec * ec).mean(1, keepdim=True)) / rms + (math.ceil(b["cout"] / 256) + 12.0) * U))
    return torch.cat(ref, 1), torch.cat(E, 1)


def reference(case, emb_stored, ops=None):
    """dict(emb, E_emb from (t, cond); cvec, E_cvec from the stored embedding rows)"""
    ops = ops or operands(case["cfg"], case["sd"])
    emb, Ee = embedding(ops, case["t"], case["cond"], case["step"], case["tile"], case["t_slack"])
    cv, Ec = modulation(ops, emb_stored)
    return dict(ops=ops, emb=emb, E_emb=Ee, cvec=cv, E_cvec=Ec)


# ------------------------------------------------------------------------------------------------ the criterion
def _honest(case, ref, E, what):
    """every pair of rows with different (step, tile) -- different step only, without conditional inputs -- differs somewhere by more than HONEST * E"""
    step, tile = case["step"], case["tile"]
    key = step * case["n"] + tile if case["cond"] else step
    worst = float("inf")
    for i in range(ref.shape[0] - 1):
        other = key[i + 1:] != key[i]
        if not bool(other.any()):
            continue
        d = (ref[i + 1:][other] - ref[i]).abs() / torch.maximum(E[i + 1:][other], E[i])
        m = d.amax(1)
        worst = min(worst, float(m.min()))
        if worst <= HONEST:
            j = int(torch.arange(i + 1, ref.shape[0])[other][int(m.argmin())])
            raise AssertionError(f"{case['name']}: {what} rows {i} (step {int(step[i])}, tile {int(tile[i])}) and {j} (step {int(step[j])}, tile {int(tile[j])}) differ by at most "
                                 f"{worst:.1f} E anywhere: a wrong-row read could pass (honesty needs > {HONEST:.0f})")
    return worst


def measure(hip, ref, E, spans=None):
    """statistics of one tensor, nothing asserted: worst |err| / E, the B ratio, the median(s) of E / |ref| (per span), the mask of A violations"""
    assert hip.shape == ref.shape, (tuple(hip.shape), tuple(ref.shape))
    err = (hip - ref).abs()
    bad = ~(err <= E)                                                              # (a NaN fails)
    ratio = (err / E).nan_to_num(nan=float("inf"))
    spans = spans or [(0, ref.shape[1])]
    med = [float((E[:, a:b] / ref[:, a:b].abs()).median()) for a, b in spans]
    return dict(worst=float(ratio.max()), nbad=int(bad.sum()), rms=float(torch.sqrt(((hip - ref) ** 2).mean()) / torch.sqrt((ref ** 2).mean())), median=max(med)), bad, ratio


def check(case, hip_emb, hip_cvec, honesty=True):
    """Conditions A and B, the cap and the honesty condition on one case.  hip_emb / hip_cvec: what "@emb:rows" / "@cvec:rows" returned (any float dtype).
    Returns the statistics; raises AssertionError naming the worst element."""
    hip_emb, hip_cvec = hip_emb.double(), hip_cvec.double()
    R = case["step"].numel()
    assert hip_emb.shape[0] == R and hip_cvec.shape[0] == R, (case["name"], tuple(hip_emb.shape), tuple(hip_cvec.shape), R)
    r = reference(case, hip_emb)
    ops = r["ops"]
    st = dict(name=case["name"], rows=R, arm=arm_of(case["cfg"]))
    spans = [(b["off"], b["off"] + b["cout"]) for b in ops["blocks"]]
    for what, hip, ref, E, sp, cmax in (("emb", hip_emb, r["emb"], r["E_emb"], None, C_RMS_EMB), ("cvec", hip_cvec, r["cvec"], r["E_cvec"], spans, C_RMS_CVEC)):
        m, bad, ratio = measure(hip, ref, E, sp)
        st.update({what + "_" + k: v for k, v in m.items()})
        if m["nbad"]:
            i, j = [int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape)]
            idx = bad.nonzero()
            blk = "" if what == "emb" else " (block " + next(b["name"] for b in ops["blocks"] if b["off"] <= j < b["off"] + b["cout"]) + ")"
            raise AssertionError(f"{case['name']} [{st['arm']}]: {m['nbad']} of {ref.numel()} {what} elements outside E; worst at row {i} (step {int(case['step'][i])}, tile "
                                 f"{int(case['tile'][i])}), column {j}{blk}: hip {float(hip[i, j]):.9g} ref {float(ref[i, j]):.9g}, error {m['worst']:.3g} x E; failing rows "
                                 f"{int(idx[:, 0].min())}..{int(idx[:, 0].max())}, columns {int(idx[:, 1].min())}..{int(idx[:, 1].max())}")
        assert m["median"] <= CAP, f"{case['name']}: median E / |ref| of the {what} rows = {m['median'] / U:.0f} u > {CAP / U:.0f} u: the bound is too loose to mean anything"
        assert m["rms"] <= cmax, f"{case['name']} [{st['arm']}]: rms({what} - ref) / rms(ref) = {m['rms'] / U:.2f} u > {cmax / U:.2f} u (condition B)"
        if honesty:
            st[what + "_honest"] = _honest(case, ref, E, what)
    return st


def line(st):
    return (f"{st['name']} [{st['arm']}, {st['rows']} rows]: emb worst err / E {st['emb_worst']:.3f}, B {st['emb_rms'] / U:.2f} u (<= {C_RMS_EMB / U:.1f}), median E {st['emb_median'] / U:.0f} u; "
            f"cvec worst err / E {st['cvec_worst']:.3f}, B {st['cvec_rms'] / U:.2f} u (<= {C_RMS_CVEC / U:.1f}), max block median E {st['cvec_median'] / U:.0f} u (cap {CAP / U:.0f})")


# ------------------------------------------------------------------------------------------------ the emulation
def _lane_dot32(w, x):
    """wave_sum form: x (R, K) . w (J, K) in fp32, 64 lanes, lane l sums k = l, l + 64, ... in order, then the xor butterfly 32 .. 1"""
    K = w.shape[1]
    Kp = (K + 63) // 64 * 64
    wp = torch.zeros(w.shape[0], Kp, dtype=F32); wp[:, :K] = w
    xp = torch.zeros(x.shape[0], Kp, dtype=F32); xp[:, :K] = x
    acc = torch.zeros(x.shape[0], w.shape[0], 64, dtype=F32)
    for s in range(Kp // 64):
        acc = acc + xp[:, None, s * 64:(s + 1) * 64] * wp[None, :, s * 64:(s + 1) * 64]
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ o]
    return acc[..., 0]


def _mfma_dot32(w, x, swap_b=False, drop=None):
    """cvec_mfma_kernel: per output one fp32 accumulator, MFMA t of super-step m adds the four products k = 16 m + 4 g + t, g = 0 .. 3 (summed exactly here,
    one rounding per accumulate step).  swap_b: the B operand takes k = 16 m + 4 t + g instead (the operands disagree inside a 16-group); drop: that step is skipped."""
    K = w.shape[1]
    assert K % 16 == 0
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=F32)
    wd, xd = w.double(), x.double()
    g = torch.arange(4)
    s = 0
    for m in range(K // 16):
        for t in range(4):
            ka = 16 * m + 4 * g + t
            kb = 16 * m + 4 * t + g if swap_b else ka
            if s != drop:
                acc = acc + (xd[:, kb] @ wd[:, ka].T).to(F32)
            s += 1
    return acc


def _silu32(z):
    return z / (1.0 + torch.exp(-z)) * (torch.tensor(1.0, dtype=F32) / torch.tensor(0.596, dtype=F32))


def _norm32(c, cout_div=None):
    """cvec_norm_kernel on one block's span c (R, cout) fp32: thread i sums c[i], c[i + 256], ...; butterfly per wave; red[0] + red[1] + red[2] + red[3]"""
    R, cout = c.shape
    P = (cout + 255) // 256 * 256
    sq = torch.zeros(R, P, dtype=F32); sq[:, :cout] = c * c
    s = torch.zeros(R, 256, dtype=F32)
    for q in range(P // 256):
        s = s + sq[:, q * 256:(q + 1) * 256]
    s = s.reshape(R, 4, 64)
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lanes ^ o]
    tot = ((s[:, 0, 0] + s[:, 1, 0]) + s[:, 2, 0]) + s[:, 3, 0]
    return 1.0 / torch.sqrt(tot / torch.tensor(float(cout_div or cout), dtype=F32) + torch.tensor(1e-8, dtype=F32))


MUTATIONS = ("tile_step_layout", "clamped_row", "k_order", "dropped_group", "no_plus1", "norm_neighbour", "norm_ctotal", "silu_on_float", "no_silu_on_tensor",
             "inv_norm_ignores_weights", "sincos_swapped", "xoff_dims", "no_diag_copy")


def emulate(case, mutate=None, ops=None):
    """(emb rows, cvec rows) in fp32 as the kernels would store them.  mutate: one of MUTATIONS (deliberately broken kernels, for the tests of the criterion)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    ops = ops or operands(case["cfg"], case["sd"])
    n, ns = case["n"], case["t"].numel()
    step, tile = row_index(ns, n, False)
    if mutate == "tile_step_layout":                                               # row = tile * n_steps + step
        r = torch.arange(ns * n)
        step, tile = r % ns, r // ns
    t = case["t"].to(F32)[step]
    y = t[:, None] * ops["freqs"][None, :]
    s2 = torch.tensor(SQRT2_32, dtype=F32)
    halves = [torch.sin(y) * s2, torch.cos(y) * s2]
    if mutate == "sincos_swapped":
        halves.reverse()
    a = _lane_dot32(ops["w_noise"], torch.cat(halves, 1))
    # the conditioning matrix as the C ABI takes it: `dims` columns per tensor input, ONE per float input
    cols = [x.to(F32).reshape(n, -1) for x in case["cond"]]
    mat = torch.cat(cols, 1) if cols else torch.zeros(n, 0)
    mat = torch.cat([mat, torch.zeros(n, 512)], 1)                                 # (room for a kernel that walks too far)
    xoff = 0
    for c in ops["conds"]:
        if c["type"] == "tensor":
            b = _lane_dot32(c["w"], mat[tile, xoff:xoff + c["dims"]])
            g = b if mutate == "no_silu_on_tensor" else _silu32(b)
            xoff += c["dims"]
        else:
            x = mat[tile, xoff:xoff + 1]
            g = _lane_dot32(c["w"], torch.cos(x * c["freqs"][None, :] + c["phases"][None, :]) * s2)
            if mutate == "silu_on_float":
                g = _silu32(g)
            xoff += c["dims"] if mutate == "xoff_dims" else 1
        a = a + torch.tensor(c["weight"], dtype=F32) * g
    inv = torch.tensor(1.0 if mutate == "inv_norm_ignores_weights" else ops["inv_norm"], dtype=F32)      # (1 / sqrt(1 + nothing))
    emb = _silu32(a * inv)
    # modulation rows
    arm = arm_of(case["cfg"])
    R = emb.shape[0]
    src = emb
    if mutate == "clamped_row":                                                    # the first row of the ragged last 64-row tile reads row R - 1 (cvec_mfma_kernel's clamp)
        r0 = (R - 1) // 64 * 64
        assert arm != "scalar" and r0 < R - 1, "the clamp belongs to the matrix-core kernel and needs a ragged last tile of more than one row"
        src = emb.clone(); src[r0] = emb[R - 1]
    craw = torch.empty(R, ops["c_total"], dtype=F32)
    for bi, b in enumerate(ops["blocks"]):
        if arm == "scalar":
            d = _lane_dot32(b["w"], src)
        else:
            d = _mfma_dot32(b["w"], src, swap_b=mutate == "k_order", drop=5 % (ops["emb_ch"] // 4) if mutate == "dropped_group" and bi == 3 else None)
        craw[:, b["off"]:b["off"] + b["cout"]] = d if mutate == "no_plus1" and bi == 2 else d + 1.0
    cv = torch.empty_like(craw)
    for bi, b in enumerate(ops["blocks"]):
        span = craw[:, b["off"]:b["off"] + b["cout"]]
        if mutate == "norm_neighbour" and bi + 1 < len(ops["blocks"]):
            nb = ops["blocks"][bi + 1]
            inv_r = _norm32(craw[:, nb["off"]:nb["off"] + nb["cout"]])
        elif mutate == "norm_ctotal":
            inv_r = _norm32(craw)
        else:
            inv_r = _norm32(span)
        cv[:, b["off"]:b["off"] + b["cout"]] = span * inv_r[:, None]
    if case["diagonal"] and mutate != "no_diag_copy":
        for i in range(1, n):
            emb[i] = emb[i * n + i]; cv[i] = cv[i * n + i]
    return emb, cv
