"""Host model ("twin") of the attention kernels (csrc/attn_mfma.hip: pack kernels + MFMA flash kernel; csrc/small_kernels.hip: the scalar attn_kernel) in plain
torch float64, the element-wise criterion they are held to, and a float32 / bf16 emulation of the flash kernel's arithmetic on the CPU that the constants rest on.
Nothing here imports `terrain_diffusion_amd`; torch shares no code with the engine.

Operands (`pack_operands`).  The twin is evaluated on what the flash kernel contracts, not on the fp32 inputs:
    Q = RNE_bf16(fp32(q) * f),  f = fp32(scale) * fp32(log2 e)  (one fp32 product, as the launcher forms it);   K = RNE_bf16(k);   V = RNE_bf16(v).
  Without `normalize` that is one IEEE multiply and reproduces exactly.  With it, x * inv, inv = 1 / (1e-4 + sqrt(ss) / sqrt(D)) [* f], is restated in fp32 in the
  pack kernels' order (lane = channel mod 64, up to three squares per lane added in ascending order, xor butterfly 32 .. 1).  The engine is built with the compiler's
  default contraction (ss += v * v may be a fused multiply-add) and sqrtf / the divisions need not be correctly rounded, so the restatement may differ from the kernel:
      sum of D squares: a rounding per square and per addition, depth 2 + 6       <= 9 u relative  -> 4.5 u behind the square root
      sqrtf(ss), sqrtf(D), the division by it, the reciprocal: 1 ulp = 2 u each   <= 8 u
      1e-4 + ..., * f, * x: one rounding each                                     <= 3 u           FLAG_U = 16 (u = 2^-24, relative to the operand)
  Every operand whose float64 value lies within FLAG_U u |a| of a bf16 rounding boundary is FLAGGED; a flagged operand may be one bf16 ulp off, pushed to the output
  exactly:   E_flip[i,c] = ln2 sum_j w_ij dS_ij |V_jc - o_ic| + sum_j w_ij [V_jc flagged] ulp(V_jc),
             dS_ij = sum_c [Q_ic flagged] ulp(Q_ic) |K_jc| + sum_c [K_jc flagged] ulp(K_jc) |Q_ic|.         Zero without `normalize`.

Reference.  w = softmax_j(ln2 * Q K^T), o = w V, float64.

Per-element bound (u_b = 2^-8, the unit roundoff of bf16 with its 8 significand bits; u = 2^-24).  The kernel contracts p~_j = p_j (1 + d_j), |d_j| <= u_b.
  folded form (D % 16 != 0: the denominator is the sum of the ROUNDED probabilities, row D of O^T):
        o^ - o = sum_j w_j d_j (V_j - o) / (1 + sum_k w_k d_k)      ->   B_p = u_b / (1 - u_b) * sum_j w_j |V_jc - o_c|
  plain form (D % 16 == 0: fp32 denominator of the unrounded probabilities):
        o^ - o = sum_j w_j d_j V_j                                   ->   B_p = u_b * sum_j w_j |V_jc|
  fp32 side, both forms:  B_32 = sum_j w_j e_ij |V_jc - o_c| + C_PV u sqrt(n_pv) sum_j w_j |V_jc| + 3 u |o_c|
        e_ij  = ln2 C_S u sqrt(Dp / 16 + 1) (sum_c |Q_ic K_jc| + max_j |s_ij| + THR) + C_EXP u: the relative perturbation of p_ij.  The logit is summed on the matrix
                core in Dp / 16 steps of 16 products; the folded form's reference point is one more product, the plain form's one more subtraction, and neither
                is larger than max |s| + THR (the deferred maximum lets the reference lag by 2^THR).  A perturbed p enters numerator and denominator alike, hence
                the factor |V - o|.  C_EXP = 2: v_exp_f32 is accurate to 1 ulp (CDNA ISA guide, "V_EXP_F32 ... 1 ULP").
        n_pv  = ceil(Lk / 16) + ceil(Lk / 64): the PV sum (and the folded denominator) takes one MFMA step per 16 keys and at most one rescale per tile; the plain
                denominator is a sum of the same length.  The last term: the reciprocal (1 ulp) and the final multiply.
  output: half an ulp of T (fp32 through td_attention, bf16 on the engine's own path) in the binade |o| + B reaches.
  Condition A, every element, nothing skipped, masked or averaged:          |hip - o| <= half_ulp_T + B_p + B_32 + E_flip.

Statistical conditions (families `random` and `moving`; on a selector input sigma vanishes and A alone judges).  The d_j are independent rounding errors; with a
  log-uniform significand sigma_rel = 2^-7 sqrt(0.541 / 12) = 2^-7 * 0.2124, sigma[i,c] = sigma_rel sqrt(sum_j w_ij^2 c_ijc^2), c = V_jc - o_ic (folded) or V_jc
  (plain).  z = |hip - o| / (sigma + B_32 + half_ulp_T + E_flip).
  Condition B: rms(z) over a case <= Z_RMS.      Condition C: max(z) <= sqrt(2 ln N_case) + Z_MAX_MARGIN (a Gaussian maximum over N elements, plus 3).

The scalar kernel (`scalar_reference`; fp16 / fp32 storage and bf16 with option attn_mfma = 0): all arithmetic in fp32 on the stored values, so B_p = 0.  From its loops,
  every sum sequential, worst case (no sqrt(n): at most 64 tokens): an operand x * inv carries 64 u (sum of 64 squares) / 2 + 2 (sqrtf) + 1 + 1 + 2 (reciprocal) + 1
  <= E_OP = 40 u;  a logit 64 products in sequence on two such operands: (65 + 2 E_OP) u sum_c |q k|;  expf 1 ulp and the subtraction of the maximum: (|s - max| + 2) u;
  denominator tokens / 4 + 2 additions;  PV tokens additions on an operand of E_OP;  reciprocal and final multiply 3:
        B_sc = sum_j w_j e_ij |V_jc - o_c| + (tokens + tokens / 4 + E_OP + 5) u sum_j w_j |V_jc|,    e_ij = ((65 + 2 E_OP) sum_c |q_ic k_jc| + |s_ij - max_j s_ij| + 2) u.

Inputs (`make_case`): `random` (the distributions of tests/test_gpu_attention.py); `selector`: keys are distinct integer vectors of EQUAL norm (sign vectors for D >= 8,
  each differing from its predecessor in one channel, so that a channel missing from the contraction makes two keys tie; signed permutations of 1..D for D = 3..7; the
  lattice points of the circle x^2 + y^2 = 325 for D = 2; +-1 for D = 1), q_i = 2 G_i k_target(i) with G_i = 32 (D >= 8: 32 / 45 / 59 by row, so that neighbouring
  rows of the folded form end with different denominators) and a scale for which f is exactly 1/2: logits are G k_t . k_j, the target wins by >= G >= 32 in log2
  units (equal norms: k_t . k_j = R - |k_t - k_j|^2 / 2 <= R - 1), its weight is >= 1 - Lk 2^-32.  Where D admits fewer distinct keys than Lk the case
  has fewer keys (D = 1: 2, D = 2: 24, D = 3: 48, D = 8: 128).  V_jc encodes (j mod 64, c) in bf16-exact values: significand 1 + ((j mod 16) + 3 (c / 16)) mod 16 / 16, exponent
  (j / 16) mod 4 + 4 ((c / 2) mod 8) - 16, sign by c mod 2 -- the 64 keys of a tile differ pairwise in every channel and the channels differ pairwise at every key, by
  >= 1/32 relative, more than 4 x the bound of condition A there (asserted by `selector_honesty`).  Targets: query 0 -> key Lk - 1 (in a ragged last tile the rows
  behind it are clamped COPIES of that key and only the mask keeps them out), then every residue mod 64 spread over the tiles, the first and the last tile.
  `moving`: shift -300 / +250 / spread 40 of test_attention_folded_reference_point_moves_both_ways, `late` (one dominant key in the last tile, > 2^8 above all before)
  and `early` (a dominant key in tile 0, everything after it far below).

Where the constants come from: `emulate` below, run by tests/test_attn_ops_cpu.py, which prints these numbers and asserts the margins (torch 2.10 CPU; 27 head dims at
70 x 150, 64 x 64 .. 128 x 4096, `normalize` on and off, the five moving families at d = 40 / 41 / 64 / 128); none is taken from a GPU kernel:
    logit accumulation   worst |s32 - s64| / (u sqrt(Dp/16 + 1) (sum |Q K| + max |s| + THR))        = 0.73     x 8 (the MFMA's summation tree is not the CPU's) -> C_S  = 6
    PV / denominator     worst |o32 - o64(same probabilities)| / (u sqrt(n_pv) sum_j w_j |V_jc|)      = 1.14     x 8                                              -> C_PV = 10
    exp2                 C_EXP = 2 from the ISA's statement (1 ulp)
    rms(z)               0.73 .. 1.06 on the random cases (the model predicts 1; 0.73 at 4096 keys, where B_32 is a third of z's denominator)   x 1.25 -> Z_RMS = 1.35
    max(z) - sqrt(2 ln N) worst -0.15 (N = 140 .. 8e4): a Gaussian maximum, as predicted                                                      Z_MAX_MARGIN = 3
  Mutations of the emulation (wrong-row denominator, leaked masked key, keys swapped inside a 16-group, a dropped 16-channel block of the logits): each breaks condition
  A on the selector inputs by a factor of 10^2 .. 10^10, and A, B and C on random inputs (rms(z) 10 .. 850).  Two limits, both by construction and both stated in the
  tests: on a one-hot row of the PLAIN form every denominator is exactly 1.0, so a neighbour's denominator is the same number -- that mutation is caught there by the
  random family only; and in the FOLDED form a leaked key cannot change the result: the clamped copy's V^T column and its entry of the denominator row are both zero
  padding -- that mutation is judged on plain-form head dims.  A key LOST from a diffuse softmax (weight 4e-4 median, 64 x 1000, d = 64) is seen by condition A on the
  8 queries that gave it more than 1.7e-3 and by no condition on the others: hence the selector family.
What the MI355X showed is in DESIGN.md, "How the attention kernels are checked".
"""
import math

import torch

U = 2.0 ** -24
UB = 2.0 ** -8
LN2 = math.log(2.0)
LOG2E32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
SIGMA_REL = 2.0 ** -7 * math.sqrt(0.541 / 12.0)
THR = 8.0
FLAG_U = 16.0
C_S, C_PV, C_EXP = 6.0, 10.0, 2.0
E_OP = 40.0
Z_RMS = 1.35
Z_MAX_MARGIN = 3.0
G_SEL = 32.0
G_ROWS = (32.0, 45.0, 59.0)     # per-query gains of the selector inputs (D >= 8: entries +-1, any integer gain is bf16-exact)
PREC = {"bf16": (8, -126), "fp16": (11, -14), "fp32": (24, -126)}
TORCH_T = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def fold_of(D):
    return D % 16 != 0


def dp_of(D):
    return (D + 15) // 16 * 16


def z_max(n):
    return math.sqrt(2.0 * math.log(max(n, 2))) + Z_MAX_MARGIN


def rne(x, T):
    return x.to(torch.float32).to(TORCH_T[T]).to(x.dtype)


def ulp(x, T):
    """unit in the last place of T in the binade the float64 x lies in"""
    p, emin = PREC[T]
    e = ((x.abs().contiguous().view(torch.int64) >> 52) & 0x7FF) - 1023
    return ((e.clamp_min(emin) - (p - 1) + 1023) << 52).view(torch.float64)


def pow2_scale():
    """an fp32 scale for which fp32(scale) * fp32(log2 e) is EXACTLY 1/2 in fp32 (the selector inputs: Q = q / 2 without a rounding)"""
    l2 = torch.tensor(LOG2E32, dtype=torch.float32)
    s = torch.tensor(0.5, dtype=torch.float32) / l2
    for _ in range(8):
        for cand in (s, torch.nextafter(s, torch.tensor(0.0)), torch.nextafter(s, torch.tensor(1.0))):
            if float(cand * l2) == 0.5:
                return float(cand)
        s = torch.nextafter(s, torch.tensor(0.0))
    raise AssertionError("no fp32 scale gives an exact 1/2")


# ------------------------------------------------------------------------------------------------ inputs
def _selector_keys(D, want, g):
    """`want` (or as many as D admits) distinct integer vectors of equal norm, (n, D) float32"""
    if D == 1:
        return torch.tensor([[1.0], [-1.0]])[:want]
    if D == 2:
        pts = []
        for a in range(1, 19):                        # x^2 + y^2 = 325 = 5^2 * 13: 24 lattice points (logits stay below 2^15)
            b2 = 325 - a * a
            b = int(round(math.sqrt(b2))) if b2 > 0 else 0
            if b > 0 and b * b == b2:
                pts += [(a, b), (a, -b), (-a, b), (-a, -b)]
        return torch.tensor(pts[:want], dtype=torch.float32)
    if D < 8:
        import itertools
        out = []
        for perm in itertools.permutations(range(1, D + 1)):
            for signs in range(1 << D):
                out.append([p if (signs >> i) & 1 else -p for i, p in enumerate(perm)])
                if len(out) >= 4 * want:
                    break
            if len(out) >= 4 * want:
                break
        idx = torch.randperm(len(out), generator=g)[:want]
        return torch.tensor(out, dtype=torch.float32)[idx]
    want = min(want, 1 << min(D - 1, 30))
    cur = (torch.randint(0, 2, (D,), generator=g) * 2 - 1).tolist()
    seen, rows = {tuple(cur)}, [list(cur)]
    j = 0
    while len(rows) < want:
        cur[(j * 37) % D] *= -1                       # one channel away from the predecessor: the walk visits every 16-channel block
        while tuple(cur) in seen:
            cur[int(torch.randint(0, D, (1,), generator=g))] *= -1
        seen.add(tuple(cur)); rows.append(list(cur)); j += 1
    return torch.tensor(rows, dtype=torch.float32)


def _selector_values(Lk, D):
    j = torch.arange(Lk).view(Lk, 1)
    c = torch.arange(D).view(1, D)
    sig = 1.0 + (((j % 16) + 3 * (c // 16)) % 16).double() / 16.0
    ex = ((j // 16) % 4 + 4 * ((c // 2) % 8) - 16).double()
    return (torch.where(c % 2 == 1, -1.0, 1.0) * sig * torch.exp2(ex)).to(torch.float32)


def selector_targets(Lq, Lk):
    nt = (Lk + 63) // 64
    t = [Lk - 1]
    for r in range(min(64, Lk)):
        k = r + 64 * (r % nt)
        t.append(k if k < Lk else k - 64)
    t += [0, 64 * (nt - 1)]
    g = torch.Generator().manual_seed(Lq * 131 + Lk)
    while len(t) < Lq:
        t.append(int(torch.randint(0, Lk, (1,), generator=g)))
    return t[:Lq]


def make_case(kind, B, H, Lq, Lk, D, seed, normalize=False):
    """deterministic inputs: dict(q, k, v [fp32, (B, H, L, D)], scale, normalize, kind, [target (B, H, Lq)])"""
    g = torch.Generator().manual_seed(seed)
    scale = 1.0 / math.sqrt(D)
    case = dict(kind=kind, normalize=bool(normalize), D=D)
    if kind == "random":
        q, k, v = (torch.randn(B, H, L, D, generator=g) * s for L, s in ((Lq, 1.3), (Lk, 0.9), (Lk, 2.0)))
    elif kind == "selector":
        assert not normalize
        keys = _selector_keys(D, Lk, g)
        Lk = keys.shape[0]
        vals = _selector_values(Lk, D)
        base = torch.tensor(selector_targets(Lq, Lk))
        k = torch.empty(B, H, Lk, D); v = torch.empty(B, H, Lk, D); q = torch.empty(B, H, Lq, D)
        tg = torch.empty(B, H, Lq, dtype=torch.long)
        for b in range(B):
            for h in range(H):
                bh = b * H + h
                k[b, h] = torch.roll(keys, bh, 0)                      # another key set per head: a wrong head or batch stride reads another key
                v[b, h] = vals * 2.0 ** (bh % 3)
                tg[b, h] = torch.cat([base[:1], torch.roll(base[1:], 5 * bh)])
                gain = torch.tensor(G_ROWS if D >= 8 else (G_SEL,) * 3)[torch.arange(Lq) % 3].view(Lq, 1)
                q[b, h] = 2.0 * gain * k[b, h][tg[b, h]]
        scale = pow2_scale()
        case["target"] = tg
    else:
        q, k, v = (torch.randn(B, H, L, D, generator=g) for L in (Lq, Lk, Lk))
        c = 4.0
        q[..., 0] = c
        if kind in ("shift-300", "shift+250"):
            k[..., 0] = float(kind[5:]) / (c * scale)
        elif kind == "spread40":
            k[..., 0] = 0.0
            k = k * torch.linspace(1.0, 40.0, Lk).view(1, 1, Lk, 1)
        elif kind == "late":
            k[..., 0] = 0.0
            k[:, :, Lk - 3, 0] = 400.0 / (c * scale)       # 577 in log2 units: > 2^8 above every key before it, in the last tile
        elif kind == "early":
            k[..., 0] = 0.0
            k[:, :, 1, 0] = 60.0 / (c * scale)             # everything behind key 1 lies ~2^-86 below it
        else:
            raise ValueError(kind)
    case.update(q=q.contiguous(), k=k.contiguous(), v=v.contiguous(), scale=float(torch.tensor(scale, dtype=torch.float32)))
    return case


# ------------------------------------------------------------------------------------------------ operands
def _inv32(x, D):
    """the pack kernels' 1 / (1e-4 + sqrt(ss) / sqrt(D)) in fp32: lane = channel mod 64, squares added per lane in ascending order, xor butterfly 32 .. 1"""
    f32 = torch.float32
    pad = 192 - D
    xp = torch.nn.functional.pad(x.to(f32), (0, pad)).reshape(*x.shape[:-1], 3, 64)
    sq = xp * xp
    ss = (sq[..., 0, :] + sq[..., 1, :]) + sq[..., 2, :]
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        ss = ss + ss[..., lanes ^ o]
    ss = ss[..., :1]
    return 1.0 / (torch.tensor(1e-4, dtype=f32) + torch.sqrt(ss) / torch.sqrt(torch.tensor(float(D), dtype=f32)))


def pack_operands(case, dev="cpu"):
    """dict(Q, K, V: the bf16 operands as float64; Q64, K64, V64: their float64 values before the rounding; FQ, FK, FV: one bf16 ulp where flagged, else 0)"""
    D = case["D"]
    f = torch.tensor(case["scale"], dtype=torch.float32) * torch.tensor(LOG2E32, dtype=torch.float32)
    out = {}
    for name, post in (("q", f), ("k", None), ("v", None)):
        x = case[name].to(torch.float32)
        if case["normalize"]:
            inv = _inv32(x, D)
            if post is not None:
                inv = inv * post
            a32 = x * inv
            x64 = x.double()
            inv64 = 1.0 / (float(torch.tensor(1e-4, dtype=torch.float32)) + x64.pow(2).sum(-1, keepdim=True).sqrt() / math.sqrt(D))
            a64 = x64 * (inv64 * float(post) if post is not None else inv64)
            ul = ulp(a64, "bf16")
            fr = a64 / ul
            near = (fr - torch.floor(fr) - 0.5).abs() * ul <= FLAG_U * U * a64.abs()
            flag = torch.where(near, ul, torch.zeros_like(ul))
        else:
            a32 = x * post if post is not None else x
            a64 = a32.double()
            flag = torch.zeros_like(a64)
        N = name.upper()
        out[N] = a32.to(torch.bfloat16).double().to(dev)
        out[N + "64"] = a64.to(dev)
        out["F" + N] = flag.to(dev)
    return out


# ------------------------------------------------------------------------------------------------ the reference and the bound
def reference(ops, D, normalize=False, budget=1 << 24):
    """float64 attention on the packed operands and every term of the criterion, each (B, H, Lq, D): o, Bp, B32, Eflip, sigma; `maxw` (B, H, Lq)"""
    Q, K, V = ops["Q"], ops["K"], ops["V"]
    B, H, Lq, _ = Q.shape
    Lk = K.shape[2]
    fold = fold_of(D)
    ksteps = dp_of(D) // 16 + 1
    n_pv = (Lk + 15) // 16 + (Lk + 63) // 64
    res = {k_: torch.empty_like(Q) for k_ in ("o", "Bp", "B32", "Eflip", "sigma")}
    res["maxw"] = torch.empty(Q.shape[:3], dtype=torch.float64, device=Q.device)
    cc = max(1, min(D, budget // max(1, Lq * Lk)))
    for b in range(B):
        for h in range(H):
            q, k, v = Q[b, h], K[b, h], V[b, h]
            s = q @ k.T
            w = torch.exp2(s - s.max(-1, keepdim=True).values)
            w = w / w.sum(-1, keepdim=True)
            o = w @ v
            A1 = w @ v.abs()
            e = LN2 * C_S * U * math.sqrt(ksteps) * (q.abs() @ k.abs().T + s.abs().max(-1, keepdim=True).values + THR) + C_EXP * U
            g1 = w * e
            g2 = None
            if normalize:
                g2 = w * LN2 * (ops["FQ"][b, h] @ k.abs().T + q.abs() @ ops["FK"][b, h].T)
            A2, X1, X2 = torch.empty_like(o), torch.empty_like(o), torch.zeros_like(o)
            for c0 in range(0, D, cc):
                diff = (v[None, :, c0:c0 + cc] - o[:, None, c0:c0 + cc]).abs()
                A2[:, c0:c0 + cc] = torch.einsum("ij,ijc->ic", w, diff)
                X1[:, c0:c0 + cc] = torch.einsum("ij,ijc->ic", g1, diff)
                if normalize:
                    X2[:, c0:c0 + cc] = torch.einsum("ij,ijc->ic", g2, diff)
                del diff
            w2 = w * w
            if fold:
                sig2 = (w2 @ (v * v) - 2.0 * o * (w2 @ v) + o * o * w2.sum(-1, keepdim=True)).clamp_min(0.0)
                Bp = UB / (1.0 - UB) * A2
            else:
                sig2 = w2 @ (v * v)
                Bp = UB * A1
            res["o"][b, h] = o
            res["Bp"][b, h] = Bp
            res["B32"][b, h] = X1 + C_PV * U * math.sqrt(n_pv) * A1 + 3.0 * U * o.abs()
            res["Eflip"][b, h] = X2 + (w @ ops["FV"][b, h] if normalize else 0.0)
            res["sigma"][b, h] = SIGMA_REL * sig2.sqrt()
            res["maxw"][b, h] = w.max(-1).values
    return res


def scalar_reference(q, k, v):
    """the scalar attn_kernel's float64 twin on the STORED q, k, v (B, H, L, 64): per-token unit-RMS norm, logits / 8, softmax, and B_sc (see the module docstring)"""
    q, k, v = q.double(), k.double(), v.double()
    nrm = lambda x: x / (1e-4 + x.pow(2).sum(-1, keepdim=True).sqrt() * 0.125)
    q, k, v = nrm(q), nrm(k) * 0.125, nrm(v)
    L = q.shape[2]
    s = q @ k.transpose(-1, -2)
    smax = s.max(-1, keepdim=True).values
    w = torch.exp(s - smax)
    w = w / w.sum(-1, keepdim=True)
    o = w @ v
    A1 = w @ v.abs()
    e = ((65.0 + 2.0 * E_OP) * (q.abs() @ k.abs().transpose(-1, -2)) + (s - smax).abs() + 2.0) * U
    diff = (v[:, :, None, :, :] - o[:, :, :, None, :]).abs()
    X1 = torch.einsum("bhij,bhijc->bhic", w * e, diff)
    zero = torch.zeros_like(o)
    return dict(o=o, Bp=zero, B32=X1 + (L + L / 4.0 + E_OP + 5.0) * U * A1, Eflip=zero, sigma=zero, maxw=w.max(-1).values)


def measure(hip, ref, T="fp32", name=""):
    """the statistics of one case against the three conditions, nothing asserted; returns (statistics, the tensors bad, ratio, z)"""
    o = ref["o"]
    assert hip.shape == o.shape, (tuple(hip.shape), tuple(o.shape))
    E = ref["Bp"] + ref["B32"] + ref["Eflip"]
    half = 0.5 * ulp(o.abs() + E, T)
    err = (hip - o).abs()
    bad = ~(err <= half + E)                                   # (a NaN fails)
    ratio = (err / (half + E)).nan_to_num(nan=float("inf"))
    z = (err / (ref["sigma"] + ref["B32"] + half + ref["Eflip"])).nan_to_num(nan=float("inf"))
    n = o.numel()
    st = dict(name=name, n=n, bad=int(bad.sum()), worstA=float(ratio.max()), rms_z=float(z.pow(2).mean().sqrt()), max_z=float(z.max()),
              z_max=z_max(n), exact=float((hip == rne(o, T).to(hip.dtype)).double().mean()), loose=float((ref["Bp"] / o.abs().clamp_min(1e-300)).median()))
    return st, bad, ratio, z


def check(hip, ref, T="fp32", name="", stat=True):
    """Conditions A (always), B and C (stat) on one case.  hip: the kernel's output as float64.  Returns the statistics; raises AssertionError naming the worst element."""
    st, bad, ratio, z = measure(hip, ref, T, name)
    o, n = ref["o"], st["n"]
    if st["bad"]:
        wi = [int(i) for i in torch.unravel_index(torch.where(bad, ratio, torch.zeros_like(ratio)).argmax(), ratio.shape)]
        idx = bad.nonzero()
        raise AssertionError(f"{name}: {st['bad']} of {n} elements outside half_ulp + B_p + B_32 + E_flip; worst at (b, h, query, channel) = {tuple(wi)}: "
                             f"hip {float(hip[tuple(wi)]):.9g} ref {float(o[tuple(wi)]):.9g}, error {st['worstA']:.3g} x the bound; failing queries "
                             f"{int(idx[:, 2].min())}..{int(idx[:, 2].max())}, channels {int(idx[:, 3].min())}..{int(idx[:, 3].max())}")
    if stat:
        assert st["rms_z"] <= Z_RMS, f"{name}: rms(z) = {st['rms_z']:.3f} > {Z_RMS} (condition B)"
        if st["max_z"] > st["z_max"]:
            wi = [int(i) for i in torch.unravel_index(z.argmax(), z.shape)]
            raise AssertionError(f"{name}: max(z) = {st['max_z']:.2f} > sqrt(2 ln {n}) + {Z_MAX_MARGIN} = {st['z_max']:.2f} (condition C) at (b, h, query, channel) = {tuple(wi)}")
    return st


def line(st):
    return (f"{st['name']}: {st['n']} elements, A violations {st['bad']}, worst |err| / bound {st['worstA']:.3f}, rms(z) {st['rms_z']:.3f}, max(z) {st['max_z']:.2f} "
            f"(<= {st['z_max']:.2f}), == RNE(float64) on {100.0 * st['exact']:.1f} %, median B_p / |o| {st['loose']:.1e}")


def selector_honesty(case, ref, T="fp32", full=True):
    """the conditions that make a selector case name the key and the channel that were read, asserted on the twin's own float64 weights"""
    assert float(ref["maxw"].min()) >= 1.0 - 2.0 ** -20, float(ref["maxw"].min())
    tg = case["target"]
    Lk = case["k"].shape[2]
    if full:
        for b in range(tg.shape[0]):
            for h in range(tg.shape[1]):
                t = tg[b, h]
                assert set((t % 64).tolist()) >= set(range(min(64, Lk))), "every key residue mod 64 is some query's target"
                assert int(t[0]) == Lk - 1 and int(t.min()) < 64 and int(t.max()) >= 64 * ((Lk - 1) // 64)
    # V entries a wrong key (same tile, same channel) or a wrong channel (same key) could confuse: >= 1/32 of the larger apart; the bound of condition A relative to
    # the value it belongs to must be less than a quarter of that
    v = case["v"][0, 0].double()
    for blk in range(0, Lk, 64):
        t = v[blk:blk + 64]
        d = (t[:, None, :] - t[None, :, :]).abs() / torch.maximum(t[:, None, :].abs(), t[None, :, :].abs())
        d = d + torch.eye(t.shape[0], dtype=torch.float64)[:, :, None]
        assert float(d.min()) >= 1.0 / 32.0, ("keys", blk, float(d.min()))
    d = (v[:, :, None] - v[:, None, :]).abs() / torch.maximum(v[:, :, None].abs(), v[:, None, :].abs()) + torch.eye(v.shape[1], dtype=torch.float64)[None]
    assert float(d.min()) >= 1.0 / 32.0, ("channels", float(d.min()))
    E = ref["Bp"] + ref["B32"] + ref["Eflip"]
    bound = (0.5 * ulp(ref["o"].abs() + E, T) + E) / ref["o"].abs()
    assert 4.0 * float(bound.max()) < 1.0 / 32.0, float(bound.max())
    return float(bound.max())


# ------------------------------------------------------------------------------------------------ the emulation
def emulate(case, mutate=None, ratios=None, out_T="fp32"):
    """The flash kernel's arithmetic in torch fp32 / bf16 on the CPU: 64-key tiles, 16 products per accumulate step, per-32-query deferred maximum (THR = 8),
    bf16-rounded reference point in a padding channel (folded form), bf16 probabilities, the two denominator forms.  mutate: 'wrong_row_den', 'leaked_key',
    'swapped_keys', 'dropped_block' (deliberately broken kernels, for the tests of the criterion).  Returns the output as float64 (B, H, Lq, D)."""
    f32, f64 = torch.float32, torch.float64
    D = case["D"]
    ops = pack_operands(case)
    B, H, Lq, _ = ops["Q"].shape
    Lk = ops["K"].shape[2]
    fold, Dp = fold_of(D), dp_of(D)
    BH, Lqp, nt = B * H, (Lq + 31) // 32 * 32, (Lk + 63) // 64
    Q = torch.zeros(BH, Lqp, Dp, dtype=f64); Q[:, :Lq, :D] = ops["Q"].reshape(BH, Lq, D)
    K = torch.zeros(BH, nt * 64, Dp, dtype=f64); K[:, :Lk, :D] = ops["K"].reshape(BH, Lk, D)
    K[:, Lk:] = K[:, Lk - 1:Lk]                                  # rows behind Lk: clamped copies of the last key
    Dv = D + 1 if fold else D
    V = torch.zeros(BH, nt * 64, Dv, dtype=f64); V[:, :Lk, :D] = ops["V"].reshape(BH, Lk, D)
    if fold:
        K[:, :, D] = 1.0                                         # (the copies carry it too: they are copies of a packed row)
        V[:, :Lk, D] = 1.0                                       # the denominator row: real keys only
    O = torch.zeros(BH, Lqp, Dv, dtype=f32); O64 = torch.zeros(BH, Lqp, Dv, dtype=f64)
    m_run = torch.full((BH, Lqp), -3.0e38, dtype=f32)
    m_ref = torch.zeros(BH, Lqp, dtype=f32)
    l_run = torch.zeros(BH, Lqp, dtype=f32); l64 = torch.zeros(BH, Lqp, dtype=f64)
    wave_any = lambda m: m.reshape(BH, Lqp // 32, 32).any(-1, keepdim=True).expand(BH, Lqp // 32, 32).reshape(BH, Lqp)
    s_ratio = 0.0
    lim = Lk + 1 if mutate == "leaked_key" else Lk
    for t in range(nt):
        kt, vt = K[:, t * 64:(t + 1) * 64], V[:, t * 64:(t + 1) * 64]
        if fold:
            Q[:, :, D] = -m_ref.double()
        s = torch.zeros(BH, Lqp, 64, dtype=f32)
        for ks in range(Dp // 16):
            if mutate == "dropped_block" and ks == 0:
                continue
            s = s + (Q[:, :, ks * 16:ks * 16 + 16] @ kt[:, :, ks * 16:ks * 16 + 16].transpose(1, 2)).to(f32)
        if ratios is not None and mutate is None:
            s64 = Q @ kt.transpose(1, 2)
            den = U * math.sqrt(Dp // 16 + 1) * (Q.abs() @ kt.abs().transpose(1, 2) + s64.abs().amax(-1, keepdim=True) + THR)
            s_ratio = max(s_ratio, float(((s.double() - s64).abs() / den)[:, :Lq].max()))
        key = t * 64 + torch.arange(64)
        s = torch.where((key >= lim).view(1, 1, 64), torch.tensor(-3.0e38, dtype=f32), s)
        mt = s.amax(-1)
        if fold:
            m_run = torch.maximum(m_run, mt)
            moved = wave_any((mt > THR) | (m_run < -64.0))
            mr_new = (m_ref + m_run).to(torch.bfloat16).to(f32)
            delta = torch.where(moved, mr_new - m_ref, torch.zeros_like(m_ref))
            alpha = torch.where(moved, torch.exp2(torch.minimum(-delta, torch.tensor(64.0))), torch.ones_like(delta))
            m_ref = m_ref + delta; m_run = m_run - delta
            s = s - delta[..., None]
            p = torch.exp2(s)
        else:
            moved = wave_any(mt > m_run + THR)
            m_new = torch.where(moved, torch.maximum(m_run, mt), m_run)
            alpha = torch.where(moved, torch.exp2(m_run - m_new), torch.ones_like(m_run))
            p = torch.exp2(s - m_new[..., None])
            l_run = l_run * alpha + p.sum(-1)
            l64 = l64 * alpha.double() + p.double().sum(-1)
            m_run = m_new
        pb = p.to(torch.bfloat16).double()
        O = O * alpha[..., None]; O64 = O64 * alpha.double()[..., None]
        if mutate == "swapped_keys":                              # the V^T key order {0-3, 8-11, 4-7, 12-15} forgotten on one side
            perm = torch.arange(64)
            perm = (perm & ~15) | (perm & 3) | (((perm >> 3) & 1) << 2) | (((perm >> 2) & 1) << 3)
            vt = vt[:, perm]
        for st in range(4):
            part = pb[:, :, st * 16:st * 16 + 16] @ vt[:, st * 16:st * 16 + 16]
            O = O + part.to(f32); O64 = O64 + part
    if fold:
        den, den64 = O[:, :, D], O64[:, :, D]
    else:
        den, den64 = l_run, l64
    if mutate == "wrong_row_den":
        den = den[:, torch.arange(Lqp) ^ 1]
    out = O[:, :Lq, :D] * (1.0 / den)[:, :Lq, None]
    if ratios is not None and mutate is None:
        o64 = O64[:, :Lq, :D] / den64[:, :Lq, None]
        r = reference(ops, D, case["normalize"])
        A1 = (r["Bp"] / UB).reshape(BH, Lq, D) if not fold else None
        if A1 is None:                                           # sum_j w_j |V_jc|: from the operands
            w = torch.softmax(LN2 * (ops["Q"] @ ops["K"].transpose(-1, -2)), -1)
            A1 = (w @ ops["V"].abs()).reshape(BH, Lq, D)
        n_pv = (Lk + 15) // 16 + (Lk + 63) // 64
        ratios["acc_s"] = max(ratios.get("acc_s", 0.0), s_ratio)
        ratios["acc_pv"] = max(ratios.get("acc_pv", 0.0), float(((out.double() - o64).abs() / (U * math.sqrt(n_pv) * A1).clamp_min(1e-300)).max()))
    out = out.reshape(B, H, Lq, D)
    return (out.to(torch.bfloat16) if out_T == "bf16" else out).double()


# ------------------------------------------------------------------------------------------------ the engine's own path
def split_qkv(qkv):
    """a stored attn_qkv output (n, 3C, h, w), channel = (head * 64 + d) * 3 + {q, k, v}  ->  q, k, v (n, heads, h * w, 64) float32"""
    n, c3, h, w = qkv.shape
    y = qkv.to(torch.float32).reshape(n, c3 // 192, 64, 3, h * w)
    return tuple(y[:, :, :, i].transpose(2, 3).contiguous() for i in range(3))


def merge_heads(att):
    """a stored attention output (n, C, h, w), channel = head * 64 + d  ->  (n, heads, h * w, 64)"""
    n, C, h, w = att.shape
    return att.reshape(n, C // 64, 64, h * w).transpose(2, 3)


def check_engine_attention(qkv, att, T, mfma, name="", dev="cpu"):
    """the engine's attention op on its own stored input: `mfma` (bf16 storage, option attn_mfma = 1): attn_pack_qkv64_kernel + flash kernel + bf16 store, conditions
    A, B, C; otherwise the scalar attn_kernel, condition A with B_sc"""
    q, k, v = split_qkv(qkv)
    hip = merge_heads(att).double().to(dev)
    if mfma:
        assert T == "bf16"
        case = dict(q=q, k=k, v=v, scale=0.125, normalize=True, D=64, kind="engine")
        ref = reference(pack_operands(case, dev), 64, True)
        return check(hip, ref, "bf16", name, stat=True)
    ref = scalar_reference(q.to(dev), k.to(dev), v.to(dev))
    return check(hip, ref, T, name, stat=False)
