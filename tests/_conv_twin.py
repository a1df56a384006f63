"""Host model ("twin") of every fused conv op of the U-Net engine, in plain torch float64, and the element-wise criterion it is held to.

What it is.  `describe_ae(cfg, kind)` is the same for the two stacks of the EDMAutoencoder (tests/_ae_twin.py's plan; tests/test_ae_conv_ops_cpu.py holds both
op lists to csrc/model_graph.h field for field).  `describe(cfg)` walks `oracle.unet.build_plan(cfg)` and restates, op by op, what `build_plan` / `finalize` in
`terrain_diffusion_amd/csrc/engine.hip` emit: the K-segments of each fused conv (source op, real channels, taps, resample, transform), the weight
slice and its `mul` factor, the epilogue and the output type.  `Twin.eval(op, stored, cvec)` computes ONE op in float64 FROM THE TENSORS THE
ENGINE STORED (the outputs of the producing ops as `read_activation` returns them), so an error cannot hide behind the layers in front of it or be
diluted by the layers behind it.  `check_op` then holds every element of the op's stored output to

    |hip - ref| <= half_ulp_T(ref) + E,      E = E_acc + E_epi + E_pro          (every op, `attn_proj` included: it reads the STORED attention output)

Nothing here imports `terrain_diffusion_amd`; torch shares no code with the engine.

The model of one op
  operand   a_k = RNE_T(xform(resample(x)))      xform 0: x;  1: mp_silu(scale * x);  2: mp_silu(rn * x), rn = 1 / (1e-4 + sqrt(sum_c x^2 / C))
  weight    w_k = RNE_T(fp32(w_folded) * fp32(mul))          (`fold_host` below; mul = 1, kMixNew, kMixRes * sa, kMixRes * sb; no RNE in fp32 mode)
  K sum     v   = sum_k a_k w_k                               (float64)
  epilogue  EPI_PLAIN v;  EPI_EMB_SILU mp_silu(v * c[n, co]);  EPI_RESIDUAL clip(v + kMixRes * [rn] * res, +-256 where the plan clips)
  returned  ref (before the output rounding), s = g * sqrt(sum_k (a_k w_k)^2), K = number of real products; g = |d ref / d v| (1, or the slope of the
            modulated mp_silu), so that s is the scale of the K sum AT THE OUTPUT; and the three parts of E.

The slack E (three named parts; u = 2^-24)
  accumulation   E_acc = C_ACC * u * sqrt(S) * sqrt(s0^2 + v^2), pushed through the epilogue (s0 = s before that).  The matrix core sums 16 products
                 (4 in fp32 mode, C_ACC32) and adds that to its fp32 accumulator: S roundings, S = `acc_steps` = sum over the K-segments of taps * ceil(C / 16),
                 which is K / 16 for every block conv.  (First stated as K / 16 for all ops.  The autoencoder's 3x3 input conv of 1 + 1 or 2 + 1 channels showed
                 that to be wrong where a few real channels sit in a padded chunk: 9 accumulate steps, not 18 / 16, and an emulation ratio of 3.42 / 3.72 in fp16
                 under the K / 16 form, 1.5 / 1.3 over S (the same errors over the right count); the count was corrected, C_ACC was not touched.  The U-Net's input conv, 5 + 1 channels, has
                 S = 9 against 54 / 16 as well, and `decoder_conv` S = 1.  For that one U-Net op the corrected count LOOSENS the criterion its GPU arms already held:
                 E_acc of `enc.*_conv` grows by sqrt(9 / 3.375) = 1.63 in bf16 and fp16 and by sqrt(18 / 13.5) = 1.15 in fp32, every other U-Net op keeps its S.  The basis is
                 the count itself -- one rounding per tap per real channel group, none for the all-zero groups -- and the CPU emulation, not a GPU measurement.)  Each rounding is relative to the running sum -- whose random part
                 scales with s0 and whose coherent part with |v|.  With s0 alone (the form first tried) the worst emulation ratios come from 1x1 convs of
                 pixel-normed inputs, whose terms share a sign (3.9 - 4.5 against 2.0 - 2.3 with the v term), and the constant they force makes
                 E_acc / half_ulp > 0.5 on the K = 1536 * 9 layers in fp16: the model was tightened, not the condition.
  epilogue       E_epi = C_EPI * u * m * (1 + |t| sig(t))         m = |ref| (EMB_SILU) or |v| + |residual term| (RESIDUAL); 0 for EPI_PLAIN (no arithmetic);
                 t = the exponent argument of exp2, whose rounding is amplified by |t| ln 2 on the side of the sigmoid that matters (sig(t) = e^t / (1 + e^t)).
                 A normed residual adds u * e_rn * |term| (e_rn below).  An error e of the K sum reaches the output of EMB_SILU as
                 sup |mp_silu(z') - mp_silu(z)| over |z' - z| <= |c| e (`_through_silu`: not linearised, the tail of the silu is too curved for that).
  prologue       The activation is evaluated in fp32 as (x k2) rcp(1 + exp2(x k1)) and THEN rounded to 16 bits, so an operand sometimes lands one ulp_T
                 from RNE_T(float64 value).  The statistical form  c * ulp_T(1) * sqrt(p_flip) * s  fails the median condition below: with p_flip ~ 2^-15 an
                 output sees 0.05 flips, the worst of 10^6 outputs is one flip of a 4-sigma product, 17 x the model, so c ~ 60 and E ~ 1.3 half-ulps.
                 Tightened instead: the twin evaluates the activation in fp32 IN THE KERNELS' OWN FORM (the multiplies and the add are IEEE and
                 reproduce; rn comes from the engine's own sum-of-squares planes, added in ascending order in fp32 as pixel_rn does), so only v_exp_f32 and
                 v_rcp_f32 can differ from torch's exp2 and reciprocal: 1 ulp each by the ISA's statement, <= 1 ulp each for torch's, two roundings behind
                 them -> d_k = u |a_k| (C_PRO + e_rn (1 + |t| sig(t))), C_PRO = 6.  The twin knows WHICH operands can flip -- those within d_k of a rounding
                 boundary of T -- and
                     E_pro = sum_k [a_k can flip] * ulp_T(a_k) * |w_k|            (one extra conv of the flagged ulps with |w|)
                 a deterministic bound, zero for ~95 % of the outputs.  In fp32 mode there is no operand rounding and the same conv carries d_k itself.
                 Zero for transform-0 segments (the stored tensor IS the operand).
  e_rn           allowance for rn in u: 2 with the producer's planes (sqrt and the division, should either not be correctly rounded); 6 when the producer ran
                 on the 64 px x 16 cout flavour, of whose planes the reader returns the first half (the rest restated in fp32 from the stored tensor: another
                 order inside each 16); E_RN(C) = 2 sqrt(C) + 3 without planes (float64 rn against fp32 sums of C squares, see C_SS).
  half_ulp_T     of the binade |ref| + E reaches: RNE acts on the value the kernel holds, which lies within E of ref.
  attention      `attn_proj` is an ordinary 1x1 conv of the attention op's stored output (`read_activation("<block>.attn")`).  The attention op itself -- from the
                 stored `attn_qkv` output to that tensor -- is held to its own element-wise criterion, tests/_attn_twin.py (`check_forward` runs it per block).

Where the constants come from.  Not from the GPU kernels.  `Twin.emulate` evaluates the same op models in float32 with the kernels' operand and output
rounding, the kernels' activation form and 16 (4) products per accumulate step; tests/test_conv_ops_cpu.py runs it, asserts zero violations and prints
these ratios (worst over the tiny attention model in bf16 / fp16 / fp32 and the base model in bf16 on a 32 x 32 map; torch 2.10 CPU, +-5 % from run to run
with the threading of the sums):
    accumulation, 16-bit   worst |v32 - v64| / (u sqrt(K / 16) sqrt(s0^2 + v^2)) = 2.26     x 8 (the MFMA's summation tree is not the CPU's) -> C_ACC   = 20
    accumulation, fp32     worst, K / 4                                           = 1.74     x 8                                              -> C_ACC32 = 16
                           (as recorded when the constants were fixed, over K / 16 resp. K / 4.  Over S = `acc_steps`, which differs for the input conv only, the same four
                           runs give 1.99 / 1.84 / 2.07 in bf16 / fp16 / base bf16 and 1.74 in fp32: the constants keep their factor of 8.)
    epilogue               worst |epi32 - epi64| / (u m (1 + |t| sig(t)))         = 4.93     x 4                                              -> C_EPI   = 22
    prologue               C_PRO = 6 from the ISA's statements as above; the emulation's activation IS the twin's, so it has no ratio of its own.  For the
                           record: fp32 form against float64, |a32 - a64| / (u |a| (1 + |t| sig(t))) = 4.9 (transform 1), 6.0 (transform 2, fp32 sums).
    sum of squares         worst |ss32 - ss64| / (u sqrt(C) ss) = 0.42 x 4 -> C_SS = 4 (>= 1.7), capped by the worst case C u

The two conditions that keep the criterion honest, both asserted by `check_op`: no element is skipped, masked or averaged; and for every 16-bit op the
median over its elements of (E_acc + E_epi + E_pro) / half_ulp_T(ref) is <= 0.5 (elements with |ref| < 2^-6 rms(ref) are left out of THAT STATISTIC only:
near zero the half-ulp vanishes while E does not).  Largest median per run: CPU emulation 0.04 (base bf16, enc.64x64_block2.conv_res0), 0.02 (tiny bf16),
0.19 (tiny fp16, dec.128x128_block0.conv_res0); MI355X 0.02 - 0.04 in every bf16 arm, 0.32 / 0.38 in the fp16 arms (n = 64 / n = 1).
The autoencoder's stacks (tests/test_ae_conv_ops_cpu.py has their ratio table, tests/test_ae_conv_ops_gpu.py the arms): CPU emulation 0.016 (released bf16), 0.169
(released fp16, encoder.enc.64x64_down.conv_res0); MI355X 0.006 - 0.041 in every bf16 arm, 0.118 / 0.222 / 0.215 in the fp16 arms (decoder / encoder / dihedral encoder).
What else the MI355X showed is in DESIGN.md, "How the conv kernels are checked".

Run as a script on a GPU box for a per-op table of one forward:  python tests/_conv_twin.py [bf16|fp16|fp32] [n]
"""
import math
import re
import time

import torch
import torch.nn.functional as F

from oracle.unet import OracleUnet, build_plan, fold_weight, mp_concat_scales

U = 2.0 ** -24
C_ACC, C_ACC32, C_EPI, C_PRO, C_SS = 20.0, 16.0, 22.0, 6.0, 4.0
MEDIAN_MAX = 0.5
LOG2E = 1.4426950408889634
MIX_DEN = math.sqrt(0.7 ** 2 + 0.3 ** 2)
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
# engine.hip: kMixRes = 0.7f / 0.76157731058639082f, kMixNew = 0.3f / 0.76157731058639082f (fp32 divisions)
KMIX_RES32 = float(torch.tensor(0.7, dtype=torch.float32) / torch.tensor(0.76157731058639082, dtype=torch.float32))
KMIX_NEW32 = float(torch.tensor(0.3, dtype=torch.float32) / torch.tensor(0.76157731058639082, dtype=torch.float32))
KMIX_RES64, KMIX_NEW64 = 0.7 / MIX_DEN, 0.3 / MIX_DEN
TORCH_T = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": None}
PREC = {"bf16": (8, -126), "fp16": (11, -14)}     # significand bits (with the hidden one), exponent of the smallest normal


def E_RN(C):
    return 2.0 * math.sqrt(C) + 3.0


E_RN_F5 = 6.0               # ... and half of the planes restated from the stored tensor (see Twin._rn)
E_RN_PLANES = 2.0           # rn from the engine's own planes: sqrt and the division, should either not be correctly rounded


# ------------------------------------------------------------------------------------------------ number formats
def rne(x, T):
    """x (float32 or float64) rounded to storage type T, returned in x's dtype"""
    t = TORCH_T[T]
    return x if t is None else x.to(torch.float32).to(t).to(x.dtype)


def ulp(x, T):
    """unit in the last place of T in the binade x lies in (the subnormal spacing below the smallest normal)"""
    p, emin = PREC[T]
    e = ((x.abs().contiguous().view(torch.int64) >> 52) & 0x7FF) - 1023          # exponent field of the double: exact, on any device
    return ((e.clamp_min(emin) - (p - 1) + 1023) << 52).view(torch.float64)


def _mul32(*f):
    """product of fp32 factors in fp32, left to right (the engine's `kMixRes * sa`)"""
    r = torch.tensor(f[0], dtype=torch.float32)
    for v in f[1:]:
        r = r * torch.tensor(v, dtype=torch.float32)
    return float(r)


def fold_host(w, gain=1.0):
    """The folded fp32 weight the engine is handed (prefolded = 1): MPConv.forward's eval-mode arithmetic as torch executes it in the reference,
    W / add(1e-4, ||W||, alpha = sqrt(1 / numel)) * (gain / sqrt(fan_in)).  `oracle.unet.fold_weight` writes the same formula as eps + norm * alpha: torch's
    add-with-alpha is one fused multiply-add there, the norm differs by one fp32 ulp for some tensors and with it nearly every weight of those tensors -- one
    16-bit rounding flip in ~2^-16 of them, which this criterion sees (the first MI355X run of these tests failed on exactly that, on three output channels of
    enc.512x512_block0.conv_res1).  tests/test_conv_ops_cpu.py pins this function to the host's own, bit for bit."""
    import numpy as np
    w = w.to(torch.float32)
    norm = torch.linalg.vector_norm(w, dim=None, keepdim=True)
    norm = torch.add(1e-4, norm, alpha=np.sqrt(norm.numel() / w.numel()))
    w = w / norm
    return w * (gain / np.sqrt(w[0].numel()))      # gain: the int 1, or the fp32 tensor out_gain (then an fp32 division), as the host passes them


# ------------------------------------------------------------------------------------------------ the plan
class _Graph:
    """the op list under construction: what `describe` (the U-Net) and `describe_ae` (the autoencoder's two stacks) have in common.  One op is a dict
    label / segs / cout / shift / epi / cvec_off / res / clip / out_f32 / sumsq / K; one K-segment a dict src / C / taps / resample / xform / wname / gain (name
    of the scalar parameter folded into the weight, or None) / cin_tot / cin_off / scale64 / scale32 / mul64 / mul32."""

    def __init__(self, modulated):
        self.ops, self.modulated, self.coff = [], modulated, 0

    @staticmethod
    def seg(src, C, taps, rs, xf, wname, cin_tot, cin_off, scale=(1.0, 1.0), mul=(1.0, 1.0), gain=None):
        return dict(src=src, C=C, taps=taps, resample=rs, xform=xf, wname=wname, gain=gain, cin_tot=cin_tot, cin_off=cin_off, scale64=scale[0], scale32=scale[1],
                    mul64=mul[0], mul32=mul[1])

    def op(self, label, segs, cout, shift, epi="plain", cvec_off=-1, res=None, clip=0.0, out_f32=False, sumsq=False):
        self.ops.append(dict(label=label, segs=segs, cout=cout, shift=shift, epi=epi, cvec_off=cvec_off, res=res, clip=clip, out_f32=out_f32, sumsq=sumsq,
                             K=sum(s["C"] * s["taps"] for s in segs)))
        return label

    def cvec_off(self, b):
        """a modulated block (the U-Net) owns `cout` columns of @cvec; the autoencoder's blocks all read the one row of ones from its start"""
        if not self.modulated:
            return 0
        b["cvec_off"] = self.coff
        self.coff += b["cout"]
        return b["cvec_off"]

    def attn(self, n, o, cout, shift, sumsq):
        seg, op = self.seg, self.op
        op(n + ".attn_qkv", [seg(o, cout, 1, 0, 0, n + ".attn_qkv.weight", cout, 0)], 3 * cout, shift)
        return op(n + ".attn_proj", [seg(n + ".attn", cout, 1, 0, 0, n + ".attn_proj.weight", cout, 0, mul=(KMIX_NEW64, KMIX_NEW32))], cout, shift,
                  epi="res", res=dict(src=o, resample=0, norm=False, C=cout), clip=256.0, sumsq=sumsq)

    def enc_block(self, b, cur, shift, next_norms):
        """-> (output label, shift): the first 3x3 conv, or an encoder block (pixel-normed input, optional 1x1 skip conv in front, normed residual)"""
        seg, op, n = self.seg, self.op, b["name"]
        if b["kind"] == "conv":
            return op(n, [seg(cur, b["cin"], 9, 0, 0, n + ".weight", b["cin"], 0)], b["cout"], shift, sumsq=next_norms), shift
        coff = self.cvec_off(b)
        rs = 1 if b["resample"] == "down" else 0
        shift += rs
        xs = cur
        if b["cin"] != b["cout"]:
            xs = op(n + ".conv_skip", [seg(cur, b["cin"], 1, rs, 0, n + ".conv_skip.weight", b["cin"], 0)], b["cout"], shift, sumsq=True)
            rs = 0
        y1 = op(n + ".conv_res0", [seg(xs, b["cout"], 9, rs, 2, n + ".conv_res0.weight", b["cout"], 0)], b["cout"], shift, epi="emb", cvec_off=coff)
        o = op(n + ".conv_res1", [seg(y1, b["cout"], 9, 0, 0, n + ".conv_res1.weight", b["cout"], 0, mul=(KMIX_NEW64, KMIX_NEW32))], b["cout"], shift, epi="res",
               res=dict(src=xs, resample=rs, norm=True, C=b["cout"]), clip=0.0 if b["attn"] else 256.0, sumsq=next_norms and not b["attn"])
        if b["attn"]:
            o = self.attn(n, o, b["cout"], shift, next_norms)
        return o, shift

    def dec_block(self, b, cur, shift, skip=None, skip_c=0, t=0.5):
        """-> (output label, shift): a decoder block; with `skip` its input is mp_concat([cur, skip]) (the U-Net), without (the autoencoder) `cur` alone, and a
        channel change then rides on conv_res1 as ONE untransformed 1x1 tail with mul = kMixRes * 1"""
        seg, op, n = self.seg, self.op, b["name"]
        coff = self.cvec_off(b)
        rs = 2 if b["resample"] == "up" else 0
        shift -= 1 if rs else 0
        cx = b["cin"] - skip_c
        sa64 = sb64 = sa32 = sb32 = 1.0
        if skip is not None:
            sa64, sb64 = mp_concat_scales(cx, skip_c, t)
            sa32, sb32 = F32(sa64), F32(sb64)
        w0 = n + ".conv_res0.weight"
        s0 = [seg(cur, cx, 9, rs, 1, w0, b["cin"], 0, scale=(sa64, sa32))]
        if skip is not None:
            s0.append(seg(skip, skip_c, 9, 0, 1, w0, b["cin"], cx, scale=(sb64, sb32)))
        y1 = op(n + ".conv_res0", s0, b["cout"], shift, epi="emb", cvec_off=coff)
        s1 = [seg(y1, b["cout"], 9, 0, 0, n + ".conv_res1.weight", b["cout"], 0, mul=(KMIX_NEW64, KMIX_NEW32))]
        res = None
        if b["cin"] != b["cout"]:
            ws = n + ".conv_skip.weight"
            s1.append(seg(cur, cx, 1, rs, 0, ws, b["cin"], 0, mul=(KMIX_RES64 * sa64, _mul32(KMIX_RES32, sa32))))
            if skip is not None:
                s1.append(seg(skip, skip_c, 1, 0, 0, ws, b["cin"], cx, mul=(KMIX_RES64 * sb64, _mul32(KMIX_RES32, sb32))))
        else:
            res = dict(src=cur, resample=rs, norm=False, C=b["cout"])
        o = op(n + ".conv_res1", s1, b["cout"], shift, epi="res", res=res, clip=0.0 if b["attn"] else 256.0)
        if b["attn"]:
            o = self.attn(n, o, b["cout"], shift, False)
        return o, shift


def describe(cfg):
    """Every fused conv op the engine emits for `cfg`, in execution order (mirror of csrc/model_graph.h, kind 0; tests/test_ae_conv_ops_cpu.py holds it to that
    graph field for field).  Sizes are relative: `shift` = log2 of the downsampling of the op's map against the network input."""
    plan = build_plan(cfg)
    t = cfg.get("concat_balance", 0.3)
    g = _Graph(modulated=True)
    enc, cur, shift, skips = plan["enc"], "@input", 0, []
    for bi, b in enumerate(enc):
        cur, shift = g.enc_block(b, cur, shift, bi + 1 < len(enc) and enc[bi + 1]["cin"] == enc[bi + 1]["cout"])
        skips.append((cur, b["cout"]))
    for b in plan["dec"]:
        skip, skip_c = skips.pop() if b.get("concat") else (None, 0)
        cur, shift = g.dec_block(b, cur, shift, skip, skip_c, t)
    g.op("out_conv", [g.seg(cur, plan["final_c"], 9, 0, 0, "out_conv.weight", plan["final_c"], 0, gain="out_gain")], cfg.get("out_channels") or cfg["in_channels"], shift,
         out_f32=True)
    return g.ops, g.coff


def describe_ae(cfg, kind):
    """The same for one stack of the EDMAutoencoder (kind 1: the encoder alone, out_conv on the bottleneck; kind 2: the skip-less decoder behind the 1x1
    decoder_conv), from tests/_ae_twin.py's `ae_plan`.  -> (ops, width of the row of ones every modulated epilogue reads: the stack's largest cout, at least 64).
    What no U-Net plan has: `decoder_conv` (one tap, latent + direct + ones channels straight from the staged input); a channel-changing decoder block's
    conv_res1 with a SINGLE tail (mul = kMixRes, no concat scale); `encoder.out_conv` (2 * latent_channels fp32 couts at the deepest level); `shift` < 0 (the
    decoder's maps grow from the latent); cvec_off = 0 everywhere."""
    import _ae_twin
    plan = _ae_twin.ae_plan(cfg)
    L, D = cfg["latent_channels"], len(cfg.get("direct_skips") or [])
    g = _Graph(modulated=False)
    cur, shift = "@input", 0
    if kind == 1:
        enc = plan["enc"]
        for bi, b in enumerate(enc):
            cur, shift = g.enc_block(b, cur, shift, bi + 1 < len(enc) and enc[bi + 1]["cin"] == enc[bi + 1]["cout"])
        g.op("encoder.out_conv", [g.seg(cur, plan["enc_c"], 9, 0, 0, "encoder.out_conv.weight", plan["enc_c"], 0, gain="encoder.out_gain")], 2 * L, shift, out_f32=True)
        blocks = [b for b in enc if b["kind"] == "block"]
    else:
        assert kind == 2
        cur = g.op("decoder_conv", [g.seg(cur, L + D + 1, 1, 0, 0, "decoder_conv.weight", L + D + 1, 0)], plan["dec_c0"], shift)
        for b in plan["dec"]:
            cur, shift = g.dec_block(b, cur, shift)
        g.op("out_conv", [g.seg(cur, plan["final_c"], 9, 0, 0, "out_conv.weight", plan["final_c"], 0, gain="out_gain")], cfg.get("out_channels") or cfg["in_channels"], shift,
             out_f32=True)
        blocks = plan["dec"]
    return g.ops, max([64] + [b["cout"] for b in blocks])


def gains_of(ops):
    """{weight name: name of the scalar gain folded into it} of an op list"""
    return {s["wname"]: s["gain"] for o in ops for s in o["segs"] if s["gain"]}


def level_dim(v, shift):
    """a map side `shift` halvings (negative: doublings) from the stack's input, with build_plan's arithmetic"""
    for _ in range(max(shift, 0)):
        v = (v + 1) // 2
    return v << max(-shift, 0)


def _resample(x, rs):
    if rs == 1:
        return x[:, :, ::2, ::2]
    if rs == 2:
        return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    return x


def _conv(a, w):
    """sum over taps of 1x1 products (zero padding 1 for 3x3): nothing but slices and matmuls, in a's dtype, on a's device"""
    k = w.shape[-1]
    if k == 1:
        return torch.einsum("oc,nchw->nohw", w[:, :, 0, 0], a)
    h, wd = a.shape[2:]
    ap = F.pad(a, (1, 1, 1, 1))
    out = None
    for ky in range(3):
        for kx in range(3):
            o = torch.einsum("oc,nchw->nohw", w[:, :, ky, kx], ap[:, :, ky:ky + h, kx:kx + wd])
            out = o if out is None else out + o
    return out


KSTEP = {"bf16": 16, "fp16": 16, "fp32": 4}      # products per accumulate step of the MFMA the kernels use (32x32x16 / 16x16x32 16-bit, 16x16x4 fp32)


def acc_steps(o, T):
    """accumulate steps of one output element: per tap, the real channels of a K-segment in groups of KSTEP.  K / KSTEP where the channel counts are multiples of
    the group (every block conv); more where a few real channels sit in a padded chunk -- the 3x3 input conv of 2 + 1 channels adds 9 partial sums, not 27 / 16 --
    and the all-zero groups of the padding add nothing and round nothing"""
    return sum(s["taps"] * ((s["C"] + KSTEP[T] - 1) // KSTEP[T]) for s in o["segs"])


def _conv_steps32(a, w, step):
    """the emulation's K sum: like the matrix core, `step` products at a time are summed (here in float64) and each such partial sum is added to an fp32
    accumulator, one rounding per step, taps and channel groups in sequence"""
    n, C, h, wd = a.shape
    k = w.shape[-1]
    ap = F.pad(a, (1, 1, 1, 1)) if k == 3 else a
    G = (C + step - 1) // step
    pad = G * step - C
    acc = torch.zeros((n, w.shape[0], h, wd), dtype=torch.float32)
    for ky in range(k):
        for kx in range(k):
            at = ap[:, :, ky:ky + h, kx:kx + wd].double()
            wt = w[:, :, ky, kx].double()
            if pad:
                at, wt = F.pad(at, (0, 0, 0, 0, 0, pad)), F.pad(wt, (0, pad))
            parts = torch.einsum("ogc,ngchw->gnohw", wt.reshape(-1, G, step), at.reshape(n, G, step, h, wd)).to(torch.float32)
            for g in range(G):
                acc = acc + parts[g]
    return acc


def _sig(z):
    return torch.sigmoid(z)


def _silu64(z):
    return z * torch.sigmoid(z) / 0.596


def _silu_k32(x, s32):
    """the kernels' 16-bit-mode form in fp32: (x * k2) * rcp(1 + exp2(x * k1)), k1 = -s log2(e), k2 = s / 0.596 (conv_common.h silu_k / silu_k1); s a tensor or a float"""
    s = torch.as_tensor(s32, dtype=torch.float32, device=x.device)
    k1 = s * torch.tensor(-1.4426950408889634, dtype=torch.float32)
    k2 = s * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(0.596, dtype=torch.float32))
    return (x * k2) * torch.reciprocal(1.0 + torch.exp2(x * k1))


def _silu_f32(z):
    """the fp32-mode form: z / (1 + expf(-z)) * (1 / 0.596f)"""
    return z / (1.0 + torch.exp(-z)) * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(0.596, dtype=torch.float32))


Z_MIN, F_MIN = -1.2784645427610738, -0.27846454276107374 / 0.596      # the minimum of mp_silu


def _through_silu(z, d, fz):
    """sup of |mp_silu(z') - mp_silu(z)| over |z' - z| <= d: the two ends, and the minimum of the function where the interval holds it"""
    e = torch.maximum((_silu64(z + d) - fz).abs(), (_silu64(z - d) - fz).abs())
    inside = (z - d < Z_MIN) & (z + d > Z_MIN)
    return torch.maximum(e, torch.where(inside, (F_MIN - fz).abs(), torch.zeros_like(e)))


def attention64(qkv):
    """OracleUnet._attn between the two 1x1 convs, float64, from a stored attn_qkv output (n, 3C, h, w)"""
    from oracle.unet import normalize
    n, c3, h, w = qkv.shape
    heads = c3 // 3 // 64
    y = qkv.double().reshape(n, heads, -1, 3, h * w)
    q, k, v = normalize(y, dim=2).unbind(3)
    wts = torch.einsum("nhcq,nhck->nhqk", q, k / math.sqrt(q.shape[2])).softmax(dim=3)
    return torch.einsum("nhqk,nhck->nhcq", wts, v).reshape(n, c3 // 3, h, w)


# ------------------------------------------------------------------------------------------------ the op model
class Twin:
    """mode 'exact': float64 everywhere, exact mul factors, no rounding (the chain test against OracleUnet);
    mode 'bf16' / 'fp16' / 'fp32': the engine's operands and weights in that storage type, evaluated in float64."""

    def __init__(self, cfg, sd, mode, device="cpu", ops=None, gains=None, c_total=None):
        """ops / gains / c_total: an op list in `describe`'s form, its {weight name: gain name} map and the width of a modulation row (default: the U-Net's,
        `describe(cfg)`; for a stack of the autoencoder `describe_ae(cfg, kind)`, `gains_of(ops)` and the width of its row of ones)"""
        self.cfg, self.mode, self.dev = cfg, mode, torch.device(device)
        if ops is None:
            ops, c_total = describe(cfg)
        self.ops, self.c_total = ops, c_total
        self.gains = gains_of(ops) if gains is None else dict(gains)
        self.by_label = {o["label"]: o for o in self.ops}
        self.folded = {}
        for o in self.ops:
            for s in o["segs"]:
                if s["wname"] not in self.folded:
                    gn = self.gains.get(s["wname"])
                    # 'exact' follows the float64 reference networks (OracleUnet, AETwin: the chain tests' references) to the last bit, the storage-type modes follow
                    # the host that feeds the engine (the gain an fp32 tensor, as `load_state_dict` passes it)
                    self.folded[s["wname"]] = fold_weight(torch.as_tensor(sd[s["wname"]]), float(sd[gn]) if gn else 1.0) if mode == "exact" else \
                        fold_host(torch.as_tensor(sd[s["wname"]]), torch.as_tensor(sd[gn]).to(torch.float32) if gn else 1)
        self._wcache = {}

    def weight(self, o, i, dtype=torch.float64):
        key = (o["label"], i, dtype)
        if key not in self._wcache:
            s = o["segs"][i]
            w = self.folded[s["wname"]][:, s["cin_off"]:s["cin_off"] + s["C"]]
            if self.mode == "exact":
                w = w.double() * s["mul64"]
            else:
                w = rne(w * torch.tensor(s["mul32"], dtype=torch.float32), self.mode)
            self._wcache = {k: v for k, v in self._wcache.items() if k[0] == o["label"]}   # one op's weights at a time
            self._wcache[key] = w.to(self.dev, dtype)
        return self._wcache[key]

    def _rn64(self, x):
        return 1.0 / (1e-4 + torch.sqrt((x * x).mean(dim=1, keepdim=True)))

    def _rn(self, x, planes):
        """(rn, allowance in u): pixel_rn of conv_common.h.  With the producer's sum-of-squares planes (what the kernel itself reads; `check_sumsq` holds them to
        the stored tensor) it is the kernel's own fp32 arithmetic, planes added in ascending order; without them float64 from the stored tensor"""
        if self.mode == "exact" or planes is None:
            return self._rn64(x), E_RN(x.shape[1])
        e_rn = E_RN_PLANES
        if isinstance(planes, tuple):
            # producer on the 64 px x 16 cout flavour: one plane per 16 couts, of which read_activation returns the first half.  The others are restated
            # from the stored tensor in fp32 (another order inside the 16: a few u of that plane, E_RN_F5 in all); the ascending sum over the planes is the kernel's
            planes, e_rn = planes[0], E_RN_F5
            x32 = x.to(torch.float32)
            rest = [(x32[:, 16 * g:16 * g + 16] ** 2).sum(1) for g in range(planes.shape[0], (x.shape[1] + 15) // 16)]
            planes = torch.cat([planes.to(torch.float32), torch.stack(rest)], 0) if rest else planes
        t = planes[0].to(torch.float32)
        for q in range(1, planes.shape[0]):
            t = t + planes[q].to(torch.float32)
        rn = 1.0 / (torch.tensor(1e-4, dtype=torch.float32) + torch.sqrt(t * torch.tensor(1.0 / x.shape[1], dtype=torch.float32)))
        return rn[:, None].double(), e_rn

    def operand(self, s, x, planes=None):
        """(a, u): the operand tensor of one K-segment from its stored source x (float64, already the wanted batch samples), and the bound on what the
        kernel's own evaluation may add to |a| (None where it cannot differ)"""
        T = self.mode
        x = x[:, :s["C"]]
        if s["xform"] == 0:
            return _resample(x, s["resample"]), None
        if s["xform"] == 1:
            sc, e_rn = (s["scale64"] if T == "exact" else s["scale32"]), 0.0
        else:
            sc, e_rn = self._rn(x, planes)
        z = _resample(sc * x, s["resample"])
        if T == "exact":
            return _silu64(z), None
        # the kernels' own fp32 form of the activation (the multiplies and the add are IEEE and reproduce; exp2 / rcp may differ by C_PRO u in all)
        xr = _resample(x, s["resample"]).to(torch.float32)
        sr = _resample(sc, s["resample"]).to(torch.float32) if torch.is_tensor(sc) else sc
        a = (_silu_f32(xr * sr) if T == "fp32" else _silu_k32(xr, sr)).double()
        amp = 1.0 + z.abs() * LOG2E * _sig(-z)                 # |t| sig(t), t = -z log2(e): what an error of the scale is amplified by
        d = U * a.abs() * (C_PRO + e_rn * amp)
        if T == "fp32":
            return a, d
        ul = ulp(a, T)
        fr = a / ul
        near = ((fr - torch.floor(fr) - 0.5).abs() * ul <= d)
        return rne(a, T), torch.where(near, ul, torch.zeros_like(ul))

    def eval(self, o, src, cvec=None):
        """src(label) -> stored tensor (float64, the wanted batch samples, on self.dev); cvec: (n, c_total) of the same samples.
        Returns dict(ref, s, K, E_acc, E_epi, E_pro)."""
        T = self.mode
        v = s2 = ep = None
        for i, sg in enumerate(o["segs"]):
            x = src(sg["src"])
            a, u = self.operand(sg, x, src("sumsq:" + sg["src"]) if sg["xform"] == 2 else None)
            w = self.weight(o, i)
            t_ = _conv(a, w)
            v = t_ if v is None else v + t_
            if T != "exact":
                q = _conv(a * a, w * w)
                s2 = q if s2 is None else s2 + q
                if u is not None:
                    e = _conv(u, w.abs())
                    ep = e if ep is None else ep + e
        zero = torch.zeros_like(v)
        gain, e_epi = 1.0, zero
        if o["epi"] == "emb":
            c = cvec[:, o["cvec_off"]:o["cvec_off"] + o["cout"]].double()[:, :, None, None]
            z = v * c
            ref = _silu64(z)
            sg_ = _sig(z)
            gain = (c * sg_ * (1.0 + z * (1.0 - sg_))).abs() / 0.596
            fprop = lambda ev: _through_silu(z, c.abs() * ev, ref)     # what an error ev of the K sum becomes at the output (not linearised)
            e_epi = C_EPI * U * ref.abs() * (1.0 + z.abs() * LOG2E * _sig(-z))
        elif o["epi"] == "res":
            ref = v
            if o["res"] is not None:
                r = src(o["res"]["src"])[:, :o["res"]["C"]]
                k = KMIX_RES64 if T == "exact" else KMIX_RES32
                rn, e_rn = self._rn(r, src("sumsq:" + o["res"]["src"])) if o["res"]["norm"] else (1.0, 0.0)
                term = _resample(k * rn * r, o["res"]["resample"])
                ref = v + term
                e_epi = U * (C_EPI * (v.abs() + term.abs()) + e_rn * term.abs())
            if o["clip"] > 0:
                ref = ref.clamp(-o["clip"], o["clip"])
        else:
            ref = v
        out = dict(ref=ref, K=o["K"])
        if T != "exact":
            s = gain * torch.sqrt(s2)
            ea = (C_ACC32 if T == "fp32" else C_ACC) * U * math.sqrt(acc_steps(o, T)) * torch.sqrt(s2 + v * v)
            ep = zero if ep is None else ep
            if o["epi"] == "emb":
                tot = fprop(ea + ep)
                ea, ep = tot * ea / (ea + ep).clamp_min(1e-300), tot * ep / (ea + ep).clamp_min(1e-300)
            out.update(s=s, E_acc=ea, E_epi=e_epi, E_pro=ep)
        return out

    # ---- float32 emulation of the same op, with the kernels' roundings (the CPU stand-in the constants are measured on)
    def emulate(self, o, src, cvec, ratios, hook=None):
        """hook (tests only: deliberately broken kernels): {'v': f(v, operands, weights) -> v, 'c': f(c) -> c, 'no_rn': bool, 'out': f(out) -> out}"""
        T = self.mode
        f32 = torch.float32
        hook = hook or {}
        v = v64 = s2 = None
        A, Wt = [], []
        for i, sg in enumerate(o["segs"]):
            x = src(sg["src"])
            x = x[:, :sg["C"]]
            x32 = x.to(f32)
            if sg["xform"] == 0:
                a = _resample(x32, sg["resample"])
            else:
                if sg["xform"] == 1:
                    sc32, sc64 = sg["scale32"], sg["scale32"]
                else:
                    ss = (x32 * x32).sum(dim=1, keepdim=True)
                    ratios["ss"] = max(ratios.get("ss", 0.0), float(((ss.double() - (x * x).sum(1, keepdim=True)).abs() / (U * math.sqrt(sg["C"]) * ss.double())).max()))
                    sc32 = 1.0 / (1e-4 + torch.sqrt(ss * torch.tensor(1.0 / sg["C"], dtype=f32)))
                    sc64 = self._rn64(x)
                xr, z = _resample(x32, sg["resample"]), _resample(sc64 * x, sg["resample"])
                a = _silu_f32(xr * _resample(sc32, sg["resample"]) if torch.is_tensor(sc32) else xr * sc32) if T == "fp32" else \
                    _silu_k32(xr, _resample(sc32, sg["resample"]) if torch.is_tensor(sc32) else sc32)
                a64 = _silu64(z)
                den = U * a64.abs() * (1.0 + z.abs() * LOG2E * _sig(-z))
                m = den > 1e-30
                r = float(((a.double() - a64).abs()[m] / den[m]).max())
                ratios["pro%d" % sg["xform"]] = max(ratios.get("pro%d" % sg["xform"], 0.0), r)
                a = rne(a, T)
            w = self.weight(o, i)
            A.append(a); Wt.append(w.to(f32))
            t_ = _conv_steps32(a, w.to(f32), KSTEP[T])
            v = t_ if v is None else v + t_
            t64 = _conv(a.double(), w)
            v64 = t64 if v64 is None else v64 + t64
            q = _conv(a.double() ** 2, w * w)
            s2 = q if s2 is None else s2 + q
        key = "acc32" if T == "fp32" else "acc"
        ratios[key] = max(ratios.get(key, 0.0), float(((v.double() - v64).abs() / (U * math.sqrt(acc_steps(o, T)) * torch.sqrt(s2 + v64 * v64)).clamp_min(1e-300)).max()))
        ratios[key + "_s_alone"] = max(ratios.get(key + "_s_alone", 0.0), float(((v.double() - v64).abs() / (U * math.sqrt(acc_steps(o, T)) * torch.sqrt(s2)).clamp_min(1e-300)).max()))
        if "v" in hook:
            v = hook["v"](v, A, Wt)
        if o["epi"] == "emb":
            c = cvec[:, o["cvec_off"]:o["cvec_off"] + o["cout"]].to(f32)
            c = (hook["c"](c) if "c" in hook else c)[:, :, None, None]
            out = _silu_f32(v * c) if T == "fp32" else _silu_k32(v * c, 1.0)
            z = v.double() * c.double()
            e64 = _silu64(z)
            ratios["epi_emb"] = max(ratios.get("epi_emb", 0.0), float(((out.double() - e64).abs() / (U * e64.abs() * (1.0 + z.abs() * LOG2E * _sig(-z))).clamp_min(1e-300)).max()))
        elif o["epi"] == "res":
            out = v
            if o["res"] is not None:
                r = src(o["res"]["src"])[:, :o["res"]["C"]]
                r32 = r.to(f32)
                sc = torch.tensor(KMIX_RES32, dtype=f32)
                sc64 = KMIX_RES32
                if o["res"]["norm"] and not hook.get("no_rn"):
                    ss = (r32 * r32).sum(dim=1, keepdim=True)
                    sc = sc * (1.0 / (1e-4 + torch.sqrt(ss * torch.tensor(1.0 / o["res"]["C"], dtype=f32))))
                    sc64 = KMIX_RES32 * self._rn64(r)
                out = v + _resample(sc * r32, o["res"]["resample"])
                term = _resample(sc64 * r, o["res"]["resample"])
                den = U * (v.double().abs() + term.abs() + (E_RN(o["res"]["C"]) / C_EPI if o["res"]["norm"] else 0.0) * term.abs())
                ratios["epi_res"] = max(ratios.get("epi_res", 0.0), float(((out.double() - (v.double() + term)).abs() / den.clamp_min(1e-300)).max()))
            if o["clip"] > 0:
                out = out.clamp(-o["clip"], o["clip"])
        else:
            out = v
        out = out.double() if (o["out_f32"] or T == "fp32") else rne(out, T).double()
        return hook["out"](out) if "out" in hook else out


def run_chain(tw, x, cvec, emulate=False, ratios=None, on_op=None, hooks=None):
    """every op of the network in order, each fed the chain's own earlier outputs.  mode 'exact': the float64 network (-> stored[label] = ref).
    emulate: the float32 emulation with the kernels' roundings (stored = what the kernel would have stored); hooks: {op label: `Twin.emulate`'s hook} (tests only)."""
    T = tw.mode
    ones = torch.ones_like(x[:, :1])
    xin = torch.cat([x, ones], 1).double()      # (the autoencoder's stacks stage their input the same way: image / latent channels, then the ones channel)
    stored = {"@input": xin if T == "exact" else rne(xin, T)}
    src = lambda lab: stored.get(lab) if lab.startswith("sumsq:") else stored[lab]
    for o in tw.ops:
        if emulate:
            out = stored[o["label"]] = tw.emulate(o, src, cvec, ratios, hook=(hooks or {}).get(o["label"]))
            if o["sumsq"]:   # one plane, fp32
                stored["sumsq:" + o["label"]] = (out.to(torch.float32) ** 2).sum(1)[None]
        else:
            stored[o["label"]] = tw.eval(o, src, cvec)["ref"]
        if o["label"].endswith(".attn_qkv"):   # the attention op (no conv): its float64 formula; the emulation stores it in the storage type as the engine does
            a = attention64(stored[o["label"]])
            stored[o["label"][:-4]] = rne(a, T) if emulate and T != "fp32" else a
        if on_op:
            on_op(o, src)
    return stored


def oracle_cvec(cfg, sd, t, cond, dtype=torch.float64):
    """(n, c_total) modulation rows in the engine's @cvec layout (blocks in execution order), from OracleUnet's own embedding arithmetic"""
    orc = OracleUnet(cfg, sd, dtype=dtype)
    emb = orc.embeddings(t, cond)
    rows = []
    for b in orc.plan["enc"] + orc.plan["dec"]:
        if b["kind"] == "conv":
            continue
        c = F.linear(emb, orc.w[b["name"] + ".emb_linear"]) + 1
        rows.append(c / torch.sqrt(torch.mean(c ** 2, dim=1, keepdim=True) + 1e-8))
    return torch.cat(rows, 1)


# ------------------------------------------------------------------------------------------------ the criterion
def flavour_of(profile_label):
    """'enc.64x64_conv [64x64 k1 f2w bn96 wg.. ks1 ...]' -> ('enc.64x64_conv', 'f2w', 1); the per-tap flavour's tag is 'f0'"""
    m = re.search(r"^(.*) \[.* (f\d\w*) bn\d+ wg\d+ ks(\d+) ", profile_label)
    return m.group(1), m.group(2), int(m.group(3))


def check_op(o, r, hip, T, flavour="?", samples=None, stats=None):
    """Every element of `hip` (the stored output, float64, same samples as r) against r = Twin.eval(...).  Raises AssertionError naming the op, the
    flavour, the worst element, its error in ulps, the number of failing elements and their bounding box; returns the op's statistics."""
    ref = r["ref"]
    assert hip.shape == ref.shape, (o["label"], tuple(hip.shape), tuple(ref.shape))
    sixteen = T != "fp32" and not o["out_f32"]
    E = r["E_acc"] + r["E_epi"] + r["E_pro"]
    ul = ulp(ref, T) if sixteen else None
    # RNE moves the value it rounds -- which lies within E of ref -- by at most half an ulp of ITS binade: where |ref| + E crosses a power of two that is the
    # larger binade's (one element in 10^9 on the MI355X: a flagged operand flip had carried -0.00711 over 2^-7)
    half = 0.5 * ulp(ref.abs() + E, T) if sixteen else torch.zeros_like(ref)
    err = (hip - ref).abs()
    bad = ~(err <= half + E)            # (a NaN fails)
    excess = (err - half) / E.clamp_min(1e-300)
    st = dict(label=o["label"], flavour=flavour, elements=ref.numel(), worst=float(excess.max()), median=0.0,
              rounded_off=float((hip != rne(ref, T)).double().mean()) if sixteen else float("nan"))
    if sixteen:
        keep = ref.abs() >= 2.0 ** -6 * ref.pow(2).mean().sqrt()
        st["median"] = float((E / (0.5 * ul))[keep].median()) if bool(keep.any()) else 0.0
    if stats is not None:
        stats.append(st)
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()
        worst = torch.where(bad, err / (ul if sixteen else E.clamp_min(1e-300)), torch.zeros_like(err))
        wi = [int(v) for v in torch.unravel_index(worst.argmax(), worst.shape)] if hasattr(torch, "unravel_index") else [int(v) for v in idx[0]]
        n_ = samples[wi[0]] if samples is not None else wi[0]
        lo, hi = idx[:, 1:].min(0).values.tolist(), idx[:, 1:].max(0).values.tolist()
        raise AssertionError(
            f"{o['label']} [{flavour}, {T}]: {nbad} of {ref.numel()} elements outside half-ulp + E; worst at (n, c, y, x) = ({n_}, {wi[1]}, {wi[2]}, {wi[3]}): "
            f"hip {float(hip[tuple(wi)]):.9g} ref {float(ref[tuple(wi)]):.9g}, error {float(worst[tuple(wi)]):.2f} {'ulp' if sixteen else 'x E'} "
            f"(allowed {float(((half + E) / (ul if sixteen else E.clamp_min(1e-300)))[tuple(wi)]):.3f}); failing elements span c {lo[0]}..{hi[0]}, y {lo[1]}..{hi[1]}, x {lo[2]}..{hi[2]}"
            f" in samples {sorted(set((samples[i] if samples is not None else i) for i in idx[:, 0].unique().tolist()))}")
    if sixteen:
        assert st["median"] <= MEDIAN_MAX, f"{o['label']} [{flavour}, {T}]: median E / half-ulp = {st['median']:.3f} > {MEDIAN_MAX}: the slack is too loose to see a rounding-sized error"
    return st


def check_sumsq(o, planes, stored, T, flavour="?", samples=None):
    """sum over the planes' first axis against float64 sum_c stored^2, per pixel, relative.  `planes`: (parts, n, h, w); the 64 px x 16 cout flavour keeps one
    plane per 16 couts and read_activation returns the first cout_pad / 32 of them: those cover the first half of the (padded) couts."""
    C = stored.shape[1]
    if flavour.startswith("f5"):
        C = min(C, planes.shape[0] * 16)
    tot = planes.double().sum(0)
    ref = (stored[:, :C] ** 2).sum(1)
    tol = U * min(float(C), C_SS * math.sqrt(C)) * ref + 1e-30
    bad = ~((tot - ref).abs() <= tol)
    if bool(bad.any()):
        idx = bad.nonzero()
        w = ((tot - ref).abs() / tol)
        wi = [int(v) for v in idx[w[bad].argmax()]]
        raise AssertionError(f"sumsq:{o['label']} [{flavour}, {T}]: {int(bad.sum())} of {ref.numel()} pixels off; worst at (n, y, x) = "
                             f"({samples[wi[0]] if samples is not None else wi[0]}, {wi[1]}, {wi[2]}): planes {float(tot[tuple(wi)]):.9g} stored {float(ref[tuple(wi)]):.9g} "
                             f"({float(w[tuple(wi)]):.2f} x the bound); span y {int(idx[:, 1].min())}..{int(idx[:, 1].max())}, x {int(idx[:, 2].min())}..{int(idx[:, 2].max())}")
    return float(((tot - ref).abs() / tol).max())


def pick_samples(n):
    """first image, every slot of an image group of 4 (the narrow 8x8 tiles pack 2 or 4 images), one in the middle, the last image"""
    return sorted(set(i for i in (0, 1, 2, 3, n // 2 + 1, n - 2, n - 1) if 0 <= i < n))[:7] if n > 6 else list(range(n))


def ones_cvec(n, width, dtype=torch.float32):
    """the modulation rows of an autoencoder stack: `td_unet::d_ones`, one shared row of ones"""
    return torch.ones((n, width), dtype=dtype)


def check_forward(model, tw, x, t, cond, T, flavours, device="cuda", samples=None, attn_mfma=True, attn_stats=None, cvec=None, stored_input=False):
    """All conv ops of one engine forward (already run on `model` with x) against the twin.  flavours: {label: (tag, ksplit)} from the profile labels.
    Every attention op on the way is held to tests/_attn_twin.py's criterion on its own stored input (attn_mfma: whether the plan runs bf16 attention on the MFMA
    kernel; its statistics are appended to attn_stats).  Returns (list of per-op statistics, number of sum-of-squares planes checked).
    A stack of the autoencoder (`model`: anything with EDMUnet2D's `read_activation(n, H, W, label, max_elems=)`, `ae_stack` below): cvec = the (n, width) rows of ones
    it reads in place of @cvec, and stored_input = True: the `@input` source is the staged `@xin` the engine stored (x then only gives n, H, W)."""
    n, _, H, W = x.shape
    samples = samples or pick_samples(n)
    dev = torch.device(device)
    sel = torch.tensor(samples)
    cache = {}

    def src(label):
        if label.startswith("sumsq:"):
            lab = label[6:]
            # (the 64 px x 16 cout flavour keeps twice the planes read_activation returns: rn then comes from the stored tensor in float64)
            if lab not in tw.by_label or not tw.by_label[lab]["sumsq"]:
                return None
            if label not in cache:
                cache[label] = model.read_activation(n, H, W, label, max_elems=size(lab, planes=True))[:, sel].to(dev)
            return (cache[label], "f5") if flavours.get(lab, ("?", 1))[0].startswith("f5") else cache[label]
        if label not in cache:
            if label == "@input" and stored_input:
                cache[label] = model.read_activation(n, H, W, "@xin", max_elems=n * H * W * 64)[sel].double().to(dev)
            elif label == "@input":
                xi = x[sel].double().cpu()
                cache[label] = rne(torch.cat([xi, torch.ones_like(xi[:, :1])], 1), T).to(dev)
            else:
                try:
                    cache[label] = model.read_activation(n, H, W, label, max_elems=size(label))[sel].double().to(dev)
                except Exception as e:
                    raise RuntimeError(f"reading {label} ({size(label)} elements expected): {e}") from e
        return cache[label]

    def size(label, planes=False):
        o_ = tw.by_label[label + "_proj" if label.endswith(".attn") else label]      # (the attention output has the geometry of the conv that reads it)
        px = n * level_dim(H, o_["shift"]) * level_dim(W, o_["shift"])
        return px * ((o_["cout"] + 63) // 64 * 4 + 2) if planes else px * o_["cout"]

    cvec = (model.read_activation(n, H, W, "@cvec").reshape(n, -1) if cvec is None else cvec)[sel].to(dev)
    stats, nss = [], 0
    last_use = {}
    for o in tw.ops:
        for lab in [s["src"] for s in o["segs"]] + ([o["res"]["src"]] if o["res"] else []):
            last_use[lab] = o["label"]
    for o in tw.ops:
        fl = flavours.get(o["label"], ("?", 1))
        tag = fl[0] + (f" ks{fl[1]}" if fl[1] > 1 else "")
        if o["label"].endswith(".attn_proj"):
            import _attn_twin as at
            blk = o["label"][:-10]
            st_ = at.check_engine_attention(src(blk + ".attn_qkv"), src(blk + ".attn"), T, attn_mfma and T == "bf16", f"{blk}.attn [{T}]", dev)
            if attn_stats is not None:
                attn_stats.append(st_)
            cache.pop(blk + ".attn_qkv", None)
        r = tw.eval(o, src, cvec)
        hip = src(o["label"])
        check_op(o, r, hip, T, tag, samples, stats)
        if o["sumsq"]:
            planes = src("sumsq:" + o["label"])
            planes = planes[0] if isinstance(planes, tuple) else planes
            check_sumsq(o, planes, hip, T, tag, samples)
            nss += 1
        for lab in [k for k, v in last_use.items() if v == o["label"]]:
            cache.pop(lab, None); cache.pop("sumsq:" + lab, None)
        if o["label"] not in last_use:
            cache.pop(o["label"], None); cache.pop("sumsq:" + o["label"], None)
    return stats, nss


class ae_stack:
    """one stack of an EDMAutoencoder (1 the encoder, 2 the decoder) with the read-back interface `check_forward` uses"""

    def __init__(self, ae, stack):
        self.ae, self.stack = ae, stack

    def read_activation(self, n, H, W, label, max_elems=1 << 26):
        return self.ae.read_activation(self.stack, n, H, W, label, max_elems=max_elems)


def summary_line(name, stats, nss, wall):
    el = sum(s["elements"] for s in stats)
    ro = [s["rounded_off"] * s["elements"] for s in stats if s["rounded_off"] == s["rounded_off"]]
    el16 = sum(s["elements"] for s in stats if s["rounded_off"] == s["rounded_off"])
    return (f"{name}: {len(stats)} ops, {nss} sumsq totals, {el} elements, worst (|err| - half_ulp) / E = {max(s['worst'] for s in stats):.3f}, "
            f"stored != RNE(ref) on {100.0 * sum(ro) / max(1, el16):.3f} %, max median E/half_ulp {max(s['median'] for s in stats):.3f}, {wall:.1f} s")


if __name__ == "__main__":   # per-op table of one base-model forward on the GPU (what tests/_op_err.py printed for three ops, for all of them)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import terrain_diffusion_amd as td
    from oracle import rng
    from oracle.unet import BASE_CONFIG, synth_state_dict
    T = sys.argv[1] if len(sys.argv) > 1 else "bf16"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    cfg = dict(BASE_CONFIG); sd = synth_state_dict(cfg, seed=1234)
    x = torch.from_numpy(rng.standard_normal(7, (n, 5, 64, 64))); cond = torch.from_numpy(rng.standard_normal(8, (n, 58)))
    m = td.EDMUnet2D(**cfg, dtype=T).load_state_dict(sd)
    m(x.cuda(), torch.full((n,), 1.1), [cond.cuda()])
    t0 = time.time()
    st, nss = check_forward(m, Twin(cfg, sd, T, "cuda"), x, None, None, T, {})
    for s in st:
        print(f"{s['label']:36s} worst {s['worst']:8.3f}  stored != RNE(ref) {100 * s['rounded_off']:7.3f} %  median E/half_ulp {s['median']:.3f}")
    print(summary_line(f"base {T} n={n}", st, nss, time.time() - t0))
