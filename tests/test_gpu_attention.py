"""MFMA attention kernel (VERDICT row N1): parity against the einsum formulation of UNetBlock.attn (unet_block.py:102-108) on the terrain block's
shape and against plain scaled-dot-product attention on SD-v1.5-shaped synthetic cases (annotated_infinite_panorama.py:109-134: head dims
40 / 80 / 160, self-attention up to 4096 x 4096, cross-attention against 77 tokens), ragged lengths included.  Operands are bf16 inside the
kernel (fp32 accumulate): tolerance 1.5e-2 relative RMS against the fp32 reference, 2e-3 against a reference fed bf16-rounded operands."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_rms
from _engine_opts import engine_options_guard, pinned  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu


def _ref(q, k, v, scale, normalize):
    q, k, v = q.double(), k.double(), v.double()
    if normalize:   # mp_layers.normalize over the channel dim: x / (1e-4 + ||x|| / sqrt(D))
        n = lambda x: x / (1e-4 + x.norm(dim=-1, keepdim=True) / math.sqrt(x.shape[-1]))
        q, k, v = n(q), n(k), n(v)
    w = torch.einsum("bhqd,bhkd->bhqk", q, k * scale).softmax(dim=-1)
    return torch.einsum("bhqk,bhkd->bhqd", w, v).float()


CASES = [  # B, H, Lq, Lk, D, normalize
    (3, 4, 64, 64, 64, True),       # terrain block at 8x8 (unet_block.py:102-108), batched over tiles
    (2, 3, 256, 256, 64, True),     # terrain block at 16x16
    (1, 2, 4096, 4096, 40, False),  # SD-v1.5 self-attention, 64x64 latents
    (1, 2, 4096, 77, 40, False),    # SD-v1.5 cross-attention against CLIP tokens
    (1, 2, 1024, 1024, 80, False),
    (2, 2, 256, 256, 160, False),
    (1, 1, 100, 77, 40, False),     # ragged: not multiples of the 128-query / 64-key tiles
    (2, 1, 1, 130, 8, False),
    (1, 2, 129, 65, 96, True),
    # round 6, software-pipelined loop (>= 512 keys, head dims 32 / 64 / 96 / 128): its LEAN form (d <= 64: reference point in the accumulator input, row sum on the
    # matrix pipe) and its plain form; even / odd tile counts, ragged last tile, one query block and several
    (1, 2, 1024, 1024, 64, True),
    (1, 2, 700, 1000, 64, False),
    (1, 2, 520, 513, 32, False),
    (1, 1, 200, 600, 96, False),
    (1, 1, 300, 640, 128, False),
]


@pytest.mark.parametrize("B,H,Lq,Lk,D,norm", CASES)
def test_attention_vs_reference(B, H, Lq, Lk, D, norm):
    from terrain_diffusion_amd.attention import attention
    g = torch.Generator().manual_seed(B * 1000 + Lq + D)
    q, k, v = (torch.randn(B, H, L, D, generator=g) * s for L, s in ((Lq, 1.3), (Lk, 0.9), (Lk, 2.0)))
    scale = 1.0 / math.sqrt(D)
    out = attention(q, k, v, scale=scale, normalize=norm).cpu()
    ref = _ref(q, k, v, scale, norm)
    assert out.shape == ref.shape and torch.isfinite(out).all()
    e32 = rel_rms(out.numpy(), ref.numpy())
    rb = lambda t: t.bfloat16().float()
    if norm:
        n = lambda x: x / (1e-4 + x.norm(dim=-1, keepdim=True) / math.sqrt(D))
        e16 = rel_rms(out.numpy(), _ref(rb(n(q)), rb(n(k)), rb(n(v)), scale, False).numpy())
    else:
        e16 = rel_rms(out.numpy(), _ref(rb(q), rb(k), rb(v), scale, False).numpy())
    print(f"attention B{B} H{H} {Lq}x{Lk} d{D} norm={norm}: rel-RMS {e32:.2e} vs fp32, {e16:.2e} vs bf16-operand reference")
    assert e32 < 1.5e-2 and e16 < 4e-3


@pytest.mark.parametrize("scale", [0.173, 0.31])
def test_attention_arbitrary_scale_long_keys_d40(scale):
    """the kernel folds scale * log2(e) into Q before the bf16 rounding and sums an fp32 denominator against a bf16 numerator;
    a scale that is not a power of two, head dim 40 (zero-padded to 48) and 4096 keys is where a drift in that normalisation would show."""
    from terrain_diffusion_amd.attention import attention
    g = torch.Generator().manual_seed(4040)
    q, k, v = (torch.randn(1, 2, L, 40, generator=g) * s for L, s in ((512, 1.3), (4096, 0.9), (4096, 2.0)))
    out = attention(q, k, v, scale=scale).cpu()
    rb = lambda t: t.bfloat16().float()
    e32 = rel_rms(out.numpy(), _ref(q, k, v, scale, False).numpy())
    e16 = rel_rms(out.numpy(), _ref(rb(q), rb(k), rb(v), scale, False).numpy())
    # the operand the kernel really contracts: Q scaled by scale * log2(e) and THEN rounded to bf16
    f = scale * 1.4426950408889634
    e16s = rel_rms(out.numpy(), _ref(rb(q * f) / f, rb(k), rb(v), scale, False).numpy())
    print(f"attention 512x4096 d40 scale {scale}: rel-RMS {e32:.2e} vs fp32, {e16:.2e} vs bf16-operand reference, {e16s:.2e} vs the reference with Q rounded after scaling")
    # sharper softmax (logit std ~2.3 at scale 0.31) amplifies operand rounding: 6e-3 against plainly rounded operands; against the operands the
    # kernel actually uses (Q rounded after scaling) the usual 4e-3 holds -- the gap between the two is the extra rounding the kernel header states
    assert e32 < 1.5e-2 and e16 < 6e-3 and e16s < 4e-3


@pytest.mark.parametrize("D", [40, 64, 128])
@pytest.mark.parametrize("shift,spread", [(-300.0, 1.0), (250.0, 1.0), (0.0, 40.0)])
def test_attention_folded_reference_point_moves_both_ways(shift, spread, D):
    """(D = 64: the pipelined loop's LEAN form keeps the same kind of reference point -- in the accumulator input of the S MFMAs, corrected one tile late after a move;
    D = 128: the pipelined loop's plain form, for comparison.)  Round 6: at head dims with padding (D % 16 != 0) the softmax's reference point rides in a padding channel of the Q K^T contraction and starts at 0
    (csrc/attn_mfma.hip, attn_fold).  It has to move DOWN when every logit of a query lies far below it (shift -300: exp2 of the raw logits would underflow
    to a zero row sum), UP when they lie far above (shift +250: overflow), and repeatedly when the maxima keep growing along the keys (spread 40: logits of
    increasing magnitude; the in-register Q fragment is rewritten on each move).  Logits are shifted by adding a constant channel pair to q and k."""
    from terrain_diffusion_amd.attention import attention
    g = torch.Generator().manual_seed(606)
    Lq, Lk = 200, 700
    q, k, v = (torch.randn(1, 2, L, D, generator=g) for L in (Lq, Lk, Lk))
    scale = 1.0 / math.sqrt(D)
    # channel 0: q = c, k = shift / (c * scale)  ->  every logit gets +shift (in natural-log units); bf16 rounds c and the quotient, the reference uses the rounded values
    c = 4.0
    q[..., 0] = c
    k[..., 0] = shift / (c * scale)
    k = k * torch.linspace(1.0, spread, Lk).view(1, 1, Lk, 1) if spread != 1.0 else k   # growing key norms: the running maximum keeps moving
    out = attention(q, k, v, scale=scale).cpu()
    assert torch.isfinite(out).all()
    f = scale * 1.4426950408889634
    rb = lambda t: t.bfloat16().float()
    e = rel_rms(out.numpy(), _ref(rb(q * f) / f, rb(k), rb(v), scale, False).numpy())
    print(f"folded softmax, logits shifted by {shift}, key spread {spread}: rel-RMS {e:.2e} vs the reference on the kernel's operands")
    assert e < 6e-3


def test_unet_attention_blocks_use_the_mfma_kernel_and_match():
    """the engine's own attention blocks (bf16 mode) go through the MFMA kernel; option attn_mfma=0 selects the scalar fp32 kernel of round 1:
    the two must agree to bf16 rounding, and 16x16-level attention (256 tokens) -- impossible for the scalar kernel -- runs."""
    import terrain_diffusion_amd as td
    from oracle.unet import OracleUnet, synth_state_dict, tiny_config
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    cfg = tiny_config(64, 1)
    sd = synth_state_dict(cfg, seed=77)
    m = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(sd)
    g = torch.Generator(device="cuda").manual_seed(0)
    x, c, t = torch.randn(4, 5, 64, 64, device="cuda", generator=g), torch.randn(4, 58, device="cuda", generator=g), torch.full((4,), 0.9)
    a = m(x, t, [c])
    with pinned(eng, attn_mfma=0):
        b = m(x, t, [c])
    assert rel_rms(a.cpu().numpy(), b.cpu().numpy()) < 1e-2
    ref = OracleUnet(cfg, sd)(x.cpu(), t, [c.cpu()])
    assert rel_rms(a.cpu().numpy(), ref.detach().numpy()) < 2e-2
    # 128x128 input: the mid block attends over 16x16 = 256 tokens
    cfg2 = tiny_config(64, 1)
    m2 = td.EDMUnet2D(**cfg2, dtype="bf16").load_state_dict(sd)
    x2 = torch.randn(1, 5, 128, 128, device="cuda", generator=g)
    y2 = m2(x2, t[:1], [c[:1]])
    ref2 = OracleUnet(cfg2, sd)(x2.cpu(), t[:1], [c[:1].cpu()])
    assert rel_rms(y2.cpu().numpy(), ref2.detach().numpy()) < 2e-2
    m.close(); m2.close()


@pytest.mark.parametrize("B,H,D,Lq,Lk", [(1, 2, 64, 700, 1000), (1, 2, 40, 520, 4096), (1, 2, 32, 300, 513), (1, 2, 8, 130, 640),
                                         (2, 8, 64, 4096, 1024), (2, 8, 40, 4096, 640)])   # the last two: 256 workgroups of 8 waves (the SD shapes' form)
def test_pipelined_loop_is_bit_identical_to_the_unpipelined_one(B, H, D, Lq, Lk, tmp_path):
    """Round 6: the software-pipelined tile loop (csrc/attn_mfma.hip, PIPE: >= 512 keys, head dims <= 64) issues the same MFMAs with the same operands in the same
    order as the unpipelined loop -- plain (D % 16 == 0) and folded (D % 16 != 0) softmax forms, ragged last tile, odd and even tile counts.  The launcher reads its
    A/B hook TD_ATTN_PIPE once per process, so each side runs in its own process; the outputs must be EQUAL, not close."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, torch\n"
        f"sys.path.insert(0, {root!r})\n"
        "from terrain_diffusion_amd.attention import attention\n"
        f"g = torch.Generator().manual_seed({D * 7 + Lk})\n"
        f"q, k, v = (torch.randn({B}, {H}, L, {D}, generator=g) * s for L, s in (({Lq}, 1.3), ({Lk}, 0.9), ({Lk}, 2.0)))\n"
        f"out = attention(q, k, v, scale={1.0 / math.sqrt(D)!r}).cpu()\n"
        "assert torch.isfinite(out).all()\n"
        "torch.save(out, sys.argv[1])\n")
    outs = []
    for pipe in ("0", "1"):
        path = str(tmp_path / f"o{pipe}.pt")
        env = dict(os.environ, TD_ATTN_PIPE=pipe)
        r = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(torch.load(path))
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())
