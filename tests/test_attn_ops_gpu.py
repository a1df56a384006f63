"""The attention kernels, element by element, against their float64 twin (tests/_attn_twin.py): the MFMA flash kernel through td_attention at every head dim 1..160 and on
every arm of its dispatcher (4 / 8 waves, pipelined or not, folded or plain softmax form; the arm is asserted from the shape by restating the dispatch rule), the
moving-reference family, the argument checks; and the engine's own attention op (pack + flash kernel + bf16 store, or the scalar kernel) from the stored `attn_qkv`
output to the stored `<block>.attn` output.  Condition A on every element; conditions B and C (rms(z), max(z)) on the random and moving families.  One line per case."""
import math
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_twin as at
from _engine_opts import engine_options_guard, pinned  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu

LINES = []


def dispatch(B, H, Lq, Lk, D):
    """csrc/attn_mfma.hip, attn_mfma(): (waves per workgroup, pipelined loop, folded softmax form) -- with the defaults of its A/B hooks, which no test sets"""
    dp16, fold = at.dp_of(D) // 16, at.fold_of(D)
    big = (Lq + 255) // 256 * H * B >= 256
    nwgs = ((Lq + 255) // 256 if big else (Lq + 127) // 128) * H * B
    pipe = Lk >= 512 and nwgs <= 384 and (fold or dp16 % 2 == 0) and dp16 <= 4
    return (8 if big else 4, pipe, fold)


def run_case(kind, B, H, Lq, Lk, D, normalize=False, arm=None, stat=None):
    from terrain_diffusion_amd.attention import attention
    case = at.make_case(kind, B, H, Lq, Lk, D, seed=D * 7 + Lk + Lq, normalize=normalize)
    Lk = case["k"].shape[2]
    got = dispatch(B, H, Lq, Lk, D)
    if arm is not None:
        assert got == arm, f"{kind} {B}x{H} {Lq}x{Lk} d{D}: the shape runs arm {got}, the test meant {arm}"
    out = attention(case["q"], case["k"], case["v"], scale=case["scale"], normalize=normalize)
    torch.cuda.synchronize()
    ref = at.reference(at.pack_operands(case, "cuda"), D, normalize)
    name = f"{kind} {B}x{H} {Lq}x{Lk} d{D}{' norm' if normalize else ''} [{got[0]} waves{', pipelined' if got[1] else ''}, {'folded' if got[2] else 'plain'}]"
    if kind == "selector":
        at.selector_honesty(case, ref, full=Lq >= min(64, Lk) + 3)
    st = at.check(out.double(), ref, "fp32", name, stat=(kind != "selector") if stat is None else stat)
    LINES.append(at.line(st))
    print(LINES[-1])
    return st


@pytest.mark.parametrize("D0", range(1, 161, 16))
def test_every_head_dim(D0):
    """every head dim 1..160 at one small ragged shape, random + selector: all 20 (Dp / 16, Dm / 32, form) classes, every D % 16 and D % 32 residue, odd D"""
    for D in range(D0, D0 + 16):
        run_case("random", 1, 2, 70, 150, D, arm=(4, False, at.fold_of(D)))
        run_case("selector", 1, 2, 70, 150, D, arm=(4, False, at.fold_of(D)))


# (B, H, Lq, Lk, D, normalize) per arm (waves, pipelined, folded)
ARMS = {
    "4 waves, short keys": [((4, False, True), 1, 2, 70, 150, 40, False), ((4, False, False), 1, 2, 70, 150, 64, True), ((4, False, False), 2, 3, 200, 77, 128, False)],
    "4 waves, pipelined": [((4, True, False), 1, 2, 70, Lk, 64, Lk == 513) for Lk in (512, 513, 575, 576, 577)] +
                          [((4, True, True), 1, 2, 70, Lk, 40, Lk == 576) for Lk in (512, 513, 575, 576, 577)] + [((4, True, False), 1, 2, 130, 640, 32, False), ((4, True, True), 1, 2, 70, 577, 24, False), ((4, True, True), 1, 2, 70, 513, 8, True)],
    "4 waves, long keys, not pipelined": [((4, False, False), 1, 2, 70, 577, 96, False), ((4, False, False), 1, 2, 70, 640, 128, False), ((4, False, True), 1, 2, 70, 513, 72, False),
                                          ((4, False, False), 1, 2, 70, 576, 48, False), ((4, False, False), 25, 8, 130, 577, 64, False), ((4, False, True), 25, 8, 130, 513, 40, False)],     # (the last two: 400 workgroups of 4 waves, more than the pipelined loop takes)
    "8 waves, short keys": [((8, False, False), 4, 64, 70, 150, 64, True), ((8, False, True), 4, 64, 70, 77, 40, False), ((8, False, True), 1, 128, 300, 150, 24, False)],
    "8 waves, pipelined": [((8, True, False), 4, 64, 70, 513, 64, False), ((8, True, False), 4, 64, 70, 576, 64, True), ((8, True, True), 4, 64, 70, 577, 40, False),
                           ((8, True, True), 3, 128, 70, 512, 40, False)],
    "8 waves, long keys, not pipelined": [((8, False, False), 4, 100, 70, 577, 64, False), ((8, False, True), 4, 100, 70, 576, 40, False), ((8, False, False), 4, 64, 70, 600, 96, False),
                                          ((8, False, False), 4, 64, 70, 513, 128, False)],
}


@pytest.mark.parametrize("arm", list(ARMS))
def test_every_dispatch_arm(arm):
    worst = dict(A=0.0, rms=0.0, mx=-9.0)
    for want, B, H, Lq, Lk, D, norm in ARMS[arm]:
        st = run_case("random", B, H, Lq, Lk, D, norm, arm=want)
        worst = dict(A=max(worst["A"], st["worstA"]), rms=max(worst["rms"], st["rms_z"]), mx=max(worst["mx"], st["max_z"] - st["z_max"]))
        if not norm:
            worst["A"] = max(worst["A"], run_case("selector", B, H, Lq, Lk, D, arm=want)["worstA"])
    LINES.append(f"ARM {arm}: worst |err| / bound {worst['A']:.3f}, worst rms(z) {worst['rms']:.3f}, worst max(z) - bound {worst['mx']:+.2f}")
    print(LINES[-1])


@pytest.mark.parametrize("Lq", [1, 31, 32, 33, 255, 256, 257])
def test_query_lengths(Lq):
    for D, norm in ((40, False), (64, True), (64, False)):
        run_case("random", 1, 2, Lq, 150, D, norm)
        if not norm:
            run_case("selector", 1, 2, Lq, 150, D)


@pytest.mark.parametrize("Lk", [1, 63, 64, 65])
def test_key_lengths(Lk):
    for D in (40, 64, 17, 160):
        run_case("random", 1, 2, 70, Lk, D, stat=Lk > 1)     # (one key: the output is V itself, sigma vanishes)
        run_case("selector", 1, 2, 70, Lk, D)


@pytest.mark.parametrize("D", [40, 64])
def test_sd_self_attention_shape(D):
    """4096 x 4096, the SD-v1.5 shape (the float64 twin runs in torch on the device)"""
    run_case("random", 1, 2, 4096, 4096, D, arm=(4, True, at.fold_of(D)))
    run_case("selector", 1, 2, 4096, 4096, D, arm=(4, True, at.fold_of(D)))


@pytest.mark.parametrize("D", [40, 41, 44, 56, 64, 128])
@pytest.mark.parametrize("kind", ["shift-300", "shift+250", "spread40", "late", "early"])
def test_moving_reference(kind, D):
    run_case(kind, 1, 2, 200, 700, D)
    run_case(kind, 1, 2, 70, 330, D)


def test_arguments_are_refused_and_nothing_is_touched():
    from terrain_diffusion_amd._lib import lib
    from terrain_diffusion_amd.engine import get_engine, ptr
    eng = get_engine("cuda")
    q = torch.randn(1, 2, 8, 161, device="cuda")
    out = torch.full((1, 2, 8, 161), 7.0, device="cuda")
    for B, H, Lq, Lk, D in ((1, 2, 8, 8, 0), (1, 2, 8, 8, 161), (1, 2, 0, 8, 40), (1, 2, 8, 0, 40), (0, 2, 8, 8, 40), (1, 0, 8, 8, 40)):
        rc = lib().td_attention(eng._h, ptr(q), ptr(q), ptr(q), B, H, Lq, Lk, D, 0.1, 0, ptr(out))
        assert rc != 0 and lib().td_last_error(), (B, H, Lq, Lk, D)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- the engine's own attention op: stored attn_qkv -> stored <block>.attn
def _engine_arm(which, T, n, H, W, mfma):
    import terrain_diffusion_amd as td
    from oracle import rng
    from oracle.unet import BASE_CONFIG, synth_state_dict, tiny_config
    from terrain_diffusion_amd.engine import get_engine
    import _conv_twin as ct
    cfg, seed = {"base": (dict(BASE_CONFIG), 1234), "tiny_attn": (tiny_config(64, 2, attn_resolutions=[128]), 77), "tiny": (tiny_config(64, 1), 77)}[which]
    sd = synth_state_dict(cfg, seed=seed)
    eng = get_engine("cuda")
    blocks = [o["label"][:-9] for o in ct.describe(cfg)[0] if o["label"].endswith(".attn_qkv")]
    assert blocks
    x = torch.from_numpy(rng.standard_normal(7, (n, cfg["in_channels"], H, W)))
    cond = [torch.from_numpy(rng.standard_normal(8 + i, (n, c[1]))).cuda() for i, c in enumerate(cfg.get("conditional_inputs", []))]
    m = td.EDMUnet2D(**cfg, dtype=T).load_state_dict(sd)
    stats = []
    try:
        with pinned(eng, attn_mfma=1 if mfma else 0):
            m(x.cuda(), torch.full((n,), 1.1), cond)
            torch.cuda.synchronize()
            sel = ct.pick_samples(n)
            for blk in blocks:
                qkv = m.read_activation(n, H, W, blk + ".attn_qkv")[sel]
                att = m.read_activation(n, H, W, blk + ".attn")[sel]
                assert att.shape == (len(sel), qkv.shape[1] // 3) + qkv.shape[2:]
                tokens, heads = qkv.shape[2] * qkv.shape[3], qkv.shape[1] // 192
                name = f"engine {which} {T} n{n} {H}x{W} {blk}.attn ({tokens} tokens, {heads} heads, {'MFMA ' + str(dispatch(n, heads, tokens, tokens, 64)) if mfma and T == 'bf16' else 'scalar kernel'})"
                st = at.check_engine_attention(qkv, att, T, mfma and T == "bf16", name, "cuda")
                stats.append(st)
                LINES.append(at.line(st))
                print(LINES[-1])
    finally:
        m.close()
    return stats


ENGINE_ARMS = {
    "tiny attention bf16 n3 32x32": ("tiny_attn", "bf16", 3, 32, 32, True),
    "tiny attention fp16 n3 32x32": ("tiny_attn", "fp16", 3, 32, 32, True),
    "tiny attention fp32 n3 32x32": ("tiny_attn", "fp32", 3, 32, 32, True),
    "tiny attention bf16 n3 32x32 attn_mfma=0": ("tiny_attn", "bf16", 3, 32, 32, False),
    "base bf16 n64": ("base", "bf16", 64, 64, 64, True),
    "base bf16 n1": ("base", "bf16", 1, 64, 64, True),
    "tiny bf16 n1 128x128 (256 tokens)": ("tiny", "bf16", 1, 128, 128, True),
}


@pytest.mark.parametrize("arm", list(ENGINE_ARMS))
def test_engine_attention_op_elementwise(arm):
    which, T, n, H, W, mfma = ENGINE_ARMS[arm]
    stats = _engine_arm(which, T, n, H, W, mfma)
    if arm == "base bf16 n64":      # 8-wave workgroups holding 64 real queries of 256
        assert all("MFMA (8" in s["name"] for s in stats), [s["name"] for s in stats]
    if arm.startswith("tiny bf16 n1 128x128"):
        assert any("(256 tokens" in s["name"] for s in stats)


def test_scalar_kernel_is_refused_beyond_64_tokens():
    """bf16 with option attn_mfma = 0 and a 16 x 16 attention level: the scalar kernel's LDS tiles hold 64 tokens, build_plan must refuse before anything is launched
    (as it always did for fp16 / fp32)"""
    import terrain_diffusion_amd as td
    from oracle.unet import synth_state_dict, tiny_config
    from terrain_diffusion_amd._lib import TdError
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    cfg = tiny_config(64, 1)
    sd = synth_state_dict(cfg, seed=77)
    x = torch.randn(1, cfg["in_channels"], 128, 128, device="cuda")
    c = [torch.randn(1, ci[1], device="cuda") for ci in cfg.get("conditional_inputs", [])]
    for T, opt in (("bf16", 0), ("fp16", 1), ("fp32", 1)):
        m = td.EDMUnet2D(**cfg, dtype=T).load_state_dict(sd)
        try:
            with pinned(eng, attn_mfma=opt):
                with pytest.raises(TdError, match="64 tokens"):
                    m(x, torch.full((1,), 0.9), c)
        finally:
            m.close()


def test_summary():
    print("\n" + "\n".join(l for l in LINES if l.startswith("ARM")))
