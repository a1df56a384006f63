"""Every fused conv op of the EDMAutoencoder's two stacks, element by element, against the float64 twin of the same op on the op's own stored inputs
(tests/_conv_twin.py: `describe_ae`, `check_forward` with the staged `@xin` as the input source and one row of ones as the modulation), read back with
`EDMAutoencoder.read_activation` (td_ae_read_activation): |hip - ref| <= half_ulp_T(ref) + E for EVERY element of every op, and the sum-of-squares planes of every op
that writes them.  One arm per (stack, storage type, batch, map, engine options); each arm runs `preencode` or `decode` with profile = 1, asserts that the twin
describes exactly the conv ops launched and -- from the profile labels -- that the intended flavour ran, and prints `summary_line`, the flavour counts and the wall
time.  The predicates were predicted on the CPU with csrc/conv_select.h (tests/conv_select_harness.cpp fed the twin's op list at the arm's shape and options).

What these stacks launch and no U-Net plan does: `decoder_conv` (1x1, one K chunk, latent + direct + ones channels straight from the staged input), a
channel-changing decoder block's `conv_res1` with ONE untransformed 1x1 tail (mul = kMixRes), `encoder.out_conv` (2 * latent_channels fp32 couts on the narrow
bottleneck map), EPI_EMB_SILU fed from one shared row of ones, maps that grow from a narrow odd-sized latent (5x7 -> 10x14 -> 20x28 -> 40x56: the 8- and 16-wide tiles hang
over the edge at every level), and the dihedral batch n = 8 on the narrow tiles that pack 2 or 4 images.

Not forced: the 16x16x32 wide tile (`f2w ... x16`) needs a 96-cout tile, and these channel counts (64 / 128 / 256) never give it one.

The boundary checks at the end use the same read-back and are bit for bit: the staged encoder input, the latent head, the decoder's output, and determinism."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ae_twin as A
import _conv_twin as ct
from _engine_opts import engine_options_guard, pinned  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)
from test_ae_conv_ops_cpu import ATTN
from test_autoencoder_gpu import DEEP

pytestmark = pytest.mark.gpu

SEEN = {}          # arm -> {label: (tag, ksplit)}: which flavours were exercised, for the coverage test at the end of the file
CONFIGS = {"released": (A.RELEASED, 78), "tiny": (A.TINY, 77), "attn": (ATTN, 80), "deep": (DEEP, 79)}
ENC, DEC = 1, 2


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def zoo(td):
    """models and twins, built on first use and shared by the arms"""
    sds, models, twins = {}, {}, {}

    def get(which, T, kind=None):
        cfg, seed = CONFIGS[which]
        if which not in sds:
            sds[which] = A.synth_ae_state_dict(cfg, seed=seed)
        if (which, T) not in models:
            models[(which, T)] = td.EDMAutoencoder(**cfg, dtype=T).load_state_dict(sds[which])
        if kind is not None and (which, T, kind) not in twins:
            ops, width = ct.describe_ae(cfg, kind)
            twins[(which, T, kind)] = ct.Twin(cfg, sds[which], T, "cuda", ops=ops, c_total=width)
        return cfg, models[(which, T)], twins.get((which, T, kind))

    yield get
    for m in models.values():
        m.close()


def _rng(seed, shape):
    from oracle import rng
    return torch.from_numpy(rng.standard_normal(seed, shape))


def _count(fl, *prefixes):
    return sum(tag.startswith(prefixes) for tag, _ in fl.values())


def _ks(fl):
    return sum(ks > 1 for _, ks in fl.values())


def _single_tails(tw):
    """the channel-changing decoder blocks' conv_res1: a 3x3 segment plus ONE 1x1 tail"""
    return [o["label"] for o in tw.ops if len(o["segs"]) == 2 and o["segs"][1]["taps"] == 1 and o["label"].endswith(".conv_res1")]


def _no_small(fl):
    return _count(fl, "f4", "f5") == 0


def _all(fl, *prefixes):
    return all(tag.startswith(prefixes) for tag, _ in fl.values())


# name -> (model, stack, T, n, H, W of the stack's own input, engine options, check of the flavours that ran: f(flavours, twin) -> bool).
# A stack name "enc8" is the encoder's dihedral form: n_src = n / 8 sources, the 8 views made by the staging kernel.
ARMS = {
    # the released decoder from a 5x7 latent: maps 5x7, 10x14, 20x28, 40x56; n = 3 is odd against the 2- and 4-image groups of the narrow tiles
    "released dec bf16 n3 5x7 default plan": ("released", DEC, "bf16", 3, 5, 7, {}, lambda fl, tw: _count(fl, "f4") >= 20 and _count(fl, "f5c16") >= 6 and _ks(fl) >= 8),
    "released dec bf16 n3 5x7 sb0 split-K": ("released", DEC, "bf16", 3, 5, 7, dict(sb=0, glds_splitk=1),
                                             lambda fl, tw: _no_small(fl) and _ks(fl) >= 4 and any(fl[l][1] > 1 for l in _single_tails(tw))),
    "released dec bf16 n3 5x7 sb0 no split-K": ("released", DEC, "bf16", 3, 5, 7, dict(sb=0, glds_splitk=0),
                                                lambda fl, tw: _no_small(fl) and all(ks == 1 or tag == "f0" for tag, ks in fl.values())),
    "released dec bf16 n3 5x7 wide forced": ("released", DEC, "bf16", 3, 5, 7, dict(glds_wide=2, glds_splitk=0),
                                             lambda fl, tw: _count(fl, "f2w") >= 6 and any(fl[l][0] == "f2w" and tw.by_label[l]["cout"] == 64 for l in _single_tails(tw))),
    "released dec bf16 n3 5x7 per-tap kernel": ("released", DEC, "bf16", 3, 5, 7, dict(glds=0), lambda fl, tw: _all(fl, "f0")),
    "released dec bf16 n1 5x7 default plan": ("released", DEC, "bf16", 1, 5, 7, {}, lambda fl, tw: _count(fl, "f4", "f5") >= 10),
    "released dec bf16 n1 5x7 s16 everywhere": ("released", DEC, "bf16", 1, 5, 7, dict(s16=2), lambda fl, tw: _count(fl, "f5c16") >= 10),
    "released dec bf16 n8 5x7 default plan": ("released", DEC, "bf16", 8, 5, 7, {}, lambda fl, tw: _count(fl, "f4m2n2") >= 12 and _count(fl, "f5c16") >= 8),
    "released dec fp16 n3 5x7 default plan": ("released", DEC, "fp16", 3, 5, 7, {}, lambda fl, tw: _count(fl, "f4") >= 20 and _count(fl, "f5c16") >= 6 and _ks(fl) >= 8),
    "released dec fp32 n3 5x7": ("released", DEC, "fp32", 3, 5, 7, {}, lambda fl, tw: _all(fl, "f0")),
    # its 128x128 output is the smallest map conv_select gives the few-cout kernel
    "released dec bf16 n1 16x16 fewcout": ("released", DEC, "bf16", 1, 16, 16, dict(fewcout=1), lambda fl, tw: fl["out_conv"][0] == "f6"),
    "released dec bf16 n1 16x16 no fewcout": ("released", DEC, "bf16", 1, 16, 16, dict(fewcout=0), lambda fl, tw: fl["out_conv"][0] != "f6"),
    # the released encoder on a 40x56 image (bottleneck 5x7), and the dihedral batch of one 48x48 chunk (n = 8, bottleneck 6x6)
    "released enc bf16 n3 40x56 default plan": ("released", ENC, "bf16", 3, 40, 56, {}, lambda fl, tw: _count(fl, "f4") >= 15 and _count(fl, "f5c16") >= 4 and _ks(fl) >= 6),
    "released enc bf16 n3 40x56 sb0 split-K": ("released", ENC, "bf16", 3, 40, 56, dict(sb=0, glds_splitk=1), lambda fl, tw: _no_small(fl) and _ks(fl) >= 4),
    "released enc bf16 n3 40x56 sb0 no split-K": ("released", ENC, "bf16", 3, 40, 56, dict(sb=0, glds_splitk=0),
                                                  lambda fl, tw: _no_small(fl) and all(ks == 1 or tag == "f0" for tag, ks in fl.values())),
    "released enc bf16 n3 40x56 wide forced": ("released", ENC, "bf16", 3, 40, 56, dict(glds_wide=2, glds_splitk=0), lambda fl, tw: _count(fl, "f2w") >= 6),
    "released enc bf16 n3 40x56 per-tap kernel": ("released", ENC, "bf16", 3, 40, 56, dict(glds=0), lambda fl, tw: _all(fl, "f0")),
    "released enc bf16 n1 40x56 default plan": ("released", ENC, "bf16", 1, 40, 56, {}, lambda fl, tw: _count(fl, "f4", "f5") >= 10),
    "released enc bf16 n1 40x56 s16 everywhere": ("released", ENC, "bf16", 1, 40, 56, dict(s16=2), lambda fl, tw: _count(fl, "f5c16") >= 10),
    "released enc bf16 dihedral n8 48x48 default plan": ("released", "enc8", "bf16", 8, 48, 48, {}, lambda fl, tw: _count(fl, "f4m2n2") >= 8 and _count(fl, "f5c16") >= 4),
    "released enc fp16 n3 40x56 default plan": ("released", ENC, "fp16", 3, 40, 56, {}, lambda fl, tw: _count(fl, "f4") >= 15 and _count(fl, "f5c16") >= 4 and _ks(fl) >= 6),
    "released enc fp16 dihedral n8 48x48 default plan": ("released", "enc8", "fp16", 8, 48, 48, {}, lambda fl, tw: _count(fl, "f4m2n2") >= 8 and _count(fl, "f5c16") >= 4),
    "released enc fp32 n1 40x56": ("released", ENC, "fp32", 1, 40, 56, {}, lambda fl, tw: _all(fl, "f0")),
    # mid-block attention, a direct skip, 2 input channels
    "tiny enc bf16 n2 16x16": ("tiny", ENC, "bf16", 2, 16, 16, {}, lambda fl, tw: _count(fl, "f4") >= 5 and fl["encoder.out_conv"][0] == "f0"),
    "tiny enc bf16 n3 24x40": ("tiny", ENC, "bf16", 3, 24, 40, {}, lambda fl, tw: _count(fl, "f5c16") >= 5 and fl["encoder.out_conv"][0].startswith("f4")),
    "tiny dec bf16 n2 8x8": ("tiny", DEC, "bf16", 2, 8, 8, {}, lambda fl, tw: sum(l.endswith(".attn_proj") for l in fl) == 1),
    "tiny dec bf16 n3 12x20": ("tiny", DEC, "bf16", 3, 12, 20, {}, lambda fl, tw: sum(l.endswith(".attn_proj") for l in fl) == 1),
    # attention in encoder and decoder blocks, a decoder with its own layers per block
    "attention enc bf16 n3 16x16": ("attn", ENC, "bf16", 3, 16, 16, {}, lambda fl, tw: sum(l.endswith(".attn_proj") for l in fl) >= 1),
    "attention dec bf16 n3 8x8": ("attn", DEC, "bf16", 3, 8, 8, {}, lambda fl, tw: sum(l.endswith(".attn_proj") for l in fl) >= 3),
    # four levels of 64 channels
    "deep enc bf16 n3 48x48": ("deep", ENC, "bf16", 3, 48, 48, {}, lambda fl, tw: _count(fl, "f0") >= 6 and _count(fl, "f4", "f5") >= 6),
    "deep dec bf16 n3 6x6": ("deep", DEC, "bf16", 3, 6, 6, {}, lambda fl, tw: _count(fl, "f0") >= 10 and _count(fl, "f4", "f5") >= 10),
}


def _stack_input(cfg, stack, n, H, W):
    """the stack's own input (fp32, host): images for the encoder -- n / 8 sources for its dihedral form --, latents for the decoder"""
    if stack == DEC:
        return _rng(9, (n, cfg["latent_channels"] + len(cfg.get("direct_skips") or []), H, W))
    return _rng(8, (n // 8 if stack == "enc8" else n, cfg["in_channels"], H, W)) * 1.3 + 0.2


def _run(m, stack, x):
    """one engine call on the stack -> what it returned"""
    if stack == DEC:
        return (m.decode(x.cuda()),)
    return m._preencode(x.cuda(), 0.3, 1.7, stack == "enc8", True)


def _profiled(eng, m, stack, x):
    with pinned(eng, profile=1):
        eng.profile_read(reset=True)
        out = _run(m, stack, x)
        torch.cuda.synchronize()
        rows = eng.profile_ops()
    eng.profile_read(reset=True)
    fl = {}
    for r in rows:
        if " [" in r[0]:
            lab, tag, ks = ct.flavour_of(r[0])
            fl[lab] = (tag, ks)
    return out, fl


@pytest.mark.parametrize("arm", list(ARMS))
def test_every_autoencoder_conv_op_elementwise_against_its_float64_twin(td, zoo, arm):
    from terrain_diffusion_amd.engine import get_engine
    which, stack, T, n, H, W, opts, intended = ARMS[arm]
    kind = DEC if stack == DEC else ENC
    eng = get_engine("cuda")
    cfg, m, tw = zoo(which, T, kind)
    x = _stack_input(cfg, stack, n, H, W)
    t0 = time.time()
    with pinned(eng, **opts):
        out, fl = _profiled(eng, m, stack, x)
        SEEN[arm] = (kind, tw, fl)
        assert set(fl) == set(tw.by_label), set(fl) ^ set(tw.by_label)      # the twin describes exactly the conv ops the engine launched
        assert intended(fl, tw), f"{arm}: the intended flavours did not run: {sorted(fl.items())}"
        # (under the arm's options: they are part of the plan's key)
        stats, nss = ct.check_forward(ct.ae_stack(m, kind), tw, torch.empty(n, 1, H, W), None, None, T, fl, cvec=ct.ones_cvec(n, tw.c_total), stored_input=True)
    tags = {}
    for tag, ks in fl.values():
        key = tag + (" ks>1" if ks > 1 else "")
        tags[key] = tags.get(key, 0) + 1
    w = max(stats, key=lambda s_: s_["worst"])
    print("\n" + ct.summary_line(arm, stats, nss, time.time() - t0) + f"   worst op {w['label']} [{w['flavour']}]   flavours " + " ".join(f"{k}:{v}" for k, v in sorted(tags.items())))
    if os.environ.get("TD_AE_OPS_TABLE"):
        for s_ in stats:
            print(f"      {s_['label']:44s} {s_['flavour']:14s} worst {s_['worst']:7.3f}  not RNE {100 * s_['rounded_off']:7.3f} %  median {s_['median']:.3f}")
    assert len(stats) == len(tw.ops) and nss == sum(o["sumsq"] for o in tw.ops)
    assert all(torch.isfinite(o).all() for o in out if o is not None)


def test_every_autoencoder_op_shape_and_flavour_was_exercised_by_some_arm():
    """each of the four op shapes only the autoencoder has -- decoder_conv, the single-tail conv_res1, encoder.out_conv, conv_res0 without an embedding -- ran on at
    least two kernel families (the flavour tag's first two characters: f0 per-tap, f2 LDS-DMA, f4 small-batch, f5 64 px x 16 couts, f6 few-cout), and the tags f0,
    f2b or f2s, f2w, some f4*, f5c16, f6 and a split-K launch each occurred (this test reads what the arms recorded: it belongs to a run of the whole file)"""
    assert len(SEEN) == len(ARMS), f"only {len(SEEN)} of {len(ARMS)} arms recorded their flavours: run the whole file"
    shapes = {"decoder_conv": lambda kind, tw, l: l == "decoder_conv",
              "single-tail conv_res1": lambda kind, tw, l: l in _single_tails(tw),
              "encoder.out_conv": lambda kind, tw, l: l == "encoder.out_conv",
              "conv_res0 without an embedding": lambda kind, tw, l: l.endswith(".conv_res0")}
    for name, is_one in shapes.items():
        fam = {tag[:2] for kind, tw, fl in SEEN.values() for l, (tag, _) in fl.items() if is_one(kind, tw, l)}
        assert len(fam) >= 2, f"{name} ran on {sorted(fam)} only"
    tags = {tag for _, _, fl in SEEN.values() for tag, _ in fl.values()}
    assert {"f0", "f2w", "f5c16", "f6"} <= tags and tags & {"f2b", "f2s"} and any(t.startswith("f4") for t in tags), tags
    assert any(ks > 1 for _, _, fl in SEEN.values() for _, ks in fl.values())


# ------------------------------------------------------------------------------------------------ the read-back itself
REFUSED = ("@emb", "@cvec", "@emb:rows", "@cvec:rows", "@x", "@m1", "@m2", "@xt")


@pytest.mark.parametrize("label", REFUSED)
def test_read_back_refuses_what_the_stacks_do_not_have(zoo, label):
    """a kind != 0 plan has no embedding or cvec buffer and 16 bytes of sampler state: these labels are refused with TD_ERR_ARG on either stack, before anything is
    read, also after a call on that plan; so is a stack that is neither 1 nor 2"""
    import ctypes as C
    import numpy as np
    from terrain_diffusion_amd._lib import ae_lib as lib
    _, m, _ = zoo("tiny", "bf16")
    m.preencode(_rng(3, (1, 2, 16, 16)).cuda())
    m.decode(_rng(4, (1, 3, 8, 8)).cuda())
    buf = np.full(1 << 16, 7.0, dtype=np.float32)
    dims = (C.c_int32 * 4)()
    for stack, (H, W) in ((1, (16, 16)), (2, (8, 8))):
        rc = lib().td_ae_read_activation(m._h, stack, 1, H, W, label.encode(), C.c_void_p(buf.ctypes.data), buf.size, C.byref(dims))
        assert rc == -1 and label.encode() in lib().td_last_error(), (stack, rc, lib().td_last_error())       # TD_ERR_ARG
        with pytest.raises(Exception):
            m.read_activation(stack, 1, H, W, label)
    assert bool((buf == 7.0).all())
    assert lib().td_ae_read_activation(m._h, 3, 1, 16, 16, b"@xin", C.c_void_p(buf.ctypes.data), buf.size, C.byref(dims)) == -1
    assert m.read_activation(1, 1, 16, 16, "@xin").shape == (1, 64, 16, 16)          # ... and what the stacks do have is served


# ------------------------------------------------------------------------------------------------ boundary checks, bit for bit
def _rne(x, T):
    return x.to(ct.TORCH_T[T]).to(torch.float32)


@pytest.mark.parametrize("T", ["bf16", "fp16"])
@pytest.mark.parametrize("form", ["plain", "dihedral"])
def test_staged_encoder_input_is_the_rounded_normalised_image(zoo, T, form):
    """@xin of the encoder = RNE_T(fp32((x - mean) / std)), one subtraction and one true division on the CPU, the eight views those of _ae_twin.dihedral_views; the
    ones channel is exactly 1 and every padding channel of the K chunk exactly 0"""
    cfg, m, _ = zoo("tiny", T)
    C = cfg["in_channels"]
    mean, std = 0.3, 1.7
    if form == "plain":
        x = _rng(21, (3, C, 24, 40)) * 1.3 + 0.2
        want = ((x - mean) / std).float()
    else:
        x = _rng(22, (1, C, 48, 48)) * 1.3 + 0.2
        want = torch.stack(A.dihedral_views(((x[0] - mean) / std).float()))
    n, _, H, W = want.shape
    m._preencode(x.cuda(), mean, std, form == "dihedral", True)
    xin = m.read_activation(1, n, H, W, "@xin")
    assert xin.shape == (n, 64, H, W)
    assert torch.equal(xin[:, :C], _rne(want, T))
    assert bool((xin[:, C] == 1.0).all()) and bool((xin[:, C + 1:] == 0.0).all())


@pytest.mark.parametrize("T", ["bf16", "fp16"])
def test_latent_head_is_the_stored_encoder_out_conv(zoo, T):
    """means[:, :L] and logvars[:, :L] are the two halves of the stored fp32 encoder.out_conv, packed_f16 = RNE_fp16(cat(means, logvars))"""
    cfg, m, _ = zoo("tiny", T)
    L = cfg["latent_channels"]
    x = _rng(23, (3, cfg["in_channels"], 24, 40))
    means, logvars, packed = m._preencode(x.cuda(), 0.0, 1.0, False, True)
    F = m.read_activation(1, 3, 24, 40, "encoder.out_conv")
    assert F.shape == (3, 2 * L, 12, 20)
    assert torch.equal(means[:, :L].cpu(), F[:, :L]) and torch.equal(logvars[:, :L].cpu(), F[:, L:2 * L])
    assert torch.equal(packed.cpu(), torch.cat([means, logvars], dim=1).cpu().to(torch.float16))


@pytest.mark.parametrize("T", ["bf16", "fp16"])
def test_decoder_output_is_the_stored_out_conv_and_the_direct_channels(zoo, T):
    """decode(z) with std = 1, mean = 0: the non-direct channels are the stored fp32 out_conv, the direct ones the nearest-neighbour upsampling of z[:, L:]"""
    cfg, m, _ = zoo("tiny", T)
    L, direct = cfg["latent_channels"], cfg["direct_skips"]
    z = _rng(24, (3, L + len(direct), 5, 7))
    y = m.decode(z.cuda()).cpu()
    F = m.read_activation(2, 3, 5, 7, "out_conv")
    assert y.shape == F.shape == (3, cfg["in_channels"], 10, 14)
    keep = [c for c in range(y.shape[1]) if c not in direct]
    assert keep and torch.equal(y[:, keep], F[:, keep])
    for d, c in enumerate(direct):
        assert torch.equal(y[:, c], z[:, L + d].float().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))


@pytest.mark.parametrize("stack", [ENC, DEC])
def test_same_call_twice_stores_the_same_tensors(zoo, stack):
    """determinism: every conv op's stored tensor, the sum-of-squares planes and the staged input of a second identical call equal the first's, on the released
    model in bf16 at n = 3 (split-K and multi-image tiles included: whatever the default plan chose)"""
    cfg, m, tw = zoo("released", "bf16", stack)
    n, H, W = (3, 40, 56) if stack == ENC else (3, 5, 7)
    x = _stack_input(cfg, stack, n, H, W)
    labels = ["@xin"] + [o["label"] for o in tw.ops] + ["sumsq:" + o["label"] for o in tw.ops if o["sumsq"]]
    reads = []
    for _ in range(2):
        _run(m, stack, x)
        reads.append([m.read_activation(stack, n, H, W, l, max_elems=1 << 22) for l in labels])
    for l, a, b in zip(labels, *reads):
        assert torch.equal(a, b), l
