"""CPU tests of the conv-op twin on the EDMAutoencoder's two graphs (tests/_conv_twin.py: `describe_ae`), and of the twin's op lists against the engine's graph:
(a) `describe` / `describe_ae` equal csrc/model_graph.h field for field on every model of tests/golden/model_graph.npz (tests/model_graph_harness.cpp prints the
graph); (b) chained in float64 without rounding, `describe_ae` IS `_ae_twin.AETwin`, which is pinned to the reference's recorded outputs; the storage-type
modes start from the very fp32 weights `EDMAutoencoder.load_state_dict` hands the engine; (c) the float32 emulation of every autoencoder op passes `check_op` with
zero violations in bf16, fp16 and fp32 at small, ragged map sizes; (d) `check_op` flags four kernel bugs particular to these graphs that
the whole-network 2e-2 rel-RMS bound of tests/test_autoencoder_gpu.py lets through.

Printed by (c) (torch 2.10 CPU, +-5 % from run to run; worst over both stacks and all shapes of the model; the constants of _conv_twin.py stay as they are):
    model     T     acc    acc32  epi_emb  epi_res  ss     largest median E / half_ulp (op)
    tiny      bf16  1.76   -      4.08     1.89     0.35   0.011 (encoder.enc.8x8_block0.conv_res0)
    tiny      fp16  2.02   -      4.15     1.96     0.42   0.123 (encoder.enc.8x8_block0.conv_res0)
    tiny      fp32  -      1.80   3.61     2.12     0.42   -
    released  bf16  2.24   -      4.31     2.17     0.40   0.017 (encoder.enc.64x64_down.conv_res0)
    released  fp16  2.15   -      4.30     2.18     0.47   0.169 (encoder.enc.64x64_down.conv_res0)
    released  fp32  -      1.88   3.84     2.38     0.42   -
against the U-Net's recorded 2.26 / 1.74 / 4.93 / 0.42: acc32 on the released model is above its recorded value (1.88 against 1.74; 8 x 1.88 = 15.0 <= C_ACC32), and so is the
sum of squares in fp16 (0.47; 4 x 0.47 <= C_SS).  The 16-bit rows of the released model include the 48x48 chunk of the dihedral form and the 16x16 latent of the few-cout arm
(without them: acc 1.72 / 1.84); their largest values come from the 64 -> 64 convs of the 128x128 level, the U-Net decoder's own op shape at 10^6 elements per op -- the
extreme of more samples, not another shape.  In fp32 mode, whose GPU arms stay at 5x7 and 40x56, those two maps are not emulated: there the same convs give acc32 = 2.22
(`decoder.15.conv_res0`), with which `check_op` still passes at worst 0.11 but C_ACC32 = 16 is 7.2 x the emulation, not 8 x.
One op shape was worse than everything recorded, and its model was tightened: the encoder's 3x3 input conv of 1 + 1 (released) or 2 + 1 (tiny) channels gave
acc = 3.72 / 3.42 in fp16 while the slack counted K / 16 = 18 / 16 or 27 / 16 accumulate steps for it; it takes 9, one per tap (`_conv_twin.acc_steps`, the
module's docstring under "accumulation"), and over the right count the same errors are 1.3 / 1.5.  `decoder_conv` (K = 5 resp. 4 real products, one tap, ONE accumulate
step: the matrix core rounds the exact sum once) has the smallest accumulation error of all ops, worst (|err| - half_ulp) / E = 0.00 - 0.09 and a median
E / half_ulp of 0.0007 (bf16) / 0.0057 (fp16): nothing to tighten there."""
import math
import os
import struct
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ae_twin as A
import _conv_twin as ct
from oracle import rng
from test_model_graph_cpu import GOLDEN, harness  # noqa: F401  (the fixture that builds tests/model_graph_harness.cpp)

BOUNDS = {"fp32": 5e-6, "bf16": 2e-2, "fp16": 4e-3}     # tests/test_autoencoder_gpu.py's whole-network bounds
# attention in an encoder block (with a skip conv in front) and in decoder blocks, mid-block attention, and a decoder with its own layers per block
ATTN = dict(image_size=16, in_channels=2, model_channels=64, model_channel_mults=[1, 2], layers_per_block=1, layers_per_block_decoder=[2, 1], attn_resolutions=[8],
            midblock_attention=True, latent_channels=2, direct_skips=[1])
CONFIGS = {"tiny": (A.TINY, 77), "released": (A.RELEASED, 78), "attn": (ATTN, 80)}


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


# ---------------------------------------------------------------------------------------------- (a) the twin's op lists are the engine's graph
EPI = {0: "plain", 1: "emb", 2: "res"}


def _engine_ops(lines):
    """the harness's conv / seg / attn records as comparable tuples, tensor ids replaced by the label of the op that writes them"""
    names, ops, i = {0: "@input"}, [], 0
    recs = [l.split(" ") for l in lines]
    while i < len(recs):
        f = recs[i]
        i += 1
        if f[0] == "attn":
            label, qkv, out = f[1], int(f[4]), int(f[5])
            assert names[qkv] == label + "_qkv"
            names[out] = label
        elif f[0] == "conv":
            label, level, cout, epi, cvec_off, res, res_rs, res_norm, clip, sumsq, f32o, out, nseg = [f[1]] + [int(v) for v in f[2:14]]
            segs = []
            for s in recs[i:i + nseg]:
                assert s[0] == "seg"
                segs.append((s[1], s[2], int(s[3]), int(s[4]), int(s[5]), int(s[7]), names[int(s[9])], int(s[10]), int(s[11]), int(s[8]), int(s[12])))
            i += nseg
            names[out] = label
            ops.append((label, level, cout, EPI[epi], cvec_off, names[res] if res >= 0 else None, res_rs, bool(res_norm), clip, bool(sumsq), bool(f32o), tuple(segs)))
    return ops


def _twin_ops(ops):
    out = []
    for o in ops:
        segs = tuple((s["wname"], s["gain"] or "-", s["cin_tot"], s["cin_off"], s["C"], s["taps"], s["src"], s["resample"], s["xform"], _bits(s["mul32"]), _bits(s["scale32"]))
                     for s in o["segs"])
        r = o["res"]
        out.append((o["label"], o["shift"], o["cout"], o["epi"], o["cvec_off"], r["src"] if r else None, r["resample"] if r else 0, bool(r and r["norm"]), _bits(o["clip"]),
                    bool(o["sumsq"]), bool(o["out_f32"]), segs))
    return out


def _python_config(c):
    """the constructor arguments a harness config stands for (td_unet_config as unet.py / td_ae_create fill it)"""
    n = c["n_levels"]
    cfg = dict(image_size=c["image_size"], model_channels=c["model_channels"], model_channel_mults=c["channel_mults"][:n], layers_per_block=c["layers_per_block"][:n],
               attn_resolutions=c["attn_resolutions"][:c["n_attn_resolutions"]], midblock_attention=bool(c["midblock_attention"]), out_channels=c["out_channels"])
    if c["kind"] == 0:
        cfg.update(in_channels=c["in_channels"], concat_balance=struct.unpack("<f", struct.pack("<I", c["concat_balance_bits"]))[0])
    elif c["kind"] == 1:    # the encoder stack: out_channels = 2 * latent_channels
        cfg.update(in_channels=c["in_channels"], latent_channels=c["out_channels"] // 2, direct_skips=[])
    else:                   # the decoder stack: in_channels = latent + direct channels (decoder_conv sees only their sum)
        cfg.update(in_channels=c["out_channels"], latent_channels=c["in_channels"], direct_skips=[], layers_per_block_decoder=c["layers_per_block_decoder"][:n])
    return cfg


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_twin_op_list_equals_the_engine_graph(harness, name):
    """Per op: label, level <-> shift, cout, epilogue, cvec_off, residual source / resample / norm, clip, want_sumsq, out_f32; per K-segment: weight name, gain,
    cin_tot, cin_off, c_real, taps, source label, resample, xform, and mul / scale as fp32 bit patterns.  The five U-Net configs and the four autoencoder stacks,
    each at both K-chunk widths (the twin has no c_pad: the two must give it the same list)."""
    c = GOLDEN[name]["config"]
    lines = harness(c)
    assert not lines[0].startswith("error"), lines[0]
    eng = _engine_ops(lines)
    cfg = _python_config(c)
    ops, width = ct.describe(cfg) if c["kind"] == 0 else ct.describe_ae(cfg, c["kind"])
    tw = _twin_ops(ops)
    bad = [f"op {i}: twin {a!r}\n        graph {b!r}" for i, (a, b) in enumerate(zip(tw, eng)) if a != b]
    assert not bad and len(tw) == len(eng), f"{len(bad)} of {len(eng)} ops differ ({len(tw)} in the twin):\n" + "\n".join(bad[:6])
    sc = next(l.split(" ") for l in lines if l.startswith("scalars "))
    assert width == (int(sc[3]) if c["kind"] == 0 else int(sc[5]))           # c_total, or max_cout: the width of the row of ones
    assert ct.gains_of(ops) == {sc[7] + ".weight": sc[8]}                    # out_label, out_gain_name
    assert len(eng) > 3


def test_autoencoder_op_shapes_that_no_unet_plan_has():
    ops, width = ct.describe_ae(A.RELEASED, 2)
    by = {o["label"]: o for o in ops}
    dc = by["decoder_conv"]
    assert (dc["K"], dc["cout"], dc["shift"], dc["epi"]) == (5, 256, 0, "plain") and dc["segs"][0]["taps"] == 1 and dc["segs"][0]["src"] == "@input"
    tails = [o for o in ops if len(o["segs"]) == 2]
    assert [o["label"] for o in tails] == ["decoder.10.conv_res1", "decoder.14.conv_res1"] and not any(len(o["segs"]) > 2 for o in ops)
    for o in tails:
        s = o["segs"][1]
        assert (s["taps"], s["xform"], s["resample"], _bits(s["mul32"])) == (1, 0, 0, _bits(ct.KMIX_RES32)) and o["res"] is None
    assert [o["shift"] for o in ops][0] == 0 and min(o["shift"] for o in ops) == -3 == by["out_conv"]["shift"]
    assert all(o["cvec_off"] == 0 for o in ops if o["epi"] == "emb") and width == 256
    ops, _ = ct.describe_ae(A.RELEASED, 1)
    out = ops[-1]
    assert (out["label"], out["cout"], out["shift"], out["out_f32"], out["segs"][0]["gain"]) == ("encoder.out_conv", 8, 3, True, "encoder.out_gain")


# ---------------------------------------------------------------------------------------------- (b) the chain in float64, and the folded weights
def _stack_inputs(cfg, kind, n, H, W, seed=7):
    """the stack's own input: an image for the encoder, a latent for the decoder"""
    C = cfg["in_channels"] if kind == 1 else cfg["latent_channels"] + len(cfg.get("direct_skips") or [])
    return torch.from_numpy(rng.standard_normal(seed + kind, (n, C, H, W)))


def _twin(cfg, sd, kind, mode):
    ops, width = ct.describe_ae(cfg, kind)
    return ct.Twin(cfg, sd, mode, ops=ops, c_total=width)


@pytest.mark.parametrize("which", list(CONFIGS))
def test_twin_chained_in_float64_is_the_reference_autoencoder(which):
    cfg, seed = CONFIGS[which]
    sd = A.synth_ae_state_dict(cfg, seed=seed)
    ref = A.AETwin(cfg, sd, dtype=torch.float64)
    L = cfg["latent_channels"]
    worst, checked = [], 0
    for kind, (n, H, W) in ((1, (2, 16, 16)), (2, (2, 5, 7))):
        tw = _twin(cfg, sd, kind, "exact")
        x = _stack_inputs(cfg, kind, n, H, W)
        stored = ct.run_chain(tw, x, ct.ones_cvec(n, tw.c_total, torch.float64))
        taps = {}
        if kind == 1:
            means, logvars = ref.preencode(x, taps)
            enc = stored["encoder.out_conv"]
            worst += [("means", A.rel_rms(enc[:, :L], means[:, :L])), ("logvars", A.rel_rms(enc[:, L:], logvars[:, :L]))]
        else:
            y = ref.decode(x, taps)
            keep = [c for c in range(y.shape[1]) if c not in cfg["direct_skips"]]
            worst.append(("out_conv", A.rel_rms(stored["out_conv"][:, keep], y[:, keep])))
        for name, t in taps.items():
            lab = name if name in tw.by_label else (name + ".attn_proj" if name + ".attn_proj" in tw.by_label else name + ".conv_res1")
            worst.append((lab, A.rel_rms(stored[lab], t)))
            checked += 1
    w = max(worst, key=lambda p: p[1])
    print(f"{which}: {checked} block outputs + the two heads; worst rel-RMS against AETwin(float64) {w[1]:.2e} at {w[0]}")
    assert checked == len(A.ae_plan(cfg)["enc"]) + len(A.ae_plan(cfg)["dec"]) and w[1] <= 1e-12, worst


def test_twin_folds_autoencoder_weights_bit_for_bit_like_the_host_that_feeds_the_engine():
    """what `EDMAutoencoder.load_state_dict(fold="reference")` hands td_ae_set_param (its own loop: `EDMUnet2D._fold_reference` with encoder.out_gain / out_gain as
    fp32 tensors, 1 elsewhere) against `Twin.folded`; only host-side code is used: no GPU."""
    from terrain_diffusion_amd.unet import EDMUnet2D
    gains = {"encoder.out_conv.weight": "encoder.out_gain", "out_conv.weight": "out_gain"}      # terrain_diffusion_amd/autoencoder.py: load_state_dict
    n = 0
    for cfg, seed in CONFIGS.values():
        sd = A.synth_ae_state_dict(cfg, seed=seed, enc_out_gain=0.8, out_gain=0.3)
        seen = set()
        for kind in (1, 2):
            tw = _twin(cfg, sd, kind, "bf16")
            assert tw.gains == {k: v for k, v in gains.items() if k in tw.folded}
            for name, w in tw.folded.items():
                gain = torch.as_tensor(sd[gains[name]]).to(torch.float32) if name in gains else 1
                assert torch.equal(w, EDMUnet2D._fold_reference(torch.as_tensor(sd[name]).to(torch.float32), gain)), name
                n += 1
            seen |= set(tw.folded)
        assert seen == {k for k in A.ae_param_shapes(cfg) if k.endswith(".weight")}          # every weight inference reads, through one stack or the other
    assert n > 80


# ---------------------------------------------------------------------------------------------- (c) the float32 emulation
# (model, stack) -> (n, H, W) of the stack's own input, the maps of tests/test_ae_conv_ops_gpu.py's arms: released: latent 5x7 / image 40x56 (the 8- and 16-wide tiles hang
# over at every level), the 48x48 chunk of the dihedral form (bottleneck 6x6; two of its eight views' worth of images) and the 16x16 latent of the few-cout arm (128x128
# output); tiny: 16x16 and 24x40.  The median E / half_ulp of an op depends on its map and channel counts, not on the batch.  A fourth entry names the storage types
# whose GPU arms use that map (the dihedral arms are bf16 and fp16, the few-cout arm bf16 and -- for the median condition, a 16-bit matter -- fp16 here as well).
EMUL_SHAPES = {("tiny", 1): [(2, 16, 16), (1, 24, 40)], ("tiny", 2): [(2, 8, 8), (1, 12, 20)], ("released", 1): [(1, 40, 56), (2, 48, 48, ("bf16", "fp16"))],
               ("released", 2): [(1, 5, 7), (1, 16, 16, ("bf16", "fp16"))]}


@pytest.mark.parametrize("which,T", [(m, T) for m in ("tiny", "released") for T in ("bf16", "fp16", "fp32")])
def test_float32_emulation_of_every_autoencoder_op_passes_check_op(which, T):
    """zero violations on every op of both stacks; the constants keep the margins tests/test_conv_ops_cpu.py asserts for the U-Net; the median condition
    E / half_ulp <= 0.5 (asserted by `check_op` on every 16-bit op) holds for the emulation alone at these shapes.  The ratio table is in the module docstring."""
    cfg, seed = CONFIGS[which]
    sd = A.synth_ae_state_dict(cfg, seed=seed)
    ratios, stats, nops = {}, [], 0
    t0 = time.time()
    for kind in (1, 2):
        tw = _twin(cfg, sd, kind, T)
        for n, H, W, *only in EMUL_SHAPES[(which, kind)]:
            if only and T not in only[0]:
                continue
            cvec = ct.ones_cvec(n, tw.c_total)
            ct.run_chain(tw, _stack_inputs(cfg, kind, n, H, W), cvec, emulate=True, ratios=ratios,
                         on_op=lambda o, src: ct.check_op(o, tw.eval(o, src, cvec), src(o["label"]), T, "emulation", None, stats))
            nops += len(tw.ops)
    print(ct.summary_line(f"emulation ae {which} {T}", stats, 0, time.time() - t0))
    print("   ratios:", {k: round(v, 3) for k, v in sorted(ratios.items())})
    print("   largest median E/half_ulp:", [(s["label"], round(s["median"], 3)) for s in sorted(stats, key=lambda s: -s["median"])[:3]])
    print("   decoder_conv:", [(round(s["worst"], 3), round(s["median"], 4)) for s in stats if s["label"] == "decoder_conv"])
    assert len(stats) == nops
    assert max(s["worst"] for s in stats) <= 1.0
    acc = ratios.get("acc32" if T == "fp32" else "acc", 0.0)
    assert 8 * acc <= (ct.C_ACC32 if T == "fp32" else ct.C_ACC) * 1.0001, ratios
    assert 4 * max(ratios.get("epi_emb", 0.0), ratios.get("epi_res", 0.0)) <= ct.C_EPI * 1.0001, ratios
    assert ratios.get("ss", 0.0) * 4 <= ct.C_SS, ratios
    if T != "fp32":
        assert max(s["median"] for s in stats) <= ct.MEDIAN_MAX


# ---------------------------------------------------------------------------------------------- (d) the checker has teeth on these graphs
N_BUG, IMG = 8, 5        # a batch of eight latents (the dihedral batch); the image-local bugs sit in one image of it


@pytest.fixture(scope="module")
def released_decoder():
    """the released decoder in bf16 on eight 5 x 7 latents (maps 5x7 .. 40x56), and its clean emulated chain"""
    cfg, seed = CONFIGS["released"]
    tw = _twin(cfg, A.synth_ae_state_dict(cfg, seed=seed), 2, "bf16")
    z = _stack_inputs(cfg, 2, N_BUG, 5, 7)
    cvec = ct.ones_cvec(N_BUG, tw.c_total)
    return tw, z, cvec, ct.run_chain(tw, z, cvec, emulate=True, ratios={})


def _ae_mutations():
    sa32 = ct.F32(ct.mp_concat_scales(128, 64, 0.5)[0])          # the scale a U-Net block of this width applies to the running tensor of a concat with a 64-channel skip

    def cout_not_one(c):                        # one cout's modulation value is 1 + 2^-8: the row every image shares is not the row of ones
        c = c.clone(); c[:, 37] = 1.0 + 2.0 ** -8; return c

    def tail_with_concat_scale(v, A_, Wt):      # the single 1x1 tail weighted kMixRes * sa as in a U-Net concat block: one 32-cout block of one 8 x 8 tile, every image
        v = v.clone(); v[:, 0:32, 0:8, 0:8] += ((sa32 - 1.0) * ct._conv(A_[1], Wt[1]))[:, 0:32, 0:8, 0:8]; return v

    def no_ones_channel(v, A_, Wt):             # decoder_conv's K loop stops in front of the ones channel (the last real one of the chunk): one cout of one image
        c1 = A_[0].shape[1] - 1
        v = v.clone(); v[IMG:IMG + 1, 40:41] -= ct._conv(A_[0][IMG:IMG + 1, c1:], Wt[0][40:41, c1:]); return v

    def neighbour_column(out):                  # rightmost column of the first 16-wide tile holds its left neighbour's values: that tile's rows, one image
        out = out.clone(); out[IMG, :, 0:16, 15] = out[IMG, :, 0:16, 14]; return out

    return {"modulation value 1 + 2^-8 on one cout": ("decoder.12.conv_res0", dict(c=cout_not_one)),
            "single tail weighted with a concat scale": ("decoder.14.conv_res1", dict(v=tail_with_concat_scale)),
            "decoder_conv without the ones channel": ("decoder_conv", dict(v=no_ones_channel)),
            "tile-edge column taken from its neighbour": ("decoder.15.conv_res1", dict(out=neighbour_column))}


@pytest.mark.parametrize("bug", list(_ae_mutations()))
def test_check_op_flags_autoencoder_kernel_bugs_the_whole_network_bound_lets_through(released_decoder, bug):
    """each bug is put into ONE op of the emulated decoder chain: `check_op` of that op on its own stored inputs fails, while the decoder's final output -- all eight
    images, as tests/test_autoencoder_gpu.py compares them -- stays within 2e-2 rel-RMS of the clean chain's.  Each is the size a wrong tile edge, K bound or weight
    slice has: the wrong modulation value reaches every image; the tail's wrong factor one 32-cout block of one tile; the lost ones channel one cout and the stale
    column one tile of ONE image of the batch (in every image of so small a map both would show in the whole-network figure: 1.6e-1 for 32 couts of the 5 x 7 map,
    3.2e-2 for the column at batch 1)."""
    tw, z, cvec, clean = released_decoder
    label, hook = _ae_mutations()[bug]
    o = tw.by_label[label]
    broken = ct.run_chain(tw, z, cvec, emulate=True, ratios={}, hooks={label: hook})
    src = lambda lab: broken.get(lab) if lab.startswith("sumsq:") else broken[lab]
    assert all(torch.equal(broken[s["src"]], clean[s["src"]]) for s in o["segs"]) and not torch.equal(broken[label], clean[label])
    r = tw.eval(o, src, cvec)
    assert ct.check_op(o, r, clean[label], "bf16", "emulation")["worst"] <= 1.0
    with pytest.raises(AssertionError) as ei:
        ct.check_op(o, r, broken[label], "bf16", "mutant")
    rr_op, rr_out = A.rel_rms(broken[label], clean[label]), A.rel_rms(broken["out_conv"], clean["out_conv"])
    print(f"{bug} ({label}): rel-RMS {rr_op:.2e} on the op's tensor, {rr_out:.2e} on the decoder's output -> {str(ei.value)[:220]}")
    assert label in str(ei.value) and "mutant" in str(ei.value) and "span c" in str(ei.value)
    assert 0.0 < rr_out < BOUNDS["bf16"], (bug, rr_out)
