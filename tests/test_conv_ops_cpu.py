"""CPU tests of the conv-op twin (tests/_conv_twin.py): (1) chained in float64 without any rounding it IS the reference network, so its segment
order, mul factors, concat scales and resampling are the reference's; (2) a float32 emulation of the same ops with the kernels' roundings passes
`check_op` with zero violations and yields the ratios the slack constants were fixed from; (3) `check_op` flags six kinds of kernel bug that the
whole-tensor 2e-2 rel-RMS bound lets through.

The accumulation slack counts S = `_conv_twin.acc_steps` roundings, one per tap per group of 16 (4) REAL channels.  It was K / 16 (K / 4) when the constants were fixed;
the two differ for the input conv alone (5 + 1 channels: 9 against 54 / 16), whose E_acc is therefore 1.63 x (fp32: 1.15 x) what the GPU arms first held it to -- a
loosening of that op's criterion that rests on the count and on this emulation only.  Ratios of (2) over S (torch 2.10 CPU): acc 1.99 (tiny bf16) / 1.84 (tiny fp16) /
2.07 (base bf16), acc32 1.74, against the recorded 2.26 / 1.74 over K / 16."""
import math
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_twin as ct
from conftest import rel_rms
from oracle import rng
from oracle.unet import BASE_CONFIG, DECODER_CONFIG, OracleUnet, synth_state_dict, tiny_config


def _inputs(cfg, n, H, W, seed=7):
    x = torch.from_numpy(rng.standard_normal(seed, (n, cfg["in_channels"], H, W)))
    cond = [torch.from_numpy(rng.standard_normal(seed + 1 + i, (n, c[1]))) for i, c in enumerate(cfg.get("conditional_inputs", []))]
    return x, torch.full((n,), 1.1), cond


CHAIN = {"tiny": (lambda: tiny_config(64, 1), 2, 32, 32), "tiny_attn": (lambda: tiny_config(64, 2, attn_resolutions=[128]), 2, 32, 32),
         "decoder": (lambda: dict(DECODER_CONFIG), 2, 24, 40), "base": (lambda: dict(BASE_CONFIG), 1, 64, 64)}


@pytest.mark.parametrize("which", list(CHAIN))
def test_twin_chained_in_float64_is_the_reference_network(which):
    mk, n, H, W = CHAIN[which]
    cfg = mk()
    sd = synth_state_dict(cfg, seed=1234)
    x, t, cond = _inputs(cfg, n, H, W)
    taps = {}
    y = OracleUnet(cfg, sd, dtype=torch.float64)(x, t, cond, taps=taps)
    tw = ct.Twin(cfg, sd, "exact")
    stored = ct.run_chain(tw, x, ct.oracle_cvec(cfg, sd, t, cond))
    worst = [("out_conv", rel_rms(stored["out_conv"], y))]
    plan = tw.by_label
    checked = 0
    for name, ref in taps.items():
        if name.endswith(".y1"):
            lab = name[:-3] + ".conv_res0"
        else:
            lab = name if name in plan else (name + ".attn_proj" if name + ".attn_proj" in plan else name + ".conv_res1")
        worst.append((lab, rel_rms(stored[lab], ref)))
        checked += 1
    w = max(worst, key=lambda p: p[1])
    print(f"{which}: {len(tw.ops)} ops, {checked} taps + the output; worst rel-RMS against OracleUnet(float64) {w[1]:.2e} at {w[0]}")
    assert checked == len(taps) and w[1] <= 1e-12, worst


def test_plan_op_counts():
    assert len(ct.describe(dict(BASE_CONFIG))[0]) == 79
    ops, c_total = ct.describe(tiny_config(64, 2, attn_resolutions=[128]))
    proj = [o for o in ops if o["label"].endswith(".attn_proj")]
    assert len(proj) > 0 and all(o["segs"][0]["src"] == o["label"][:-5] and o["segs"][0]["xform"] == 0 for o in proj)   # ordinary 1x1 convs of the stored "<block>.attn"
    assert not any("tier" in o for o in ops)                                                                          # no op with a looser criterion than the others
    assert all(o["K"] == sum(s["C"] * s["taps"] for s in o["segs"]) for o in ops)


def test_twin_folds_weights_bit_for_bit_like_the_host_that_feeds_the_engine():
    """the storage-type modes must start from the very fp32 numbers `EDMUnet2D.load_state_dict` hands over (fold = "reference"): one fp32 ulp on a weight is a
    16-bit rounding flip on some, and `check_op` sees single flips.  (`oracle.unet.fold_weight`, which the float64 chain test follows, differs by that ulp on
    e.g. enc.512x512_block0.conv_res1.)  Only the host-side static method is used: no GPU."""
    from terrain_diffusion_amd.unet import EDMUnet2D
    n = 0
    for cfg in (dict(BASE_CONFIG), dict(DECODER_CONFIG), tiny_config(64, 2, attn_resolutions=[128])):
        sd = synth_state_dict(cfg, seed=1234, out_gain=0.75)
        tw = ct.Twin(cfg, sd, "bf16")
        for name, w in tw.folded.items():
            gain = torch.as_tensor(sd["out_gain"]).to(torch.float32) if name == "out_conv.weight" else 1
            assert torch.equal(w, EDMUnet2D._fold_reference(torch.as_tensor(sd[name]).to(torch.float32), gain)), name
            n += 1
    assert n > 200


EMUL = [("tiny_attn", "bf16"), ("tiny_attn", "fp16"), ("tiny_attn", "fp32"), ("base32", "bf16")]
RATIOS = {}


@pytest.mark.parametrize("which,T", EMUL)
def test_float32_emulation_of_every_op_passes_check_op(which, T):
    """also the place where the slack constants come from (ratios printed; C_ACC = 8 x, C_EPI / C_PRO = 4 x the worst, see the module docstring) and where the
    median condition E / half_ulp <= 0.5 is checked without a GPU"""
    cfg = dict(BASE_CONFIG) if which == "base32" else tiny_config(64, 2, attn_resolutions=[128])
    n = 1 if which == "base32" else 2
    sd = synth_state_dict(cfg, seed=1234)
    x, t, cond = _inputs(cfg, n, 32, 32)
    cvec = ct.oracle_cvec(cfg, sd, t, cond, dtype=torch.float32)
    tw = ct.Twin(cfg, sd, T)
    ratios, stats = {}, []

    def on_op(o, src):
        ct.check_op(o, tw.eval(o, src, cvec), src(o["label"]), T, "emulation", None, stats)

    t0 = time.time()
    ct.run_chain(tw, x, cvec, emulate=True, ratios=ratios, on_op=on_op)
    RATIOS[(which, T)] = ratios
    print(ct.summary_line(f"emulation {which} {T}", stats, 0, time.time() - t0))
    print("   ratios:", {k: round(v, 3) for k, v in sorted(ratios.items())})
    top = sorted(stats, key=lambda s: -s["median"])[:3]
    print("   largest median E/half_ulp:", [(s["label"], round(s["median"], 3)) for s in top])
    assert len(stats) == len(tw.ops)
    assert max(s["worst"] for s in stats) <= 1.0
    # the fixed constants keep their stated margins over what the emulation shows
    acc = ratios.get("acc32" if T == "fp32" else "acc", 0.0)
    assert 8 * acc <= (ct.C_ACC32 if T == "fp32" else ct.C_ACC) * 1.0001, ratios
    assert 4 * max(ratios.get("epi_emb", 0.0), ratios.get("epi_res", 0.0)) <= ct.C_EPI * 1.0001, ratios
    assert ratios.get("ss", 0.0) * 4 <= ct.C_SS, ratios


# ---------------------------------------------------------------------------------------------- the checker has teeth
def _standalone(tw, label, H, W, seed):
    """synthetic stored inputs of one base-model op (normal, rms 2, rounded to the storage type) and its modulation row"""
    o = tw.by_label[label]
    g = torch.Generator().manual_seed(seed)
    stored = {}
    for lab, C, rs in [(s["src"], s["C"], s["resample"]) for s in o["segs"]] + ([(o["res"]["src"], o["res"]["C"], o["res"]["resample"])] if o["res"] else []):
        if lab not in stored:
            stored[lab] = ct.rne(2.0 * torch.randn((1, C, H, W), generator=g, dtype=torch.float64), tw.mode)
    cvec = 1.0 + 0.3 * torch.randn((1, tw.c_total), generator=g, dtype=torch.float32)
    return o, stored, cvec


@pytest.fixture(scope="module")
def base_twin():
    cfg = dict(BASE_CONFIG)
    return ct.Twin(cfg, synth_state_dict(cfg, seed=1234), "bf16")


# (op with a modulated-silu epilogue, op with a normed residual) on a 192-channel and on a 768-channel level; 40 x 40 and 18 x 18 maps: 16 x 16 tiles hang over
BATCH_PIXELS = {"K=192*9": 64 * 64, "K=768*9": 8 * 8}   # pixels per image of that level in the 64 x 64-window bench batch
LAYERS = {"K=192*9": ("enc.512x512_block0", 40), "K=768*9": ("enc.64x64_block1", 18)}


def _mutations(H):
    x0 = 15                                     # rightmost column of the first 16 x 16 tile
    def drop_tap(v, A, Wt):                     # tap (ky, kx) = (1, 2) of every channel missing for that column, couts of one 32-block
        v = v.clone(); a = torch.nn.functional.pad(A[0], (1, 1, 1, 1))
        v[:, 0:32, 0:16, x0] -= torch.einsum("oc,nch->noh", Wt[0][0:32, :, 1, 2], a[:, :, 1:17, x0 + 2])
        return v
    def drop_kstep(v, A, Wt):                   # channels 16..31 of every tap missing for couts 32..63 of the first tile
        v = v.clone()
        v[:, 32:64, 0:16, 0:16] -= ct._conv(A[0][:, 16:32], Wt[0][32:64, 16:32])[:, :, 0:16, 0:16]
        return v
    def stale_row(out):                         # last row of the ragged tile keeps what the tile before it wrote
        out = out.clone(); out[:, :, H - 1, 0:16] = out[:, :, H - 17, 0:16]; return out
    def shift_c(c):                             # modulation row of cout block 32..63 read four couts too far
        c = c.clone(); c[:, 32:64] = c[:, 36:68].clone(); return c
    def bias(out):                              # one 32 px x 32 cout MFMA block rounded up instead of to nearest
        out = out.clone(); blk = out[:, 0:32, 0:2, 0:16] + 0.0; out[:, 0:32, 0:2, 0:16] = blk + ct.ulp(blk, "bf16"); return out
    return {"tap dropped in a tile's rightmost column": dict(v=drop_tap), "16-channel K-step dropped for one 32-cout block": dict(v=drop_kstep),
            "stale last row of a ragged tile": dict(out=stale_row), "modulation row shifted by 4 couts": dict(c=shift_c),
            "one-ulp upward bias on one 32 x 32 block": dict(out=bias), "residual scale applied without rn": dict(no_rn=True)}


@pytest.mark.parametrize("layer", list(LAYERS))
def test_check_op_flags_kernel_bugs_the_whole_tensor_bound_lets_through(base_twin, layer):
    """Each mutation of an emulated output must be flagged.  Printed with each is the rel-RMS it causes on the tensor OF THE OP ITSELF in the 64-window batch the
    suite's 2e-2 whole-tensor bound is applied to (mutations of one tile: the rel-RMS on this test's one small map scaled by sqrt(pixels here / pixels of that
    level in the batch); the modulation shift and the missing rn hit every pixel of every image and are not scaled).  The dropped tap, the dropped K-step and the
    one-ulp bias stay under 2e-2 on both layers (asserted), so does the stale row at the 192-channel level: they pass unseen even before the layers behind the op
    dilute them.  The modulation shift (1.8e-2 ... 8e-2 at op level, 32 of 192 / 768 couts) and the stale row on an 18 x 18 map are visible at op level and
    rely on that dilution; a residual added without rn is wrong everywhere (rel-RMS 0.8) and is listed for the message it produces."""
    tw = base_twin
    block, H = LAYERS[layer]
    seen = set()
    for suffix in (".conv_res0", ".conv_res1"):
        o, stored, cvec = _standalone(tw, block + suffix, H, H, seed=len(block))
        src = lambda lab: stored.get(lab) if lab.startswith("sumsq:") else stored[lab]
        clean = tw.emulate(o, src, cvec, {})
        r = tw.eval(o, src, cvec)
        assert ct.check_op(o, r, clean, "bf16", "emulation")["worst"] <= 1.0
        for name, hook in _mutations(H).items():
            if ("c" in hook and o["epi"] != "emb") or ("no_rn" in hook and not (o["res"] and o["res"]["norm"])):
                continue
            bad = tw.emulate(o, src, cvec, {}, hook=hook)
            assert not torch.equal(bad, clean)
            rr = rel_rms(bad, clean) * (1.0 if ("no_rn" in hook or "c" in hook) else math.sqrt(H * H / (64.0 * BATCH_PIXELS[layer])))
            with pytest.raises(AssertionError) as ei:
                ct.check_op(o, r, bad, "bf16", "mutant")
            print(f"{layer} {o['label']}: {name}: op-level rel-RMS in a 64-window batch {rr:.2e} -> {str(ei.value)[:230]}")
            assert o["label"] in str(ei.value) and "mutant" in str(ei.value) and "span c" in str(ei.value)
            if "v" in hook or name.startswith("one-ulp"):
                assert rr < 2e-2, (name, rr)     # invisible to the bound the suite had
            seen.add(name)
    assert seen == set(_mutations(H))


def test_ulp_and_rounding_helpers():
    x = torch.tensor([1.0, 1.5, 1.9999, 2.0, 3e-6, 0.0, -260.0], dtype=torch.float64)
    assert ct.ulp(x, "bf16").tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -26, 2.0 ** -133, 2.0]
    assert ct.ulp(x, "fp16").tolist()[:5] == [2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24]
    assert ct.flavour_of("enc.512x512_conv [64x64 k1 f2w bn96 wg384 ks1 gf5.44 mb1.00 mbs1.00]") == ("enc.512x512_conv", "f2w", 1)
    assert ct.flavour_of("dec.64x64_in0.attn_qkv [8x8 k12 f4m2n1 bn128 wg72 ks3 gf0.1 mb1.0 mbs1.0]")[1:] == ("f4m2n1", 3)
    assert ct.flavour_of("a [8x8 k12 f0 bn128 wg72 ks3 gf0.1 mb1.0 mbs1.0]")[1] == "f0"
    assert abs(ct.KMIX_RES64 - 0.7 / math.sqrt(0.58)) < 1e-15
