"""The attention twin and its criterion (tests/_attn_twin.py) on the CPU: the float32 / bf16 emulation of the flash kernel passes conditions A, B and C on every input
family and head-dim class with zero violations (the ratios the constants rest on are printed and pinned); deliberately broken emulations are caught; the selector
inputs are honest; the operand restatement equals RNE_bf16 of the float64 operand except on flagged elements."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_twin as at

# one head dim per (Dp / 16, Dm / 32, folded) class of the dispatcher -- all 20 -- plus odd ones
CLASS_DIMS = [8, 24, 40, 56, 72, 88, 104, 120, 136, 152, 16, 32, 48, 64, 80, 96, 112, 128, 144, 160]
ODD_DIMS = [1, 2, 3, 5, 17, 41, 77]
MOVING = ("shift-300", "shift+250", "spread40", "late", "early")


def _run(kind, B, H, Lq, Lk, D, normalize=False, mutate=None, ratios=None):
    case = at.make_case(kind, B, H, Lq, Lk, D, seed=D * 7 + Lk, normalize=normalize)
    ref = at.reference(at.pack_operands(case), D, normalize)
    out = at.emulate(case, mutate=mutate, ratios=ratios)
    return case, ref, out, f"{kind} {B}x{H} {Lq}x{case['k'].shape[2]} d{D}{' norm' if normalize else ''}{' ' + mutate if mutate else ''}"


def test_formula_selection_matches_the_head_dim():
    classes = {(at.dp_of(D) // 16, (D + 31) // 32, at.fold_of(D)) for D in range(1, 161)}
    assert len(classes) == 20 and classes == {(at.dp_of(D) // 16, (D + 31) // 32, at.fold_of(D)) for D in CLASS_DIMS}
    for D in range(1, 161):
        assert at.fold_of(D) == (D % 16 != 0)
    # the folded bound is the one built on |V - o|: it vanishes on a one-hot softmax where the plain one does not
    for D, small in ((40, True), (64, False)):
        case = at.make_case("selector", 1, 1, 70, 150, D, seed=1)
        ref = at.reference(at.pack_operands(case), D)
        assert (float((ref["Bp"] / ref["o"].abs()).max()) < 1e-6) == small
        if not small:
            assert abs(float((ref["Bp"] / ref["o"].abs()).median()) - at.UB) < 1e-6


def test_emulation_passes_every_condition_and_pins_the_constants():
    ratios, rms, mx = {}, [], []
    cases = [("random", 1, 2, 70, 150, D, False) for D in CLASS_DIMS + ODD_DIMS]
    cases += [("random", 1, 2, 70, 150, 64, True), ("random", 1, 2, 70, 150, 40, True), ("random", 2, 2, 96, 1000, 64, False), ("random", 1, 1, 128, 4096, 40, False),
              ("random", 1, 2, 256, 256, 160, False), ("random", 1, 3, 64, 64, 64, True)]
    cases += [(kind, 1, 2, 100, 330, D, False) for kind in MOVING for D in (40, 41, 64, 128)]
    for kind, B, H, Lq, Lk, D, norm in cases:
        case, ref, out, name = _run(kind, B, H, Lq, Lk, D, norm, ratios=ratios)
        st = at.check(out, ref, "fp32", name, stat=True)
        print(at.line(st))
        if kind == "random":
            rms.append(st["rms_z"]); mx.append(st["max_z"] - math.sqrt(2.0 * math.log(st["n"])))
    print(f"emulation: logit accumulation ratio {ratios['acc_s']:.3f} (x 8 <= C_S = {at.C_S}), PV / denominator ratio {ratios['acc_pv']:.3f} (x 8 <= C_PV = {at.C_PV}), "
          f"rms(z) on random inputs {min(rms):.3f} .. {max(rms):.3f} (x 1.25 <= Z_RMS = {at.Z_RMS}), worst max(z) - sqrt(2 ln N) = {max(mx):+.2f} (margin {at.Z_MAX_MARGIN})")
    assert 8.0 * ratios["acc_s"] <= at.C_S and 8.0 * ratios["acc_pv"] <= at.C_PV
    assert 1.25 * max(rms) <= at.Z_RMS and min(rms) >= 0.6          # neither too tight nor so loose that a rounding-sized error could hide
    assert max(mx) <= 1.0


def test_emulation_of_the_engine_path_rounds_to_bf16():
    case, ref, _, name = _run("random", 2, 2, 64, 64, 64, True)
    out = at.emulate(case, out_T="bf16")
    print(at.line(at.check(out, ref, "bf16", name + " bf16 out", stat=True)))


@pytest.mark.parametrize("D", CLASS_DIMS + ODD_DIMS)
def test_selector_inputs_are_honest_and_pass(D):
    case, ref, out, name = _run("selector", 1, 2, 70, 150, D)
    Lk = case["k"].shape[2]
    bound = at.selector_honesty(case, ref, full=70 >= min(64, Lk) + 3)
    st = at.check(out, ref, "fp32", name, stat=False)
    # a one-hot row: B_p vanishes in the folded form and is u_b |o| in the plain form; what remains is the fp32 side (half an ulp, the PV sum, the final multiply)
    fp32_side = at.U * (1.0 + 3.0 + at.C_PV * math.sqrt((Lk + 15) // 16 + (Lk + 63) // 64)) * 1.05
    assert bound <= fp32_side + (0.0 if at.fold_of(D) else at.UB), (bound, fp32_side)
    print(at.line(st) + f"   largest bound / |o| {bound:.2e}")


@pytest.mark.parametrize("mutate,D", [("wrong_row_den", 40), ("wrong_row_den", 88), ("leaked_key", 64), ("leaked_key", 32), ("swapped_keys", 40), ("swapped_keys", 64),
                                      ("dropped_block", 40), ("dropped_block", 64), ("dropped_block", 8), ("dropped_block", 160)])
def test_every_mutation_breaks_condition_a_on_the_selector_inputs(mutate, D):
    """(wrong_row_den: folded head dims.  In the plain form every row of a one-hot softmax has the denominator 1.0 exactly, so a neighbour's is the same number: that
    mutation is the random family's to catch, below.  leaked_key: plain head dims, see the module docstring of the twin.)"""
    case, ref, out, name = _run("selector", 1, 2, 70, 150, D, mutate=mutate)
    st, bad, ratio, _ = at.measure(out, ref, "fp32", name)
    print(at.line(st))
    assert st["bad"] > 0 and st["worstA"] > 4.0
    with pytest.raises(AssertionError):
        at.check(out, ref, "fp32", name, stat=False)
    if mutate == "leaked_key":      # the query that targets key Lk - 1 loses half of its weight to the leaked copy
        assert bool(bad[:, :, 0].all()) and float((out[:, :, 0] / ref["o"][:, :, 0]).max()) <= 0.5 + 1e-6


@pytest.mark.parametrize("D", [64, 40, 128])
def test_mutations_on_random_inputs(D):
    which = {}
    for mutate in ("wrong_row_den", "leaked_key", "swapped_keys", "dropped_block"):
        if mutate == "leaked_key" and at.fold_of(D):
            continue
        case, ref, out, name = _run("random", 1, 2, 96, 1000 if mutate != "leaked_key" else 77, D, mutate=mutate)
        st, _, _, _ = at.measure(out, ref, "fp32", name)
        broke = [c for c, hit in (("A", st["bad"] > 0), ("B", st["rms_z"] > at.Z_RMS), ("C", st["max_z"] > st["z_max"])) if hit]
        which[mutate] = broke
        print(f"{name}: breaks {', '.join(broke) or 'nothing'}   ({st['bad']} elements outside A, rms(z) {st['rms_z']:.1f}, max(z) {st['max_z']:.1f})")
        if mutate in ("wrong_row_den", "leaked_key"):
            assert "A" in broke and "B" in broke, (mutate, broke)
        else:
            assert broke, mutate


def test_a_dropped_light_key_is_beyond_the_criterion_on_diffuse_inputs():
    """why the selector family exists: on a diffuse softmax a lost key is seen only by the queries that gave it weight; where it is light, B_p alone is larger"""
    case = at.make_case("random", 1, 1, 64, 1000, 64, seed=5)
    ops = at.pack_operands(case)
    ref = at.reference(ops, 64)
    w = torch.softmax(at.LN2 * (ops["Q"] @ ops["K"].transpose(-1, -2)), -1)
    keep = [j for j in range(1000) if j != 500]
    less = dict(case, k=case["k"][:, :, keep].contiguous(), v=case["v"][:, :, keep].contiguous())
    st, bad, _, _ = at.measure(at.emulate(less), ref, "fp32", "random 64x1000 d64 without key 500")
    w500 = w[0, 0, :, 500]
    hit = bad[0, 0].any(-1)
    print(f"weight of key 500: median {float(w500.median()):.1e}, max {float(w500.max()):.1e}; condition A sees the loss on {int(hit.sum())} of 64 queries, "
          f"the lightest of them with weight {float(w500[hit].min()) if bool(hit.any()) else float('nan'):.1e}; " + at.line(st))
    assert not bool(hit.all())                                               # queries on which the key is light enough go unnoticed ...
    assert not bool(hit.any()) or float(w500[hit].min()) > float(w500[~hit].median())   # ... the heavy ones do not


@pytest.mark.parametrize("D", [1, 7, 40, 64, 65, 129, 160])
def test_operand_restatement(D):
    for normalize in (False, True):
        case = at.make_case("random", 2, 2, 50, 90, D, seed=D, normalize=normalize)
        ops = at.pack_operands(case)
        nflag, n = 0, 0
        for N in "QKV":
            same = ops[N] == at.rne(ops[N + "64"], "bf16")
            flagged = ops["F" + N] > 0
            assert bool((same | flagged).all()), (N, D, normalize)
            if not normalize:
                assert bool(same.all()) and not bool(flagged.any())
            else:   # a flagged operand lies within one bf16 ulp of the float64 rounding
                assert bool(((ops[N] - at.rne(ops[N + "64"], "bf16")).abs() <= ops["F" + N]).all())
            nflag += int(flagged.sum()); n += flagged.numel()
        if normalize:
            print(f"d{D}: {nflag} of {n} operands flagged ({100.0 * nflag / n:.3f} %)")
            assert nflag / n < 5e-3
    f = torch.tensor(at.pow2_scale(), dtype=torch.float32) * torch.tensor(at.LOG2E32, dtype=torch.float32)
    assert float(f) == 0.5


def test_scalar_kernel_twin_against_a_float32_restatement():
    """the scalar kernel's bound B_sc on an fp32 restatement of its loops (sequential sums), fp32 output: condition A, and not by a wide margin only"""
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, 2, 64, 64, generator=g) * s for s in (1.3, 0.9, 2.0))
    ref = at.scalar_reference(q, k, v)
    f32 = torch.float32
    def nrm(x, extra=1.0):
        s = torch.zeros(x.shape[:-1], dtype=f32)
        for c in range(64):
            s = s + x[..., c] * x[..., c]
        inv = 1.0 / (torch.tensor(1e-4, dtype=f32) + torch.sqrt(s) * 0.125)
        return x * (inv * extra)[..., None]
    qn, kn, vn = nrm(q), nrm(k, 0.125), nrm(v)
    s = torch.zeros(2, 2, 64, 64, dtype=f32)
    for c in range(64):
        s = s + qn[..., :, None, c] * kn[..., None, :, c]
    e = torch.exp(s - s.amax(-1, keepdim=True))
    den = e.sum(-1)
    o = torch.zeros(2, 2, 64, 64, dtype=f32)
    for j in range(64):
        o = o + e[..., :, j, None] * vn[..., None, j, :]
    out = o * (1.0 / den)[..., None]
    st = at.check(out.double(), ref, "fp32", "scalar restatement", stat=False)
    print(at.line(st))
    assert st["worstA"] > 1e-3
    for T in ("bf16", "fp16"):
        at.check(at.rne(out.double(), T), ref, T, "scalar restatement " + T, stat=False)
    bad = out.clone(); bad[0, 0, 5] = out[0, 0, 6]
    with pytest.raises(AssertionError):
        at.check(bad.double(), ref, "fp32", "scalar, wrong row", stat=False)
