"""The embedding / modulation twin and its criterion (tests/_emb_twin.py) on the CPU: the float32 emulation of emb_kernel, cvec_kernel, cvec_mfma_kernel and
cvec_norm_kernel passes condition A, the cap and the honesty condition on every case of the GPU test (the ratios that condition B's constants rest on are printed
and the constants asserted against them); the twin's float64 rows are the project's oracle's; deliberately broken emulations are caught."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_twin as ct
import _emb_twin as et

U = et.U


def _case(name):
    for nm, kind, n, kw in et.gpu_cases():
        if nm == name:
            return et.make_case(nm, kind, n, kw)
    raise KeyError(name)


def test_the_dispatch_rule_covers_all_three_arms():
    arms = {}
    for nm, kind, n, kw in et.gpu_cases():
        arms.setdefault(et.arm_of(et.tiny_config(64, 1, **kw)), []).append((nm, n if kind != "forward" else n * n))
    assert set(arms) == {"<4>", "<1>", "scalar"}
    for a, cs in arms.items():
        assert any(rows == 289 for _, rows in cs), f"no 289-row case on arm {a}"
    assert et.arm_of(et.tiny_config(64, 1)) == "<4>" and et.arm_of(et.tiny_config(64, 1, emb_channels=768)) == "<4>"
    assert et.arm_of(et.tiny_config(64, 1, emb_channels=80)) == "<1>" and et.arm_of(et.tiny_config(64, 1, emb_channels=16)) == "<1>"
    assert et.arm_of(et.tiny_config(64, 1, emb_channels=100)) == "scalar" and et.arm_of(et.tiny_config(64, 1, emb_channels=37)) == "scalar"
    couts = {b["cout"] for b in et.operands(et.tiny_config(64, 1), et.synth_state_dict(et.tiny_config(64, 1), seed=77))["blocks"]}
    assert couts == {64, 128, 192, 256}


def test_row_layout():
    s, t = et.row_index(5, 3)
    assert s.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4] and t.tolist() == [0, 1, 2] * 5
    s, t = et.row_index(3, 3, diagonal=True)
    assert list(zip(s.tolist(), t.tolist())) == [(0, 0), (1, 1), (2, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]


def test_emulation_passes_every_condition_and_pins_the_constants():
    worst = dict(emb_rms=0.0, cvec_rms=0.0, emb_worst=0.0, cvec_worst=0.0)
    med = dict(emb=[], cvec=[])
    for nm, kind, n, kw in et.gpu_cases():
        case = et.make_case(nm, kind, n, kw)
        emb, cv = et.emulate(case)
        st = et.check(case, emb, cv)
        print(et.line(st) + f"; honesty emb {st['emb_honest']:.0f} E, cvec {st['cvec_honest']:.0f} E")
        for k in worst:
            worst[k] = max(worst[k], st[k])
        med["emb"].append(st["emb_median"] / U); med["cvec"].append(st["cvec_median"] / U)
    print(f"emulation: rms(emb - ref) / rms(ref) worst {worst['emb_rms'] / U:.2f} u (x 4 = {4 * worst['emb_rms'] / U:.2f} u, C_RMS_EMB = {et.C_RMS_EMB / U:.2f} u); "
          f"rms(cvec - ref) / rms(ref) worst {worst['cvec_rms'] / U:.2f} u (x 4 = {4 * worst['cvec_rms'] / U:.2f} u, C_RMS_CVEC = {et.C_RMS_CVEC / U:.2f} u); "
          f"worst |err| / E emb {worst['emb_worst']:.2f}, cvec {worst['cvec_worst']:.2f}; median E / (u |ref|) emb {min(med['emb']):.0f} .. {max(med['emb']):.0f}, "
          f"cvec (largest block) {min(med['cvec']):.0f} .. {max(med['cvec']):.0f}")
    # the constants ARE 4 x the emulation's worst (rounded up by at most 5 %)
    assert 4.0 * worst["emb_rms"] <= et.C_RMS_EMB <= 4.2 * worst["emb_rms"]
    assert 4.0 * worst["cvec_rms"] <= et.C_RMS_CVEC <= 4.2 * worst["cvec_rms"]
    assert worst["emb_worst"] < 0.5 and worst["cvec_worst"] < 0.5                   # the fp32 restatement stays well inside the worst-case bound


def _fold_host_as_oracle(w, gain=1.0):
    return ct.fold_host(torch.as_tensor(w), 1 if gain == 1.0 else torch.tensor(gain, dtype=torch.float32))


@pytest.mark.parametrize("which", ["tiny", "coarse", "mixed"])
def test_twin_is_the_oracle_in_float64(which, monkeypatch):
    """The twin's float64 rows against OracleUnet(dtype=float64).embeddings and _conv_twin.oracle_cvec, 1e-12 relative.  Where they legitimately differ, both are given
    the same numbers: (1) OracleUnet folds with oracle.unet.fold_weight, the engine is handed fold_host's weights (one fp32 ulp apart on the norm of some tensors): the
    oracle is built on fold_host here; (2) the oracle takes the input weights and 1 / ||(1, w)|| in double, the engine holds fp32 values: the config carries the
    fp32 weights and the twin gets the double norm; (3) the oracle takes sin / cos of the fp32 argument IN fp32 whatever its dtype: the twin does the same here (trig =
    float32); with its own float64 sin / cos it stays within 1e-6."""
    import oracle.unet as ou
    monkeypatch.setattr(ou, "fold_weight", _fold_host_as_oracle)
    cfg = {"tiny": et.tiny_config(64, 1), "coarse": dict(ou.COARSE_CONFIG), "mixed": et.tiny_config(64, 1, emb_channels=80, conditional_inputs=et.MIXED8)}[which]
    cfg["conditional_inputs"] = [[typ, dim, float(torch.tensor(float(w), dtype=torch.float32))] for typ, dim, w in cfg["conditional_inputs"]]
    case = et.make_case(which, "forward", 5, cfg=cfg)
    ops = et.operands(cfg, case["sd"])
    ops64 = dict(ops, inv_norm=1.0 / math.sqrt(1.0 + sum(c["weight"] ** 2 for c in ops["conds"])))
    step, tile = case["step"], case["tile"]
    orc = ou.OracleUnet(cfg, case["sd"], dtype=torch.float64)
    t_rows, cond_rows = case["t"][step], [c[tile] for c in case["cond"]]
    o_emb = orc.embeddings(t_rows, cond_rows)
    emb, _ = et.embedding(ops64, case["t"], case["cond"], step, tile, trig=torch.float32)
    rel = float((emb - o_emb).abs().max() / o_emb.abs().max())
    emb64, _ = et.embedding(ops, case["t"], case["cond"], step, tile)
    rel64 = float((emb64 - o_emb).abs().max() / o_emb.abs().max())
    o_cv = ct.oracle_cvec(cfg, case["sd"], t_rows, cond_rows, dtype=torch.float64)
    cv, _ = et.modulation(ops, o_emb)
    relc = float((cv - o_cv).abs().max() / o_cv.abs().max())
    print(f"{which}: twin - oracle, embedding rows {rel:.1e} (twin's own float64 sin / cos and fp32 norm: {rel64:.1e}), modulation rows {relc:.1e}")
    assert rel <= 1e-12 and relc <= 1e-12 and rel64 <= 1e-6


# mutation -> (cases it is judged on, the tensor that must break)
MUTANTS = {
    "tile_step_layout": (["forward n9 emb256 tensor58", "edm 5 steps N3 emb256 tensor58"], "emb"),
    "clamped_row": (["forward n9 emb256 tensor58", "forward n9 emb80 mixed8", "forward n17 emb768 tensor58"], "cvec"),
    "k_order": (["forward n9 emb256 tensor58", "forward n9 emb80 mixed8", "forward n9 emb16 noise200"], "cvec"),
    "dropped_group": (["forward n9 emb256 tensor58", "forward n9 emb80 mixed8", "forward n9 emb16 noise200"], "cvec"),
    "no_plus1": (["forward n9 emb256 tensor58", "forward n9 emb100 5 floats"], "cvec"),
    "norm_neighbour": (["forward n9 emb256 tensor58", "forward n9 emb100 5 floats"], "cvec"),
    "norm_ctotal": (["forward n9 emb256 tensor58"], "cvec"),
    "silu_on_float": (["forward n9 emb80 mixed8", "forward n9 emb256 5 floats"], "emb"),
    "no_silu_on_tensor": (["forward n9 emb80 mixed8", "forward n9 emb256 tensor58"], "emb"),
    "inv_norm_ignores_weights": (["forward n9 emb80 mixed8", "forward n9 emb256 5 floats"], "emb"),
    "sincos_swapped": (["forward n9 emb256 tensor58", "forward n9 emb37 no cond noise6"], "emb"),
    "xoff_dims": (["forward n9 emb80 mixed8", "forward n9 emb256 5 floats"], "emb"),
    "no_diag_copy": (["forward n9 emb256 tensor58", "forward n9 emb256 no cond"], "emb"),
}


@pytest.mark.parametrize("mutate", list(MUTANTS))
def test_every_mutation_breaks_condition_a(mutate):
    """Each deliberately broken emulation misses condition A by a factor >= 10 on the stated inputs.  The modulation rows are judged against the twin evaluated on the
    rows the (broken) emulation stored, so an embedding mutant breaks the embedding rows and ONLY those: the ops do not hide behind each other.
    Limits, by construction: `clamped_row`, `k_order` and `dropped_group` are properties of the matrix-core kernel and have no meaning on the scalar arm; a model without conditional
    inputs has the same row for every tile, so no case of it can see a wrong tile (its `no_diag_copy` is seen through the step alone)."""
    cases, what = MUTANTS[mutate]
    assert set(MUTANTS) == set(et.MUTATIONS)
    for name in cases:
        case = _case(name)
        if mutate in ("clamped_row", "k_order", "dropped_group"):
            assert et.arm_of(case["cfg"]) != "scalar"
        emb, cv = et.emulate(case, mutate=mutate)
        r = et.reference(case, emb.double())
        me, bad_e, _ = et.measure(emb.double(), r["emb"], r["E_emb"])
        mc, bad_c, _ = et.measure(cv.double(), r["cvec"], r["E_cvec"])
        print(f"{mutate} on {name}: emb worst err / E {me['worst']:.3g} ({me['nbad']} elements out), cvec {mc['worst']:.3g} ({mc['nbad']} out)")
        assert (me if what == "emb" else mc)["worst"] >= 10.0, (mutate, name)
        with pytest.raises(AssertionError):
            et.check(case, emb, cv, honesty=False)
        if what == "emb" and mutate not in ("tile_step_layout", "no_diag_copy"):     # (those two move whole rows: both tensors sit in the wrong place)
            assert mc["nbad"] == 0, "the modulation rows follow the stored embedding rows"
        if mutate == "clamped_row":                                                  # exactly one row is wrong
            assert bad_c.any(1).sum() == 1 and me["nbad"] == 0
        if mutate == "no_diag_copy":                                                 # rows 1 .. n - 1, nothing else
            n = case["n"]
            assert bool(bad_e[1:n].any(1).all()) and not bool(bad_e[n:].any()) and not bool(bad_e[0].any())


def test_one_wrong_element_and_one_wrong_slice_are_seen():
    """what the aggregate check could not see: one element of the 2 x 256 it read off by 1e-4 (its relative RMS, 5e-6, passes that), and one 16-cout slice of one block
    taken from the row below"""
    case = _case("forward n9 emb256 tensor58")
    emb, cv = et.emulate(case)
    e2 = emb.clone(); e2[1, 100] += 1e-4
    assert float(torch.sqrt(((e2 - emb) ** 2)[:2].mean()) / torch.sqrt((emb ** 2)[:2].mean())) < 5e-6
    with pytest.raises(AssertionError, match="row 1 "):
        et.check(case, e2, cv, honesty=False)
    c2 = cv.clone(); c2[70, 1024 + 16:1024 + 32] = cv[71, 1024 + 16:1024 + 32]
    with pytest.raises(AssertionError, match="row 70 "):
        et.check(case, emb, c2, honesty=False)
