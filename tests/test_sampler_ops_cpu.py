"""CPU: the criterion of tests/_sampler_twin.py bites, and its float64 twin is the reference's scheduler.

* the float64 step twin, chained without rounding, reproduces the traces of the reference scheduler (tests/golden/schedule.npz, schedule3.npz) at the tolerance
  oracle/schedule.py is held to;
* the engine's coefficient table (td_dpm_coefs: the host function the sampler itself calls, no GPU needed) against the float64 restatement, which is pinned to
  oracle/schedule.py;
* a numpy fp32 emulation of dpm_update / the sampler's buffers passes A, B, the cap and every exact hand-off, and sets C_RMS_STEP;
* every broken emulation violates A or an exact hand-off; the miss factor is printed."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_twin as tw
from conftest import rel_rms
from oracle import rng, schedule

U = tw.U
SD = 0.5


def _ladder(n):
    return schedule.karras_sigmas(n)[0].numpy()


def _c_in0(sig):
    s, sd = np.float32(sig[0]), np.float32(SD)
    return np.float32(1.0) / np.sqrt(s * s + sd * sd)


# ------------------------------------------------------------------------------------------------------------------ the twin is the reference's
def test_float64_twin_reproduces_the_pinned_scheduler(golden):
    def model(xin, i, sig):
        return np.tanh(0.3 * xin) - 0.2 * math.cos(math.atan(float(sig[i]) / SD))
    cases = [("schedule", f"trace_{n}", 2, n, 900 + n) for n in (4, 12, 20, 32)] + [("schedule3", f"trace_order{o}_{n}", o, n, 950 + n) for o in (3, 1) for n in (6, 20)]
    worst = 0.0
    for file, key, order, n, seed in cases:
        sig = _ladder(n)
        x0 = rng.standard_normal(seed, (2, 5, 8, 8)).astype(np.float64) * float(sig[0])
        xs = tw.chain_float64(sig, schedule.solver_orders(n, solver_order=order), x0, lambda xin, i: model(xin, i, sig), SD)
        for i, x in enumerate(xs):
            err = rel_rms(x, golden(file)[key][i])
            worst = max(worst, err)
            assert err < 2e-6, (key, i, err)
    print(f"float64 twin against the reference scheduler's traces: worst relative RMS {worst:.2e} (< 2e-6)")


# ------------------------------------------------------------------------------------------------------------------ the coefficient table
TABLE_CASES = [(o, lof, n) for o in (1, 2, 3) for lof in (0, 1) for n in (1, 2, 3, 6, 14, 15, 20)]


def test_float64_coefficients_are_those_of_the_oracle_scheduler():
    """the restatement against oracle/schedule.py (fp32 torch scalars in the reference's order), within the tolerance it grants an fp32 evaluation"""
    for o, lof, n in TABLE_CASES:
        sig = schedule.karras_sigmas(n)[0]
        ref = tw.coef_ref(sig.numpy(), SD, o, bool(lof))
        orders = schedule.solver_orders(n, solver_order=o, lower_order_final=bool(lof))
        assert [int(v) for v in ref["val"][:, tw.FIELDS.index("order")]] == orders
        tab = np.zeros((n, len(tw.FIELDS)), np.float32)
        for i in range(n):
            a, b0, inv_r0, third = schedule.step_coefficients(sig, i, orders[i])
            r = dict.fromkeys(tw.FIELDS, 0.0)
            r.update(a=float(a), b0=float(b0), order=orders[i], last=float(i == n - 1), inv_r0=float(inv_r0) if inv_r0 is not None else 0.0)
            if third is not None:
                r.update(zip(("inv_r1", "f01", "inv_r01", "c1", "c2"), (float(v) for v in third)))
            s = sig[i]
            r["c_skip"] = float(SD ** 2 / (s ** 2 + SD ** 2))
            r["c_out"] = float(s * SD / (s ** 2 + SD ** 2) ** 0.5)
            r["c_in_next"] = 0.0 if i == n - 1 else float(1 / ((sig[i + 1] ** 2 + SD ** 2) ** 0.5))
            tab[i] = [r[f] for f in tw.FIELDS]
        worst, bad = tw.check_table(tab, ref)
        assert not bad and max(worst.values()) <= 1.0, (o, lof, n, worst, bad)


@pytest.mark.parametrize("o,lof,n", TABLE_CASES)
def test_engine_coefficient_table(o, lof, n):
    sig = _ladder(n)
    tab = tw.engine_table(sig, SD, o, bool(lof))
    ref = tw.coef_ref(sig, SD, o, bool(lof))
    worst, bad = tw.check_table(tab, ref)
    tol = {f: float(ref["tol"][:, j].max()) for j, f in enumerate(tw.FIELDS)}
    print(f"order {o} lower_order_final {lof} n_steps {n}: orders {''.join(str(int(v)) for v in tab[:, 11])}; worst err / tol "
          + " ".join(f"{f} {worst[f]:.2f}" for f in tw.FIELDS[:11]) + "; tolerance in u " + " ".join(f"{f} {tol[f] / U:.0f}" for f in tw.FIELDS[:11]))
    assert not bad, bad                                        # order, last, every coefficient the step's order does not use: exact
    assert max(worst.values()) <= 1.0, worst
    assert max(tol.values()) <= 2.0 ** -14, tol                # the cap for n_steps <= 20
    last = tw.row(tab, n - 1)
    assert last["a"] == 0.0 and last["b0"] == -1.0 and last["c_in_next"] == 0.0 and last["order"] == 1 and last["last"] == 1


def test_coefficient_tolerance_at_40_steps_is_reported():
    sig = _ladder(40)
    tab, ref = tw.engine_table(sig, SD, 3, True), tw.coef_ref(sig, SD, 3, True)
    worst, bad = tw.check_table(tab, ref)
    print("40 steps, order 3 (reported, not capped): tolerance in u " + " ".join(f"{f} {ref['tol'][:, j].max() / U:.0f}" for j, f in enumerate(tw.FIELDS[:11]))
          + f"; worst err / tol {max(worst.values()):.2f}")
    assert not bad and max(worst.values()) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ the emulation
N, C, H, W = 2, 5, 24, 40


def _emu(n_steps, order, T="bf16", guided=False, white=False, cimg=0, mutant=None, mutant_table=None, lof=True, n=N, h=H, w=W, seed=3):
    sig = _ladder(n_steps)
    tab = tw.engine_table(sig, SD, order, lof)
    Cin = C + cimg
    x0 = (rng.standard_normal(seed, (n, C, h, w)) * float(sig[0])).astype(np.float32)
    img = rng.standard_normal(seed + 1, (n, cimg, h, w)).astype(np.float32) if cimg else None
    model = tw.noise_model(C, 11) if white else tw.toy_model(C, 5)
    guide = (tw.noise_model(C, 12) if white else tw.toy_model(C, 6, 0.7)) if guided else None
    emu = tw.EmuSampler(tab, T, n, C, Cin, h, w, x0, _c_in0(sig), model, img, guide, 1.3 if guided else None, order, mutant, mutant_table)
    return tw.check_trajectory(emu.run, tab, T, C, Cin, order == 3, x0, _c_in0(sig), img, 1.3 if guided else None)


def test_fp32_emulation_passes_and_sets_the_constants():
    worstA, worstB, meds = 0.0, {False: 0.0, True: 0.0}, {False: [], True: []}
    for n_steps in (3, 6, 14, 15, 20):
        for order in (1, 2, 3):
            for guided in (False, True):
                for white in (False, True):
                    stats, viol = _emu(n_steps, order, guided=guided, white=white)
                    viol = [v for v in viol if "B(" not in v]          # B is what this test calibrates: judged below
                    assert not viol, (n_steps, order, guided, white, viol[:4])
                    worstA = max(worstA, max(max(s["A_x"], s["A_m0"]) for s in stats))
                    worstB[guided] = max(worstB[guided], max(max(s["B_x"], s["B_m0"]) for s in stats))
                    meds[guided] += [s["median_x"] for s in stats]
    allm = meds[False] + meds[True]
    print(f"emulation, {len(allm)} steps of {N * C * H * W} elements: worst err / E {worstA:.3f} (EMU_WORST_A = {tw.EMU_WORST_A}); B worst {worstB[False] / U:.3f} u "
          f"without a guide, x 4 = {4 * worstB[False] / U:.2f} u (C_RMS_STEP = {tw.C_RMS_STEP / U:.2f} u), {worstB[True] / U:.3f} u with one, x 4 = {4 * worstB[True] / U:.2f} u "
          f"(C_RMS_STEP_GUIDED = {tw.C_RMS_STEP_GUIDED / U:.2f} u); median E / |ref| {min(allm) / U:.1f} .. {max(meds[False]) / U:.1f} u without a guide, up to "
          f"{max(meds[True]) / U:.1f} u with one (cap 16 u)")
    assert 4.0 * worstB[False] <= tw.C_RMS_STEP <= 4.2 * worstB[False]
    assert 4.0 * worstB[True] <= tw.C_RMS_STEP_GUIDED <= 4.2 * worstB[True]
    assert worstA <= 1.0 and abs(worstA - tw.EMU_WORST_A) < 0.005
    lo, hi, hig = tw.MEDIAN_RANGE
    assert abs(min(allm) / U - lo) < 0.1 and abs(max(meds[False]) / U - hi) < 0.1 and abs(max(meds[True]) / U - hig) < 0.1
    assert hi * U <= tw.CAP / 2 and hig * U <= tw.CAP          # 2 x room without a guide, 1.47 x with one: A cannot go vacuous


def test_emulation_of_the_hand_offs_in_every_storage_type():
    for T in ("fp32", "bf16", "fp16"):
        for cimg in (0, 2):
            stats, viol = _emu(6, 3, T=T, cimg=cimg, n=2, h=6, w=10)
            assert not viol, (T, cimg, viol[:4])


def _mutant_tables(n_steps, order=3):
    sig = _ladder(n_steps)
    tab = tw.engine_table(sig, SD, order, True)
    j = tw.FIELDS.index("c_in_next")
    wrong_sigma = tab.copy()
    for i in range(n_steps - 1):
        wrong_sigma[i, j] = np.float32(1.0) / np.sqrt(np.float32(sig[i]) ** 2 + np.float32(SD) ** 2)
    no_clause = tab.copy()
    no_clause[n_steps - 2] = tw.engine_table(sig, SD, 2, True)[n_steps - 2]      # lower_order_second applied although n_steps >= 15
    return dict(lof=tw.engine_table(sig, SD, order, False), wrong_sigma=wrong_sigma, no_clause=no_clause)


MUTANTS = [  # name, n_steps, keyword arguments of _emu
    ("order-2 difference against m2", 6, dict(mutant="difference against m2")),
    ("0.5 of the order-2 term dropped", 6, dict(mutant="half dropped")),
    ("order 2 where the table says 3", 6, dict(mutant="order 2 for 3")),
    ("order 3 where the table says 2", 6, dict(mutant="order 3 for 2")),
    ("lower_order_final ignored", 6, dict(mutant_table="lof")),
    ("the n_steps < 15 clause ignored", 15, dict(mutant_table="no_clause")),
    ("history not shifted", 6, dict(mutant="history not shifted")),
    ("c_in_next from sigma_i", 6, dict(mutant_table="wrong_sigma")),
    ("guide mix with f and g swapped, gscale 1.3", 6, dict(mutant="guide swapped", guided=True)),
    ("last channel skipped", 6, dict(mutant="last channel skipped")),
    ("H and W swapped in the planar index", 6, dict(mutant="H and W swapped")),
    ("batch offset n * 8", 6, dict(mutant="batch offset n * 8")),
    ("the last step writes xin", 6, dict(mutant="last step writes xin")),
    ("ones channel at C, not Cin", 6, dict(mutant="ones channel at C", cimg=2)),
    ("b0 rounded to bf16", 6, dict(mutant="bf16 coefficient")),
]


@pytest.mark.parametrize("name,n_steps,kw", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_every_mutant_is_caught(name, n_steps, kw):
    kw = dict(kw)
    if "mutant_table" in kw:
        kw["mutant_table"] = _mutant_tables(n_steps)[kw["mutant_table"]]
    stats, viol = _emu(n_steps, 3, n=2, h=6, w=10, **kw)
    a, ex = tw.miss_factor(stats, viol)
    print(f"mutant '{name}': worst err / E {a:.3g}, exact hand-off elements that differ {ex}; first violation: {viol[0] if viol else None}")
    assert a > 1.0 or ex > 0, name
    assert any("A(" in v or "exact" in v for v in viol)        # caught by A or by an exact hand-off, not by B or the cap alone


def test_the_unbroken_sampler_passes_on_the_mutants_inputs():
    for cimg, guided, n_steps in ((0, False, 6), (2, False, 6), (0, True, 6), (0, False, 15)):
        stats, viol = _emu(n_steps, 3, n=2, h=6, w=10, cimg=cimg, guided=guided)
        assert not viol, viol[:4]


# ------------------------------------------------------------------------------------------------------------------ consistency sampler
def test_consistency_emulation_and_mutants():
    sample, z, F = (rng.standard_normal(40 + i, (2, C, 6, 10)).astype(np.float32) for i in range(3))
    for t in (0.3, 1.1, math.atan(80.0 / SD)):
        for smp in (sample, np.zeros_like(sample)):
            for T in ("fp32", "bf16", "fp16"):
                xt, xs, out = tw.emulate_consistency(t, SD, smp, z, F)
                xin = np.zeros((2, tw.CHUNK[T], 6, 10), np.float32)
                xin[:, :C], xin[:, C] = tw.rne(xs, T), 1.0
                st = tw.check_consistency(t, SD, smp, z, xt, xin, F, out, T, C, C)
                assert not tw.verdict_consistency(st), (t, T, tw.verdict_consistency(st))
    for mutant in ("sin and cos swapped", "sign of F"):
        xt, xs, out = tw.emulate_consistency(1.1, SD, sample, z, F, mutant)
        xin = np.zeros((2, 64, 6, 10), np.float32)
        xin[:, :C], xin[:, C] = tw.rne(xs, "bf16"), 1.0
        st = tw.check_consistency(1.1, SD, sample, z, xt, xin, F, out, "bf16", C, C)
        print(f"consistency mutant '{mutant}': err / E xt {st['A_xt']:.3g}, out {st['A_out']:.3g}")
        assert tw.verdict_consistency(st)
