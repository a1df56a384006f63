"""CPU: the ABI of the two new entry points, and the float64 twin of score scaling and of the windowed blend (tests/_sampler_args_twin.py) against the
reference's recorded `_scale_score` outputs, its own fp32 emulation, broken emulations and oracle/tiling.py."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_args_twin as sa   # noqa: E402
import _sampler_twin as tw        # noqa: E402

U = sa.U
SCORE_SIGMAS = (80.0, 3.0, 0.5, 0.002)


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def test_header_and_bindings_declare_the_new_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "td_engine.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(td_[a-z0-9_]+)\s*\(", text))
    from terrain_diffusion_amd._lib import EXPORTS
    for name in ("td_sample_edm_ext", "td_blend_windows_w"):
        assert name in declared, f"{name} is not declared in include/td_engine.h"
        assert name in EXPORTS, f"{name} is not bound in terrain_diffusion_amd/_lib.py"
    assert len(declared) == 47 and set(EXPORTS) == declared      # 45 before these two
    assert "td_edm_ext" in text and "score_cs_host" in text


def test_the_samplers_take_the_reference_arguments():
    """the signatures carry what the reference's do; the refusals that stay are not these three"""
    import inspect
    import terrain_diffusion_amd as td
    for fn in (td.sample_base_diffusion, td.sample_base_consistency, td.sample_decoder_diffusion_tiled, td.sample_decoder_consistency_tiled, td.sample_coarse_tiled):
        assert "weight_window_fn" in inspect.signature(fn).parameters
    p = inspect.signature(td.sample_decoder_diffusion_tiled).parameters
    assert {"guidance_model", "guidance_scale", "score_scaling"} <= set(p)
    assert inspect.signature(td.sample_tiles_edm).parameters["score_scaling"].default == 1.0
    src = inspect.getsource(sys.modules["terrain_diffusion_amd.sampling"])
    for gone in ("autoguidance with conditioning-image channels", "custom weight windows"):
        assert f'NotImplementedError("{gone}' not in src


def test_weight_window_fn_is_checked():
    from terrain_diffusion_amd.sampling import _weight_window
    ok = _weight_window(lambda s, d, t: torch.ones(1, 1, s, s, dtype=t), 8, "cpu")
    assert ok.shape == (8, 8) and ok.dtype == np.float32 and _weight_window(None, 8, "cpu") is None
    seen = []
    _weight_window(lambda s, d, t: seen.append((s, d, t)) or torch.ones(1, 1, s, s), 16, "cpu")
    assert seen == [(16, "cpu", torch.float32)]
    for bad in (lambda s, d, t: torch.ones(s, s), lambda s, d, t: torch.full((1, 1, s, s), float("nan")), lambda s, d, t: torch.full((1, 1, s, s), float("inf")),
                lambda s, d, t: -torch.ones(1, 1, s, s), lambda s, d, t: torch.ones(1, 1, s + 1, s)):
        with pytest.raises(ValueError):
            _weight_window(bad, 8, "cpu")


def test_score_table_is_the_reference_scalar_chain():
    """(cos t, sin t) from the same torch fp32 ops `_scale_score` uses on an fp32 sigma"""
    sig = torch.tensor([80.0, 3.0, 0.5, 0.002, 0.0])
    cs = sa.score_table(sig, 0.5)
    assert cs.shape == (4, 2) and cs.dtype == np.float32
    for i in range(4):
        t = torch.atan(sig[i] / torch.as_tensor(0.5, dtype=torch.float32))
        assert cs[i][0] == float(torch.cos(t)) and cs[i][1] == float(torch.sin(t))


def test_score_ref_reproduces_the_reference(golden):
    """every recorded `_scale_score` output (4 sigmas x 3 alphas, fp32 torch on the CPU) lies within E of the float64 twin, and within 1e-6 rel-RMS"""
    g = golden("sampler_args")
    f = g["score_f"]
    cs = sa.score_table(torch.tensor(SCORE_SIGMAS + (0.0,)), 0.5)
    worst = 0.0
    for si in range(len(SCORE_SIGMAS)):
        x = g[f"score_x:{si}"]
        for alpha in sa.ALPHAS:
            got = g[f"score:{si}:{alpha}"]
            ref, E = sa.score_ref(alpha, cs[si][0], cs[si][1], 0.5, x, f)
            ratio = float(np.max(np.abs(got.astype(np.float64) - ref) / (E * sa.SECOND_ORDER)))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (SCORE_SIGMAS[si], alpha, ratio)
            assert rel_rms(got, ref) < 1e-6, (SCORE_SIGMAS[si], alpha, rel_rms(got, ref))
            emu = sa.emulate_score(alpha, cs[si][0], cs[si][1], 0.5, x, f)
            assert np.array_equal(emu, got), f"the fp32 emulation is not the reference's fp32 result at sigma {SCORE_SIGMAS[si]}, alpha {alpha}"
    print(f"\n_scale_score goldens: worst |reference fp32 - twin| / E = {worst:.3f}; the numpy emulation equals the reference bit for bit")


def test_carry_is_step_ref_s_own_propagation():
    """carry(k) against step_ref: the guided bound minus the unguided bound at the same f is carry x E(guide mix), for every order"""
    rs = np.random.RandomState(1)
    sig = __import__("oracle.schedule", fromlist=["x"]).karras_sigmas(6)[0].numpy()
    for order in (1, 2, 3):
        table = tw.engine_table(sig, 0.5, order, True)
        for i in range(table.shape[0]):
            k = tw.row(table, i)
            x, F, g, m1, m2 = (rs.standard_normal(64).astype(np.float32) for _ in range(5))
            f, Ef = sa.guide_mix_ref(F, g, 1.3)
            a, b = tw.step_ref(k, x, F, m1, m2, g, 1.3), tw.step_ref(k, x, f, m1, m2)
            gx, gm = sa.carry(k)
            assert np.allclose(a["E_x"] - b["E_x"], gx * Ef * sa.SECOND_ORDER, rtol=1e-9, atol=1e-18)
            assert np.allclose(a["E_m0"] - b["E_m0"], gm * Ef * sa.SECOND_ORDER, rtol=1e-9, atol=1e-18)


def test_fp32_emulation_passes_and_sets_the_constants():
    """criterion A on every step of every case, tight somewhere (>= 0.5 of the bound), the cap holds, and the constants written in the twin are 4 x the worst B"""
    worst_a, worst_b, worst_med = 0.0, {False: 0.0, True: 0.0}, 0.0
    for name, sig, order, alpha, guided in sa.emu_cases():
        for st in sa.run_emu_case(sig, order, alpha, guided):
            a = max(st["A_x"], st["A_m0"])
            assert a <= 1.0, (name, st)
            worst_a = max(worst_a, a)
            worst_b[guided] = max(worst_b[guided], st["B_x"], st["B_m0"])
            worst_med = max(worst_med, st["median_x"], st["median_m0"])
    print(f"\nscore-scaled step, fp32 emulation: worst err / E {worst_a:.3f}; worst per-step rel-RMS {worst_b[False] / U:.3f} u plain, {worst_b[True] / U:.3f} u guided; "
          f"largest median E / scale {worst_med / U:.2f} u (cap {sa.CAP_SS / U:.2f} u)")
    assert worst_a >= 0.5 and abs(worst_a - sa.EMU_WORST_A) < 5e-3
    assert abs(worst_med - sa.MEDIAN_WORST) < 0.05 * U and 1.45 * worst_med <= sa.CAP_SS <= 1.55 * worst_med
    assert 4 * worst_b[False] <= sa.C_RMS_SS <= 4.2 * worst_b[False]
    assert 4 * worst_b[True] <= sa.C_RMS_SS_GUIDED <= 4.2 * worst_b[True]


@pytest.mark.parametrize("mutant", ["alpha on the noise prediction", "c and s swapped", "sign of v"])
def test_broken_emulations_miss_the_bound(mutant):
    worst = 0.0
    for name, sig, order, alpha, guided in sa.emu_cases():
        stats = sa.run_emu_case(sig, order, alpha, guided, mutant=mutant)
        miss = max(max(s["A_x"], s["A_m0"]) for s in stats)
        worst = miss if worst == 0.0 else min(worst, miss)
    print(f"\nmutant '{mutant}': misses the bound by >= {worst:.3g} x in every case")
    assert worst >= 100.0


def test_scaling_before_the_guide_mix_is_an_equivalent_mutant():
    """`_scale_score` is affine in the model output at a fixed sample (f' = A f + B x), and the guide mix's weights sum to one, so scaling both outputs and then
    mixing is the same function in real arithmetic: this candidate cannot miss the bound by a factor, only by roundings.  Asserted: the two orders agree to 1e-12 in
    float64, and the fp32 emulation of the swapped order stays within a small multiple of E (printed)."""
    rs = np.random.RandomState(2)
    x, F, g = (rs.standard_normal(256) * s for s in (80.0, 1.0, 1.0))
    cs = sa.score_table(torch.tensor([80.0, 0.0]), 0.5)[0]
    mixed_then_scaled = sa.score_ref(1.1, cs[0], cs[1], 0.5, x, g + 1.3 * (F - g))[0]
    a, b = sa.score_ref(1.1, cs[0], cs[1], 0.5, x, F)[0], sa.score_ref(1.1, cs[0], cs[1], 0.5, x, g)[0]
    assert np.max(np.abs(b + 1.3 * (a - b) - mixed_then_scaled)) <= 1e-12 * np.max(np.abs(mixed_then_scaled))
    worst = 0.0
    for name, sig, order, alpha, guided in sa.emu_cases():
        if guided:
            stats = sa.run_emu_case(sig, order, alpha, guided, mutant="scaled before the guide mix")
            worst = max(worst, max(max(s["A_x"], s["A_m0"]) for s in stats))
    print(f"\n'scaled before the guide mix': worst err / E {worst:.2f} (an equivalent mutant: roundings only)")
    assert worst < 100.0


def test_blend_ref_with_the_linear_window_is_the_oracle_blend():
    from oracle import tiling
    rs = np.random.RandomState(3)
    C, Hc, Wc, size = 3, 24, 40, 16
    rows, cols = tiling.tile_starts(Hc, size, 8), tiling.tile_starts(Wc, size, 8)
    idx = [(a, b) for a in range(len(rows)) for b in range(len(cols))]
    tiles = rs.standard_normal((len(idx), C, size, size)).astype(np.float32)
    w = tiling.linear_weight_window(size)
    ref, E = sa.blend_ref(tiles, w.numpy(), C, Hc, Wc, size, rows, cols, [a for a, _ in idx], [b for _, b in idx])
    acc, ws = torch.zeros(C, Hc, Wc, dtype=torch.float64), torch.zeros(Hc, Wc, dtype=torch.float64)
    for k, (a, b) in enumerate(idx):
        acc[:, rows[a]:rows[a] + size, cols[b]:cols[b] + size] += torch.from_numpy(tiles[k]).double() * w.double()
        ws[rows[a]:rows[a] + size, cols[b]:cols[b] + size] += w.double()
    assert np.allclose(ref[:C], acc.numpy(), rtol=1e-14, atol=1e-14) and np.allclose(ref[C], ws.numpy(), rtol=1e-14, atol=0)
    import _tile_twin as tt
    ref2, E2 = tt.blend_ref(tiles, C, Hc, Wc, size, rows, cols, [a for a, _ in idx], [b for _, b in idx])
    assert np.array_equal(ref, ref2) and np.array_equal(E, E2)
