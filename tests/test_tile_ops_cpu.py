"""CPU: the criterion of tests/_tile_twin.py bites, and its float64 twins are the project's oracles.

* every twin against the oracle of its operation with equal float64 inputs (oracle/tiling.py's weight window and blend loop, oracle/compose.py's operators and
  expressions, oracle/ddim.py), to 1e-12 relative;
* torch's own CPU grid_sample in fp32, on the reference's grid, passes criterion A of the climate twin on every case;
* the fp32 emulations pass A, the non-finite rule and the cap; C_RMS, CAP, MEDIAN_RANGE and EMU_WORST_A are re-measured and asserted;
* every broken emulation misses A; the factor is printed.
No engine library is loaded here."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tile_twin as tw

U = tw.U


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------------------------------------------------------ the twins are the oracles
def test_weight_window_and_tile_starts_are_the_oracles():
    from oracle import tiling
    for size in (2, 5, 8, 16, 64):
        assert np.array_equal(tw.weight_window(size), tiling.linear_weight_window(size).numpy()), size
    for n, t, s in ((40, 16, 8), (37, 16, 8), (29, 16, 8), (21, 8, 4), (17, 8, 4), (5, 8, 4)):
        assert tw.tile_starts(n, t, s) == tiling.tile_starts(n, t, s)


def test_blend_and_regions_twins_against_the_oracle_blend_loop():
    """oracle/tiling.py:135-136 (`output[window] += x * weights; output_weights[window] += weights`) in float64 torch with the same fp32 window; cropping an
    overhanging window is the slice of a padded canvas"""
    worst = 0.0
    for name, cs in tw.blend_cases().items():
        C, Hc, Wc, size = cs["C"], cs["Hc"], cs["Wc"], cs["size"]
        w = torch.from_numpy(tw.weight_window(size)).double()
        pad = size
        prior = cs["prior"]
        for idx, accumulate in cs["launches"]:
            wi, wj = [cs["grid"][i][0] for i in idx], [cs["grid"][i][1] for i in idx]
            out = torch.zeros((C + 1, Hc + 2 * pad, Wc + 2 * pad), dtype=torch.float64)
            if accumulate:
                out[:, pad:pad + Hc, pad:pad + Wc] = torch.from_numpy(np.asarray(prior, np.float64))
            order = sorted(range(len(idx)), key=lambda k: (wi[k], wj[k]))
            for k in order:
                i0, j0 = cs["rows"][wi[k]] + pad, cs["cols"][wj[k]] + pad
                x = torch.from_numpy(cs["tiles"][idx[k]]).double()
                out[:C, i0:i0 + size, j0:j0 + size] += x * w
                out[C, i0:i0 + size, j0:j0 + size] += w
            ref, _ = tw.blend_ref(cs["tiles"][idx], C, Hc, Wc, size, cs["rows"], cs["cols"], wi, wj, accumulate, prior)
            worst = max(worst, _rel(ref, out[:, pad:pad + Hc, pad:pad + Wc].numpy()))
            prior = tw.blend_emu(cs["tiles"][idx], C, Hc, Wc, size, cs["rows"], cs["cols"], wi, wj, accumulate, prior)
    for name, cs in tw.regions_cases().items():
        C, size, h, w_ = cs["C"], cs["size"], cs["h"], cs["w"]
        w = torch.from_numpy(tw.weight_window(size)).double()
        ref, _ = tw.regions_ref(cs["wins"], cs["desc"], C, size, h, w_)
        for r in range(cs["desc"].shape[0]):
            out = torch.zeros((C + 1, h + 2 * size + 2, w_ + 2 * size + 2), dtype=torch.float64)
            for slot, oy, ox in cs["desc"][r]:
                if slot < 0:
                    break
                i0, j0 = int(oy) + size + 1, int(ox) + size + 1
                out[:C, i0:i0 + size, j0:j0 + size] += torch.from_numpy(cs["wins"][slot]).double() * w
                out[C, i0:i0 + size, j0:j0 + size] += w
            worst = max(worst, _rel(ref[r], out[:, size + 1:size + 1 + h, size + 1:size + 1 + w_].numpy()))
    print(f"blend / regions twins against the oracle's blend loop in float64: worst relative difference {worst:.2e}")
    assert worst < 1e-12


def test_normalise_elev_and_ddim_twins_against_the_oracle_expressions():
    from oracle import ddim
    worst = {}
    for name, cs in tw.normalise_cases().items():                         # oracle/tiling.py:139 `output / output_weights / sigma_data` = x (1 / sigma_data)
        c = torch.from_numpy(cs["canvas"]).double()
        ref, _ = tw.normalise_ref(cs["canvas"], cs["scale"])
        want = (c[:-1] / c[-1:] * float(np.float32(cs["scale"]))).numpy()
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(ref), np.isnan(want)) and np.array_equal(np.isinf(ref), np.isinf(want))
        worst["normalise"] = max(worst.get("normalise", 0), _rel(ref[fin], want[fin]))
    for stats in tw.ELEV_STATS:                                           # oracle/compose.py:84 residual_p, :67 residual + up, :91 sign(e) * square(e)
        packed, low, mean, std = tw.elev_inputs(stats)
        r = torch.from_numpy(packed).double()
        m64, s64 = float(np.float32(mean)), float(np.float32(std))
        e = (r[0] / r[1]) * s64 + m64 + torch.from_numpy(low).double()
        worst["residual_plus"] = max(worst.get("residual_plus", 0), _rel(tw.elev_ref(packed, low, mean, std)[0], e.numpy()))
        for crop in tw.ELEV_CROPS.values():
            oi, oj, h, w = crop
            ec = e[oi:oi + h, oj:oj + w]
            worst["elev_finish"] = max(worst.get("elev_finish", 0), _rel(tw.elev_ref(packed, low, mean, std, crop)[0], (torch.sign(ec) * torch.square(ec)).numpy()))
    n_ddim = 0
    for name, cs in tw.ddim_cases().items():
        ref, _ = tw.ddim_ref(cs["x"], cs["uncond"], cs["cond"], cs["g"], cs["alpha_t"], cs["alpha_prev"])
        a, p = float(np.float32(cs["alpha_t"])), float(np.float32(cs["alpha_prev"]))
        eps = ddim.cfg_mix(cs["uncond"].astype(np.float64), cs["cond"].astype(np.float64), float(np.float32(cs["g"])))
        s1, s2, s3, s4 = (float(v) for v in tw.ddim_scalars(a, p))
        want = s3 * ((cs["x"].astype(np.float64) - s1 * eps) / s2) + s4 * eps          # oracle/ddim.py:40-41 on the fp32 scalars
        worst["ddim"] = max(worst.get("ddim", 0), _rel(ref, want))
        if a >= 0.5 and p >= 0.5:       # 1 - alpha is exact in fp32 there, and a double sqrt rounded to fp32 is the correctly rounded sqrtf: ddim_step's scalars ARE the kernel's
            worst["ddim_step"] = max(worst.get("ddim_step", 0), _rel(ref, ddim.ddim_step(cs["x"].astype(np.float64), eps, a, p)))
            n_ddim += 1
    print("twins against the oracle's expressions in float64: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert n_ddim >= 3 and max(worst.values()) < 1e-12, worst


def test_resample_twin_against_dense_matrices_and_the_oracle_operators():
    """The twin applies fp32 tap tables; the same tables as dense float64 matrices give Wy X Wx^T (1e-12).  oracle/compose.py's operators are spelled in fp32 and compute
    their own weights, so they pin the tables (test_compose_cpu.py), not the sums: the twin on the product's tables reproduces them to fp32 accuracy, printed."""
    from oracle import compose
    from terrain_diffusion_amd import composition as cp
    worst = 0.0
    for name, cs in tw.resample_cases().items():
        (iy, wy), (ix, wx) = cs["ty"], cs["tx"]
        x = np.where(np.isfinite(cs["x"]), cs["x"], 0.0).astype(np.float64)      # the zero-weight taps are the only ones at those cells
        My, Mx = np.zeros((iy.shape[0], x.shape[1])), np.zeros((ix.shape[0], x.shape[2]))
        for k in range(iy.shape[1]):
            np.add.at(My, (np.arange(iy.shape[0]), iy[:, k]), wy[:, k].astype(np.float64))
        for k in range(ix.shape[1]):
            np.add.at(Mx, (np.arange(ix.shape[0]), ix[:, k]), wx[:, k].astype(np.float64))
        ref, _ = tw.resample_ref(cs["x"], cs["ty"], cs["tx"])
        assert np.all(np.isfinite(ref)), name
        worst = max(worst, _rel(ref, np.einsum("ya,cab,xb->cyx", My, x, Mx)))
    x = tw.resample_cases()["composed: upsample 5x8 -> 37x64, C 3"]["x"]
    up = _rel(tw.resample_ref(x, cp.bilinear_taps(5, 37), cp.bilinear_taps(8, 64))[0], compose.tf_resize(torch.from_numpy(x), (37, 64)).numpy())
    x = tw.resample_cases()["composed: AA shrink 64x37 -> 9x5, C 1"]["x"]
    aa = _rel(tw.resample_ref(x, cp.bilinear_aa_taps(64, 9), cp.bilinear_aa_taps(37, 5))[0], compose.tf_resize(torch.from_numpy(x), (9, 5)).numpy())
    x = tw.resample_cases()["composed: Gaussian sigma 5, 12x13, C 3"]["x"]
    ga = _rel(tw.resample_ref(x, cp.gaussian_taps(12, 5), cp.gaussian_taps(13, 5))[0], compose.tf_gaussian_blur(torch.from_numpy(x), 5).numpy())
    print(f"resample twin against dense float64 matrices {worst:.2e}; against the oracle's fp32 operators: upsample {up:.2e}, AA shrink {aa:.2e}, Gaussian {ga:.2e}")
    assert worst < 1e-12 and max(up, aa, ga) < 2e-6


def _reference_grid(cs):
    """oracle/compose.py:123-126 as written (fp32 torch)"""
    i1, j1, h, w, S, ci1, cj1, Hs, Ws = cs["i1"], cs["j1"], cs["h"], cs["w"], int(cs["S"]), cs["ci1"], cs["cj1"], cs["Hs"], cs["Ws"]
    ii, jj = torch.meshgrid(torch.arange(i1, i1 + h), torch.arange(j1, j1 + w), indexing="ij")
    u = (ii + 0.5) / S - ci1 + 0.5
    v = (jj + 0.5) / S - cj1 + 0.5
    return torch.stack([(v + 0.5) * 2 / Ws - 1, (u + 0.5) * 2 / Hs - 1], dim=-1).unsqueeze(0)


def test_climate_twin_is_grid_sample():
    """(a) the twin's fp32 grid is the reference's, bit for bit; (b) its float64 blend agrees with F.grid_sample in float64 on the coordinates of the fp32 chain to
    1e-12; (c) torch's own CPU grid_sample in fp32 on the reference's grid passes criterion A on every case."""
    worst64, worstA = 0.0, 0.0
    for name, cs in tw.climate_cases().items():
        Hs, Ws, i1, j1, h, w, S, ci1, cj1 = tw.climate_args(cs)
        grid = _reference_grid(cs)
        y, _, _, gy, _ = tw.climate_coords(Hs, i1, h, S, ci1)
        x, _, _, gx, _ = tw.climate_coords(Ws, j1, w, S, cj1)
        assert grid.dtype == torch.float32 and np.array_equal(grid[0, :, 0, 1].numpy(), gy) and np.array_equal(grid[0, 0, :, 0].numpy(), gx), name
        f = tw.climate_blend64(cs["feats"], y, x)[0]
        g64 = torch.stack(torch.meshgrid(torch.from_numpy((2 * y.astype(np.float64) + 1) / Hs - 1), torch.from_numpy((2 * x.astype(np.float64) + 1) / Ws - 1), indexing="ij")[::-1], dim=-1)[None]
        up = F.grid_sample(torch.from_numpy(cs["feats"]).double()[None], g64, mode="bilinear", padding_mode="border", align_corners=False)[0].numpy()
        worst64 = max(worst64, max(_rel(f[k], up[k]) for k in range(5)))
        up32 = F.grid_sample(torch.from_numpy(cs["feats"])[None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0]
        elev = torch.from_numpy(cs["elev"])
        got = torch.stack([up32[0] + up32[1] * torch.maximum(elev, torch.zeros_like(elev)), up32[2], up32[3], up32[4], up32[1]]).numpy()      # oracle/compose.py:129-130
        ref, E = tw.climate_ref(cs["feats"], cs["elev"], Hs, Ws, i1, j1, h, w, S, ci1, cj1)
        st = tw.judge(got, ref, E)
        print(f"torch CPU grid_sample fp32 | {name}: worst err / E {st['A']:.3f} at {st['at']}")
        worstA = max(worstA, st["A"])
        assert st["A"] <= 1.0 and st["masks_ok"], (name, st)
    print(f"climate twin: float64 blend against F.grid_sample(float64) {worst64:.2e}; torch's fp32 grid_sample reaches {worstA:.3f} of E")
    assert worst64 < 1e-12


# ------------------------------------------------------------------------------------------------------------------ the emulations set the constants
def _measure():
    A, B, med = {}, {}, {}
    for fused in (True, False):
        for op, name, shape, got, ref, E in tw.all_cases(lambda op, name, cs, **kw: tw.emulate(op, name, cs, fused=fused, **kw)):
            st = tw.judge(got, ref, E)
            assert st["masks_ok"] and st["A"] <= 1.0 and st["excluded"] <= tw.MAX_EXCLUDED, (op, name, fused, st)
            A[op], B[op] = max(A.get(op, 0.0), st["A"]), max(B.get(op, 0.0), st["B"])
            med.setdefault(op, []).append(st["median"])
            if name.startswith("zero-weight taps"):
                assert np.all(np.isfinite(got)) and st["excluded"] == 0.0
    return A, B, med


def test_fp32_emulations_pass_and_set_the_constants():
    A, B, med = _measure()
    for op in tw.OPS:
        lo, hi = min(med[op]) / U, max(med[op]) / U
        print(f"{op}: {len(med[op]) // 2} cases; emulation worst err / E {A[op]:.3f} (EMU_WORST_A {tw.EMU_WORST_A[op]}); B worst {B[op] / U:.4f} u, x 4 = {4 * B[op] / U:.4f} u "
              f"(C_RMS {tw.C_RMS[op]}); median E / |ref| {lo:.3f} .. {hi:.3f} u (MEDIAN_RANGE {tw.MEDIAN_RANGE[op]}, CAP {tw.CAP[op]})")
    for op in tw.OPS:
        lo, hi = min(med[op]) / U, max(med[op]) / U
        assert abs(A[op] - tw.EMU_WORST_A[op]) < 0.005, (op, A[op])
        assert 4.0 * B[op] / U <= tw.C_RMS[op] <= 4.2 * B[op] / U, (op, B[op] / U)
        assert abs(lo - tw.MEDIAN_RANGE[op][0]) < 0.01 and abs(hi - tw.MEDIAN_RANGE[op][1]) < 0.01, (op, lo, hi)
        assert hi <= tw.CAP[op] <= 2 * hi, (op, hi)


def test_refusals_of_the_emulations():
    b = tw.blend_cases()["regular size 16 stride 8, 40x40, C 5"]
    with pytest.raises(tw.Refused):
        tw.blend_ref(np.zeros((1, 8, 4, 4), np.float32), 8, 8, 8, 4, [0], [0], [0], [0])
    with pytest.raises(tw.Refused):
        tw.blend_ref(np.zeros((5, 1, 8, 8), np.float32), 1, 12, 12, 8, [0, 1, 2, 3, 4], [0], [0, 1, 2, 3, 4], [0] * 5)
    with pytest.raises(tw.Refused):
        tw.blend_ref(b["tiles"][:1], 5, 40, 40, 16, b["rows"], b["cols"], [len(b["rows"])], [0])
    with pytest.raises(tw.Refused):
        tw.regions_ref([np.zeros((1, 4, 4), np.float32)], np.array([[[1, 0, 0]]]), 1, 4, 4, 4)
    with pytest.raises(tw.Refused):
        tw.elev_ref(np.ones((2, 19, 23), np.float32), np.ones((19, 23), np.float32), 0.0, 1.0, (10, 0, 10, 23))
    for a, p in ((0.0, 0.5), (1.5, 0.5), (0.5, 0.0), (0.5, -1.0), (float("nan"), 0.5)):
        with pytest.raises(tw.Refused):
            tw.ddim_scalars(a, p)


# ------------------------------------------------------------------------------------------------------------------ broken emulations
B_STRIDE4 = "stride size/4: 16 live terms, size 16, 28x28, C 7"
R_FIVE = "five regions sharing five windows, 17x19, maxk 6"
MUTANTS = [  # op, mutant, names of the committed cases it is run on
    ("blend", "mid = size / 2", [B_STRIDE4, "size 2 stride 1, 5x7, C 1"]),
    ("blend", "ly / lx swapped", [B_STRIDE4]),
    ("blend", "fourth covering row-window dropped", [B_STRIDE4]),
    ("blend", "weight channel misses one window", [B_STRIDE4]),
    ("blend", "accumulate ignores the prior canvas", ["accumulate over a non-zero canvas made by the test, size 8, 21x17, C 4", "two launches, the second accumulates on the first, size 8, 21x17, C 4"]),
    ("blend", "overhang clamped, not cropped", ["overhang on all four sides, size 8, 11x13, C 2"]),
    ("regions", "mid = size / 2", [R_FIVE]),
    ("regions", "ly / lx swapped", [R_FIVE]),
    ("regions", "weight channel misses one window", [R_FIVE]),
    ("regions", "terminator ignored", [R_FIVE]),
    ("regions", "bounds test <= size", [R_FIVE]),
    ("normalise", "divided by channel 0", None),
    ("resample", "last tap dropped", ["composed: upsample 5x8 -> 37x64, C 3", "composed: AA shrink 64x37 -> 9x5, C 1"]),
    ("resample", "table row stride K - 1", ["composed: upsample 5x8 -> 37x64, C 3", "composed: Gaussian sigma 5, 12x13, C 3"]),
    ("resample", "tables swapped", ["composed: hand-made table with negative weights in y, Gaussian in x, 12x12, C 3"]),
    ("resample", "zero weights not skipped", ["zero-weight taps on inf / NaN cells, 6x7 -> 8x9, C 1"]),
    ("elev_finish", "oi / oj swapped", None),
    ("elev_finish", "sign lost", None),
    ("elev_finish", "std / mean swapped", None),
    ("elev_finish", "divided by p0", None),
    ("elev_finish", "plane stride from the crop", None),
    ("residual_plus", "std / mean swapped", None),
    ("residual_plus", "divided by p0", None),
    ("climate", "align_corners=True", None),
    ("climate", "no border clamp", None),
    ("climate", "wne / wsw swapped", None),
    ("climate", "max(elev, 0) dropped", None),
    ("climate", "planes 1-4 rotated", None),
    ("climate", "no +0.5 in u", None),
    ("climate", "ci1 truncated towards zero", None),
    ("ddim", "g applied to cond only", None),
    ("ddim", "s1 / s4 swapped", None),
]


def _run_mutant(op, mutant, names):
    worst, where = 0.0, None

    def run(o, name, cs, **kw):
        return tw.emulate(o, name, cs, mutant=mutant if o == op and (names is None or name in names) else None, **kw)
    for o, name, shape, got, ref, E in tw.all_cases(run):
        if o != op or not (names is None or any(name.startswith(n) for n in names)):
            continue
        a = tw.judge(got, ref, E)["A"]
        if a > worst:
            worst, where = a, name
    return worst, where


@pytest.mark.parametrize("op,mutant,names", MUTANTS, ids=[f"{m[0]}: {m[1]}" for m in MUTANTS])
def test_every_broken_emulation_misses_A(op, mutant, names):
    worst, where = _run_mutant(op, mutant, names)
    print(f"broken {op} '{mutant}': misses A by a factor {worst:.3g} (case: {where})")
    assert worst >= 100.0, (op, mutant, worst)


def test_the_clamped_far_corner_is_an_equivalent_mutant():
    """'the far corner not skipped (index clamped instead)': on a clamped coordinate t is exactly 0, so the far corner's weight is exactly 0 and the clamped index
    names the cell already used; with finite features no bit changes.  Asserted, so that nobody reads the skip as a numerical matter (tests/_tile_twin.py header)."""
    for name, cs in tw.climate_cases().items():
        a = tw.climate_emu(cs["feats"], cs["elev"], *tw.climate_args(cs))
        b = tw.climate_emu(cs["feats"], cs["elev"], *tw.climate_args(cs), mutant="far corner clamped, not skipped")
        assert np.array_equal(a, b), name


# ------------------------------------------------------------------------------------------------------------------ the int32 guard of the noise windows
def test_noise_origins_outside_int32_are_refused_before_the_engine_is_reached():
    from terrain_diffusion_amd import noise
    ok = [(-2 ** 31, 0), (2 ** 31 - 24, 2 ** 31 - 40), (0, -2 ** 31)]
    noise.check_origins(np.asarray(ok, np.int64), 24, 40)
    for bad in ([(2 ** 31 - 23, 0)], [(0, 2 ** 31 - 39)], [(-2 ** 31 - 1, 0)], [(0, 0), (0, -2 ** 31 - 1)], [(2 ** 40, 0)]):
        with pytest.raises(ValueError):
            noise.check_origins(np.asarray(bad, np.int64), 24, 40)
        with pytest.raises(ValueError):       # raised before any engine call: no GPU and no library here
            noise.gaussian_noise_patches(1, bad, 24, 40, channels=1, tile_h=24, tile_w=40)
