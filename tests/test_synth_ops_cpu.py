"""CPU: the criterion of tests/_synth_twin.py bites, and its constants are what the fp32 emulations measure.

* the fp32 emulations of perlin_map_kernel (the recorded device table for the gradients, fused as the build fuses and unfused; numpy's own sine and cosine as a third
  table) pass A on every committed case; EMU_WORST_A, MEDIAN_RANGE, CAP and C_RMS are re-measured and asserted;
* oracle/synthmap.fbm_map, one more fp32 emulation (unfused angle, numpy's libm), passes the judge on every case;
* the narrow source range is clamped on both sides by at least 5 % of the pixels each and the wide one nowhere; the knots placed on sums of the twin are met;
* every broken emulation misses A by at least 100 x on a named case; the factor is printed.
No engine library is loaded here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _synth_twin as sw

U = sw.U


@pytest.fixture(scope="module")
def refs():
    """the float64 twin of every committed case, computed once and shared"""
    return {name: sw.fbm_ref(*cs["args"], cs["src"], cs["dst"]) for name, cs in sw.cases().items()}


def _emu(cs, **kw):
    return sw.fbm_emu(*cs["args"], cs["src"], cs["dst"], **kw)


def test_the_recorded_device_table_is_within_the_measured_error_and_its_angles_are_the_fused_chain(golden):
    t = golden("sincos_gfx950")
    assert np.array_equal(t["angle"], sw.angles(fused=True)) and int(np.count_nonzero(sw.angles(True) != sw.angles(False))) == 30
    a = t["angle"].astype(np.float64)
    ec, es = np.abs(t["cos"] - np.cos(a)).max(), np.abs(t["sin"] - np.sin(a)).max()
    print(f"recorded device table: max |cos err| {ec:.3e}, max |sin err| {es:.3e}; EPS_SINCOS {sw.EPS_SINCOS:.3e}, E uses x {sw.SINCOS_MARGIN:g}")
    assert 0.99 * sw.EPS_SINCOS <= max(ec, es) <= sw.EPS_SINCOS


def test_fp32_emulations_pass_and_set_the_constants(refs):
    A, B, med = 0.0, 0.0, []
    cases = sw.cases()
    assert len(cases) == sw.N_CASES
    for fused in (True, False):
        for name, cs in cases.items():
            ref, E, _ = refs[name]
            st = sw.judge(_emu(cs, fused=fused), ref, E)
            assert st["masks_ok"] and st["A"] <= 1.0 and st["excluded"] == 0.0, (name, fused, st)
            A, B = max(A, st["A"]), max(B, st["B"])
            if fused:
                med.append(st["median"])
    for name, cs in cases.items():                                   # numpy's sine and cosine in place of the device's: inside A too (not a constant's source)
        ref, E, _ = refs[name]
        st = sw.judge(_emu(cs, table=sw.libm_table()), ref, E)
        assert st["masks_ok"] and st["A"] <= 1.0, (name, st)
    lo, hi = min(med) / U, max(med) / U
    print(f"synth: {len(cases)} cases; emulation worst err / E {A:.3f} (EMU_WORST_A {sw.EMU_WORST_A}); B worst {B / U:.4f} u, x 4 = {4 * B / U:.4f} u (C_RMS {sw.C_RMS}); "
          f"median E / |ref| {lo:.3f} .. {hi:.3f} u (MEDIAN_RANGE {sw.MEDIAN_RANGE}, CAP {sw.CAP})")
    assert abs(A - sw.EMU_WORST_A) < 0.005, A
    assert 4.0 * B / U <= sw.C_RMS <= 4.2 * B / U, B / U
    assert abs(lo - sw.MEDIAN_RANGE[0]) < 0.01 and abs(hi - sw.MEDIAN_RANGE[1]) < 0.01, (lo, hi)
    assert hi <= sw.CAP <= 2 * hi, hi
    for name, cs in cases.items():
        assert not sw.verdict(sw.judge(_emu(cs), *refs[name][:2])), name


def test_the_oracle_fbm_map_passes_the_judge(refs):
    from oracle import synthmap
    worst = 0.0
    for name, cs in sw.cases().items():
        ref, E, _ = refs[name]
        st = sw.judge(synthmap.fbm_map(*cs["args"], cs["src"], cs["dst"]), ref, E)
        print(f"oracle fbm_map | {name}: worst err / E {st['A']:.3f}, B {st['B'] / U:.3f} u")
        assert not sw.verdict(st), (name, sw.verdict(st))
        worst = max(worst, st["A"])
    assert worst <= 1.0


def test_clamps_lattice_points_and_knots_are_what_the_cases_say(refs):
    cases = sw.cases()
    for name, cs in cases.items():
        ref, E, info = refs[name]
        s, Es = info["sum"], info["E_sum"]
        left, right = float(np.mean(s < cs["src"][0] - Es)), float(np.mean(s > cs["src"][-1] + Es))
        if "narrower" in name:
            print(f"{name}: {100 * left:.1f} % beyond the left clamp, {100 * right:.1f} % beyond the right")
            assert left >= 0.05 and right >= 0.05
            assert np.all(E[s < cs["src"][0] - Es] == 0) and np.all(ref[s > cs["src"][-1] + Es] == np.float64(cs["dst"][-1]))
        if "wider" in name:
            assert np.all(s - Es > cs["src"][0]) and np.all(s + Es < cs["src"][-1])
        if "every point on the lattice" in name:
            assert np.all(s == 0) and np.all(Es == 0)                  # the noise is exactly 0 there, and so is its bound
        if "lattice and half points" in name:
            assert 0 < np.count_nonzero((s == 0) & (Es == 0)) < s.size
        if "three knots" in name:
            src, dst, picks = sw.knot_table(cs["args"])
            assert np.array_equal(src, cs["src"]) and all(p in src for p in picks)
            on = [(np.abs(s - float(p)) <= Es) for p in picks]
            assert all(m.any() for m in on)                             # a sum within E_sum of each placed knot
            k = int(np.searchsorted(src, picks[1]))
            big = max(abs(float(dst[k + 1] - dst[k]) / float(src[k + 1] - src[k])), abs(float(dst[k] - dst[k - 1]) / float(src[k] - src[k - 1])))
            assert np.all(E[on[1]] >= big * Es[on[1]])                  # the larger adjacent slope carries E_sum there
    for n in ("1x257", "3x300", "50x70"):                               # rows that are no multiple of the 256-thread block
        assert any(k.startswith(n) for k in cases)


MUTANTS = [  # mutant, the committed cases it is run on
    ("smoothstep fade", ["3x300 straddling 0"]),
    ("trunc for floor", ["3x300 straddling 0", "23x37 at (-3, -3)"]),
    ("coordinate primes swapped", ["50x70 at (-37, 1200), default stats channel 0"]),
    ("seed not advanced per octave", ["50x70 at (-37, 1200), default stats channel 1"]),
    ("amplitude not divided by the bound", ["20x70 at (-2^20, 2^20)"]),
    ("lacunarity applied before the first octave", ["23x37 at (-3, -3)", "17x33 at (-37, 1200), f 0.075, 1 octave"]),
    ("slope from the neighbouring interval", ["17x33 at (5, -40), f 0.075, 2 octaves, nq 3", "24x50 at (-12, 7)"]),
    ("right clamp returns dst[nq - 2]", ["40x60 at (-37, 1200), f 0.075, 4 octaves, source range narrower"]),
    ("rows / cols transposed", ["3x300 straddling 0", "30x40 at (0, 0)"]),
    ("i1 added to the column", ["20x70 at (2^20, -2^20)", "50x70 at (-37, 1200), default stats channel 2"]),
]


@pytest.mark.parametrize("mutant,names", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_every_broken_emulation_misses_A(refs, mutant, names):
    worst, where, ran = 0.0, None, 0
    for name, cs in sw.cases().items():
        if not any(name.startswith(n) for n in names):
            continue
        ran += 1
        ref, E, _ = refs[name]
        got = _emu(cs, mutant=mutant)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(got == ref, 0.0, np.abs(got - ref) / E)
        finite = ratio[np.isfinite(ratio)]                              # a pixel held exactly (E = 0, beyond a clamp) that moves misses by any factor
        a = float(finite.max()) if finite.size else 0.0
        if np.isinf(ratio).any():
            a = float("inf")
        print(f"broken synth '{mutant}' | {name}: misses A by a factor {a:.3g} ({int(np.count_nonzero(ratio > 1))} of {ratio.size} elements outside E"
              f"{', worst finite factor %.3g' % finite.max() if np.isinf(a) and finite.size else ''})")
        if a > worst:
            worst, where = a, name
    assert ran == len(names) and worst >= 100.0, (mutant, worst, where)
