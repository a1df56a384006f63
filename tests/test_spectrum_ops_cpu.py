"""The fp32 restatement of the spectrum kernels (tests/_spectrum_twin.py) without a GPU: every coefficient of fft2_fp32 within the running
bound E of float64 on the committed cases and on every side 8 .. 4096 of each axis, its relative L2 within the existing 4 rho, decode_fp32
within decode_ref's Ev with the same count of v <= 0, and the power of the criteria: seeded faults that pass both criteria of
tests/test_beauty_gpu.py (relative L2 <= 4 rho, |d log|F|| < 0.1 everywhere) and are flagged by E at a coefficient, hence by the bit
comparison tests/test_spectrum_ops_gpu.py makes; and the candidates that the old criteria do catch, on record with their figures.

Worst err / E over all planes: 0.114 (thin_8x8); 0.006 - 0.11 per plane, see DESIGN.md, "How the spectrum kernels are checked"."""
import json

import numpy as np
import pytest

import _beauty_twin as twin
import _spectrum_twin as st

F = np.float32


@pytest.fixture(scope="module")
def cases(golden):
    return json.loads(str(golden("beauty")["cases"]))


@pytest.fixture(scope="module")
def planes():
    return st.all_planes()


def old_criteria(z, f64, rho):
    """(relative L2 / rho, max |log|z| - log|F64||): the two guards tests/test_beauty_gpu.py has on the transform"""
    z = z.astype(np.complex128)
    l2 = float(np.sqrt((np.abs(z - f64) ** 2).sum() / (np.abs(f64) ** 2).sum()))
    with np.errstate(divide="ignore", invalid="ignore"):
        dlog = float(np.abs(np.log(np.abs(z)) - np.log(np.abs(f64))).max())
    return l2 / rho, dlog


# ------------------------------------------------------------------------------------------------------------------------------ restatement
def test_every_restated_coefficient_is_within_E_of_float64(planes):
    worst = {}
    for name, x in st.single_planes(planes):
        z, f64, E = st.fft2_fp32(x).astype(np.complex128), twin.half_of(twin.spectrum(x)), st.fft2_bound(x)
        assert z.shape == f64.shape == E.shape == (x.shape[0], x.shape[1] // 2 + 1) and (E > 0).all()
        err = np.abs(z - f64)
        worst[name] = float((err / E).max())
        print(f"restatement {name:18s} {z.size:7d} coefficients  worst err / E {worst[name]:.4f}")
        assert (err <= E).all(), (name, worst[name])
    sides = {(a, n) for name, x in st.single_planes(planes) for a, n in enumerate(x.shape)}
    assert {(a, n) for a in (0, 1) for n in st.SIDES} <= sides                      # every side on each axis
    assert {(512, 16), (16, 2048), (2048, 16), (4096, 8), (8, 4096)} <= {x.shape for _, x in st.single_planes(planes)}
    # the bound decides something: a largest ratio below about a hundredth would mean a rounding counted many times over
    top = max(worst.values())
    print(f"restatement: largest err / E over {len(worst)} planes {top:.4f}")
    assert 0.01 <= top <= 1.0


def test_flat_planes_are_exact_off_dc(planes):
    for name in ("flat_16", "batch5_16x32"):
        x = planes[name] if planes[name].ndim == 2 else planes[name][4]
        z = st.fft2_fp32(x)
        assert z[0, 0] == 7.5 * x.size and np.count_nonzero(z) == 1


def test_restated_relative_l2_within_four_rho_on_the_committed_cases(cases, planes):
    for e in cases["spectrum"]:
        x = planes[e["name"]]
        ratio, dlog = old_criteria(st.fft2_fp32(x), twin.half_of(twin.spectrum(x)), e["rho"] or 1.0)
        print(f"restatement {e['name']:14s} rel L2 / rho {ratio if e['rho'] else 0.0:.2f} (bound 4)")
        assert ratio * (e["rho"] or 1.0) <= twin.SPECTRUM_FACTOR * e["rho"], e["name"]
        assert e["kind"] == "flat" or dlog < 0.1


def test_twiddle_table_is_the_hosts():
    tw = st.TW
    assert tw.dtype == F and tw.shape == (2048, 2) and tuple(tw[0]) == (1.0, 0.0) and tuple(tw[1024]) == (0.0, -1.0)
    k = np.arange(2048)
    exact = np.exp(-2j * np.pi * k / 4096.0)
    assert np.abs(tw[:, 0] - exact.real).max() <= st.U and np.abs(tw[:, 1] - exact.imag).max() <= st.U      # each component rounded once
    assert np.array_equal(tw[512], F([np.sqrt(0.5), -np.sqrt(0.5)]))


# ------------------------------------------------------------------------------------------------------------------------------ decode
def test_decode_fp32_within_the_float64_bound_with_the_same_count():
    seen = {"negzero": 0, "nan": 0, "zero": 0}
    for name, (low, res) in st.decode_cases().items():
        out, nonpos = st.decode_fp32(low, res)
        d, E, v, Ev, want = twin.decode_ref(low, res)
        assert out.dtype == F and out.shape == res.shape
        ok = ~np.isnan(want)
        assert np.array_equal(np.isnan(out), ~ok), name
        worst = float((np.abs(out.astype(np.float64) - want)[ok] / np.maximum(Ev[ok], 1e-300)).max())
        print(f"decode {name:18s} {out.size:6d} elements  worst err / Ev {worst:.3f}  nonpos {nonpos}")
        assert (np.abs(out.astype(np.float64) - want)[ok] <= Ev[ok]).all(), (name, worst)
        assert nonpos == int((v <= 0).sum()), name
        seen["negzero"] += int((np.signbit(out) & (out == 0)).sum())
        seen["nan"] += int(np.isnan(out).sum())
        seen["zero"] += int(((out == 0) & (v == 0)).sum())
    assert all(seen.values()), seen                        # the edge values are there: -0.0, NaN, an exact cancellation


# ------------------------------------------------------------------------------------------------------------------------------ power
def _split_scale(x, s, k):
    """the second row of pair 0 scaled by (1 + 2^-s) in the split, at column k of the row spectra (None: at every column)"""
    re, im = st.rows_fp32(x)
    sel = slice(None) if k is None else k
    re[1, sel] *= F(1.0 + 2.0 ** -s)
    im[1, sel] *= F(1.0 + 2.0 ** -s)
    return st.as_complex(*st.cols_fp32(re, im))


def _column_rotated(x, theta, k):
    """column k of the half spectrum rotated by theta rad"""
    z = st.fft2_fp32(x)
    z[:, k] = (z[:, k].astype(np.complex128) * np.exp(1j * theta)).astype(np.complex64)
    return z


def _table_entry_off(x, entry, delta):
    """one entry of the twiddle table wrong by delta in its real part (an entry only the column pass's last stage reads)"""
    table = st.TW.copy()
    table[entry, 0] += F(delta)
    return st.as_complex(*st.cols_fp32(*st.rows_fp32(x, table=table), table=table))


def _store_truncated(x, r, k, nbits):
    """one coefficient stored without its low nbits mantissa bits"""
    z = st.fft2_fp32(x)
    v = z.view(F).reshape(z.shape + (2,)).view(np.int32)
    v[r, k] &= ~((1 << nbits) - 1)
    return z


def _twiddle_index_off(x, axis, j):
    """the last stage of one pass takes the table entry of j + 1 for a single j"""
    n = x.shape[1 - axis]
    bits = st.bits_of(n)

    def index(t, idx):
        if t == bits:
            idx = idx.copy()
            idx[j] += st.MAX_N >> t
        return idx
    if axis == 0:
        return st.as_complex(*st.cols_fp32(*st.rows_fp32(x, index)))
    return st.as_complex(*st.cols_fp32(*st.rows_fp32(x), index))


def _nyquist_sign(x):
    """the sign of the imaginary part of the second rows' coefficient at k = W / 2"""
    re, im = st.rows_fp32(x)
    im[1::2, -1] = -im[1::2, -1]
    return st.as_complex(*st.cols_fp32(re, im))


# (variant, committed case, fault): each passes both old criteria and moves a coefficient beyond E
SLIPS = (
    ("split_scale_2^-16_at_nyquist", "cosine_128x16", lambda x: _split_scale(x, 16, x.shape[1] // 2)),
    ("column_rotated_1e-5_rad", "cosine_128x16", lambda x: _column_rotated(x, 1e-5, 4)),
    ("table_entry_off_2^-16", "cosine_128x16", lambda x: _table_entry_off(x, 5 * 32, 2.0 ** -16)),
    ("store_truncated_8_bits", "cosine_16", lambda x: _store_truncated(x, 5, 6, 8)),
    ("coefficient_rotated_6e-6_rad", "batch3_a", lambda x: _one_rotated(x, 6e-6, 7, 11)),
)
# (candidate, committed case, fault): the issue's candidates as stated; the old criteria catch them (or the fault changes nothing)
CAUGHT = (
    ("split_scale_2^-12", "cosine_128x16", lambda x: _split_scale(x, 12, None)),
    ("split_scale_2^-12", "noise_8x4096", lambda x: _split_scale(x, 12, None)),
    ("column_rotated_1e-3_rad", "cosine_128x16", lambda x: _column_rotated(x, 1e-3, 5)),
    ("column_rotated_1e-3_rad", "noise_4096x8", lambda x: _column_rotated(x, 1e-3, 4)),
    ("twiddle_index_off_by_one_rows", "noise_8x4096", lambda x: _twiddle_index_off(x, 0, 1025)),
    ("twiddle_index_off_by_one_cols", "noise_4096x8", lambda x: _twiddle_index_off(x, 1, 1025)),
    ("twiddle_index_off_by_one_rows", "terrain_256", lambda x: _twiddle_index_off(x, 0, 65)),
)


def _one_rotated(x, theta, r, k):
    """one coefficient rotated by theta rad"""
    z = st.fft2_fp32(x)
    z[r, k] = np.complex64(complex(z[r, k]) * np.exp(1j * theta))
    return z


@pytest.fixture(scope="module")
def refs(cases, planes):
    """(x, F64, E, rho, bits of the restatement) of the cases the variants run on, computed once"""
    rho = {e["name"]: e["rho"] for e in cases["spectrum"]}
    out = {}
    for name in {c[1] for c in SLIPS + CAUGHT}:
        x = planes[name]
        out[name] = (x, twin.half_of(twin.spectrum(x)), st.fft2_bound(x), rho[name], st.int_view(st.fft2_fp32(x)))
    return out


@pytest.mark.parametrize("variant,case", [c[:2] for c in SLIPS])
def test_a_seeded_fault_passes_the_old_criteria_and_is_flagged_element_wise(refs, variant, case):
    fault = next(c[2] for c in SLIPS if c[:2] == (variant, case))
    x, f64, E, rho, want_bits = refs[case]
    z = fault(x)
    ratio, dlog = old_criteria(z, f64, rho)
    excess = np.abs(z.astype(np.complex128) - f64) / E
    differing = int((st.int_view(z) != want_bits).any(-1).sum())
    print(f"power {variant:30s} {case:14s} rel L2 / rho {ratio:.2f} (bound 4)  max |d log|F|| {dlog:.1e} (bound 0.1)  "
          f"worst err / E {float(excess.max()):.2f} at {int((excess > 1).sum())} coefficients  differing bits at {differing}")
    assert ratio <= twin.SPECTRUM_FACTOR and dlog < 0.1                # the old criteria pass
    assert excess.max() > 1.0                                          # the element-wise bound fails
    assert differing >= int((excess > 1).sum()) >= 1                   # and so does the bit comparison, at those coefficients at least
    assert (st.int_view(z) != want_bits).any(-1)[excess > 1].all()


@pytest.mark.parametrize("k", range(len(CAUGHT)))
def test_the_issues_candidates_as_stated_are_caught_by_the_old_criteria(refs, k):
    variant, case, fault = CAUGHT[k]
    x, f64, E, rho, want_bits = refs[case]
    ratio, dlog = old_criteria(fault(x), f64, rho)
    print(f"caught {variant:30s} {case:14s} rel L2 / rho {ratio:.1f} (bound 4)  max |d log|F|| {dlog:.1e}")
    assert ratio > twin.SPECTRUM_FACTOR


def test_the_nyquist_sign_candidate_changes_no_value(planes):
    # (z.y - c.y) and (c.x - z.x) at k = W / 2 subtract a value from itself: the imaginary parts are exact zeros and their sign decides nothing
    for name in ("noise_64", "cosine_128x16", "batch3_c"):
        x = planes[name]
        re, im = st.rows_fp32(x)
        assert (im[:, -1] == 0).all() and (im[:, 0] == 0).all()
        assert np.array_equal(_nyquist_sign(x), st.fft2_fp32(x))
