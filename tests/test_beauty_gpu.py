"""The beauty score on the GPU (include/td_spectrum.h, spectrum_csrc/spectrum_kernels.hip), every result against the float64 twin
(tests/_beauty_twin.py) within the bounds its docstring derives, never against the code under test: the spectrum within 4 rho_ref in relative
L2 (phases too for the impulse and the cosine), the ring means per bin with exact counts and exactly -inf for the flat plane, the decode per
element with an exact count of pixels <= 0 and std within one ulp, the score within the propagated bound with the reference's class and early
return, NaN -> 1.0, two runs and the enqueue-only mode bit for bit, prepare_chunks with and without the option, and the C-ABI's refusals.

Measured on an MI355X (relative L2 error of the half spectrum over rho_ref, the bound being 4): see DESIGN.md, "Beauty scores"."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _beauty_twin as twin
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def bt():
    from terrain_diffusion_amd import beauty
    assert torch.cuda.is_available()
    return beauty


@pytest.fixture(scope="module")
def eng():
    from terrain_diffusion_amd.engine import get_engine
    return get_engine("cuda")


@pytest.fixture(scope="module")
def cases(golden):
    return json.loads(str(golden("beauty")["cases"]))


@pytest.fixture(scope="module")
def planes():
    return twin.spectrum_planes()


@pytest.fixture(scope="module")
def f64(planes):
    """the float64 spectrum of every committed plane, computed once and left unchanged"""
    return {name: twin.spectrum(x) for name, x in planes.items()}


@pytest.fixture(scope="module")
def score_refs(cases):
    out = {}
    for e in cases["score"]:
        low, res = twin.score_inputs(e["name"])
        out[e["name"]] = (low, res, twin.score_ref(low, res, e["rho"]))
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype in (torch.float32, torch.int32) else torch.int64).numpy()


def rel_l2(got, want):
    return float(np.sqrt((np.abs(got - want) ** 2).sum() / (np.abs(want) ** 2).sum()))


# ------------------------------------------------------------------------------------------------------------------------------ spectrum
def test_half_spectrum_within_four_rho_of_float64(bt, cases, planes, f64):
    for e in cases["spectrum"]:
        x = planes[e["name"]]
        half, logabs = bt.fft2(dev(x), spectrum=True, logabs=True)
        assert half.dtype == torch.complex64 and tuple(half.shape) == (e["H"], e["W"] // 2 + 1) and half.is_cuda
        assert logabs.dtype == torch.float32 and tuple(logabs.shape) == (e["H"], e["W"])
        got, want = half.cpu().numpy().astype(np.complex128), twin.half_of(f64[e["name"]])
        err = rel_l2(got, want)
        print(f"spectrum {e['name']:14s} rel L2 {err:.3e}  rho_ref {e['rho']:.3e}  ratio {err / e['rho'] if e['rho'] else 0.0:.2f} (bound 4)")
        assert err <= twin.SPECTRUM_FACTOR * e["rho"], (e["name"], err, e["rho"])
        if e["kind"] == "impulse":
            # |F| = 1 everywhere and the phase is that of two twiddles: a coefficient is the impulse times one twiddle per stage (the other
            # operand of every sum is zero), each product within sqrt(5) u < 4 u of its magnitude, log2(H W) stages
            stages = np.log2(e["H"] * e["W"])
            assert np.abs(np.abs(got) - 1.0).max() <= 4 * twin.U * stages
            assert np.abs(np.angle(got * np.conj(want))).max() <= 4 * twin.U * stages
        if e["kind"] == "cosine":
            # the mode (2, 3) is N / 2 e^{0.7 i} beside the impulse's unit coefficient; one coefficient errs by no more than all of them do
            n = e["H"] * e["W"]
            room = twin.SPECTRUM_FACTOR * e["rho"] * float(np.sqrt((np.abs(want) ** 2).sum())) / abs(want[2, 3])
            assert abs(abs(got[2, 3]) / abs(want[2, 3]) - 1.0) <= room and abs(np.angle(got[2, 3] * np.conj(want[2, 3]))) <= room * (1 + room)
            assert abs(np.angle(want[2, 3]) - 0.7) < 4.0 / n and abs(want[2, 3]) > 0.45 * n
        # log|F| at every position of the full plane, the second half of each row by Hermitian symmetry
        la = logabs.cpu().numpy().astype(np.float64)
        with np.errstate(divide="ignore"):
            want_la = np.log(np.abs(f64[e["name"]]))
        if e["kind"] == "flat":
            assert la[0, 0] == F(np.log(7.5 * 256)) and np.isneginf(np.delete(la.ravel(), 0)).all()
        else:
            full = np.concatenate([got, np.conj(np.roll(got[::-1], 1, 0)[:, 1:e["W"] // 2][:, ::-1])], axis=1)
            assert full.shape == want_la.shape
            with np.errstate(divide="ignore"):
                own = np.log(np.abs(full))                 # log of the device's own spectrum in float64: the kernel rounds it once
            # one rounding to fp32, and 2^-52 of |F|^2 either way in float64, which the logarithm hands on as it is
            assert np.isfinite(own).all() and (np.abs(la - own) <= twin.ulp32(own) + 2.0 ** -50 * np.maximum(1.0, np.abs(own))).all(), e["name"]
            assert np.abs(la - want_la).max() < 0.1


def test_batch_of_unlike_planes_and_the_optional_outputs(bt, planes, f64, cases):
    rho = {e["name"]: e["rho"] for e in cases["spectrum"]}
    x = dev(np.stack([planes[n] for n in twin.BATCH3]))
    half, logabs = bt.fft2(x, spectrum=True, logabs=True)
    assert tuple(half.shape) == (3, 32, 33) and tuple(logabs.shape) == (3, 32, 64)
    for k, n in enumerate(twin.BATCH3):
        assert rel_l2(half[k].cpu().numpy().astype(np.complex128), twin.half_of(f64[n])) <= twin.SPECTRUM_FACTOR * rho[n], n
        alone = bt.fft2(dev(planes[n]), spectrum=True, logabs=True)
        assert torch.equal(torch.view_as_real(alone[0]), torch.view_as_real(half[k])) and torch.equal(alone[1], logabs[k])
    only_half, none = bt.fft2(x, spectrum=True, logabs=False)
    none2, only_log = bt.fft2(x, spectrum=False, logabs=True)
    assert none is None and none2 is None
    assert torch.equal(torch.view_as_real(only_half), torch.view_as_real(half)) and torch.equal(only_log, logabs)
    # radial_spectrum hands the same half spectrum out on request, beside the same ring means
    centres, means, spec = bt.radial_spectrum(x, 4, return_spectrum=True)
    assert torch.equal(torch.view_as_real(spec), torch.view_as_real(half)) and torch.equal(means, bt.radial_spectrum(x, 4)[1])
    assert torch.equal(means, bt.radial_bins(logabs, 4)[1]) and tuple(means.shape) == (3, 4) and len(centres) == 4


# ------------------------------------------------------------------------------------------------------------------------------ ring means
def test_ring_means_within_the_pushed_through_bound_and_exact_counts(bt, golden, cases, planes):
    g = golden("beauty")
    for e in cases["spectrum"]:
        x = planes[e["name"]]
        for bins in twin.BINS:
            counts, want, bound = twin.bin_means(x, bins, rho=e["rho"])
            centres, means = bt.radial_spectrum(dev(x), bins)
            _, la = bt.fft2(dev(x), spectrum=False, logabs=True)
            got_counts, got_means = bt.radial_bins(la[None], bins)
            assert means.dtype == torch.float32 and tuple(means.shape) == (bins,) and torch.equal(got_means[0], means)
            assert np.array_equal(got_counts.cpu().numpy()[0], counts) and np.array_equal(counts, g[f"counts{bins}_{e['name']}"])
            assert np.allclose(centres.numpy(), (np.arange(bins) + 0.5) / bins, atol=1e-6)
            got = means.cpu().numpy().astype(np.float64)
            if e["kind"] == "flat":
                assert np.isneginf(got[counts > 0]).all() and (got[counts == 0] == 0.0).all() and (counts > 0).sum() >= 3
                continue
            print(f"ring means {e['name']:14s} bins {bins}: worst |gpu - D64| / bound {float(np.max(np.abs(got - want)[counts > 0] / bound[counts > 0])):.3f}")
            assert (np.abs(got - want) <= bound).all(), (e["name"], bins, got - want, bound)
            assert (got[counts == 0] == 0.0).all()


def test_infinities_and_nans_propagate_and_an_empty_ring_gives_zero(bt):
    ring = bt.host_bin_map(8, 8, 64).numpy()                # 64 rings over an 8 x 8 plane: most are empty
    members = np.argwhere(ring != bt.NO_BIN)
    r0, c0 = members[0]
    r1, c1 = next(m for m in members if ring[m[0], m[1]] != ring[r0, c0])
    la = torch.ones(2, 8, 8, device="cuda")
    la[0, r0, c0] = float("inf")
    la[1, r1, c1] = float("nan")
    counts, means = bt.radial_bins(la, 64)
    c, m = counts.cpu().numpy(), means.cpu().numpy()
    assert np.array_equal(c[0], c[1]) and np.array_equal(c[0], np.bincount(ring.ravel(), minlength=256)[:64]) and (c[0] == 0).sum() > 40
    assert (m[:, c[0] == 0] == 0.0).all() and m[0, ring[r0, c0]] == np.inf and np.isnan(m[1, ring[r1, c1]])
    rest = np.ones((2, 64), bool)
    rest[0, ring[r0, c0]] = rest[1, ring[r1, c1]] = False
    assert (m[rest & (c[0] > 0)[None]] == 1.0).all()


# ------------------------------------------------------------------------------------------------------------------------------ decode
def test_decode_every_element_within_the_bound_exact_count_and_std(bt, score_refs):
    for name, (low, res, ref) in score_refs.items():
        d, E, v, Ev, out = twin.decode_ref(low, res)
        got, stats = bt.decode_terrain(dev(low), dev(res), return_stats=True)
        assert got.dtype == torch.float32 and tuple(got.shape) == res.shape and got.is_cuda
        g = got.cpu().numpy().astype(np.float64)
        assert (np.abs(g - out) <= Ev).all(), (name, float((np.abs(g - out) / np.maximum(Ev, 1e-300)).max()))
        assert (g >= 0).all() and ((g == 0) == (v <= 0)).all()
        assert int(stats["nonpos"].cpu()) == ref["nonpos"] == int((v <= 0).sum()), name
        # the moments against float64 NumPy on the very plane the device wrote: count / mean / centred squares, and the std rounded once
        n = g.size
        mean, m2, std = float(stats["mean"].cpu()), float(stats["m2"].cpu()), stats["std"].cpu().numpy()[0]
        assert abs(mean - g.mean()) <= 4.0 * n * 2.0 ** -53 * np.abs(g).mean()
        assert abs(m2 - ((g - g.mean()) ** 2).sum()) <= 8.0 * n * 2.0 ** -53 * ((g - g.mean()) ** 2).sum()
        assert std.dtype == F and abs(float(std) - twin.std_ref(g)) <= float(twin.ulp32(twin.std_ref(g))), name
        assert abs(float(std) - ref["std"]) <= ref["std_bound"], name
    # a batch with its own stride, planes given one at a time
    names = [n for n in score_refs if n.endswith("_64")]
    lows, ress = dev(np.stack([score_refs[n][0] for n in names])), dev(np.stack([score_refs[n][1] for n in names]))
    got, stats = bt.decode_terrain(lows, ress, return_stats=True)
    for k, n in enumerate(names):
        one, s1 = bt.decode_terrain(lows[k], ress[k], return_stats=True)
        assert torch.equal(got[k], one) and all(torch.equal(stats[key][k:k + 1], s1[key]) for key in ("nonpos", "mean", "m2", "std"))


def test_decode_handles_exact_zeros_negatives_and_sizes_off_the_tile(bt):
    low = np.array([[-2.0, 0.0, 3.0], [0.0, 0.0, 1.0]], F)
    res = np.zeros((5, 7), F)
    res[0, 0] = 2.0
    d, E, v, Ev, out = twin.decode_ref(low, res)
    got, stats = bt.decode_terrain(dev(low), dev(res), return_stats=True)
    g = got.cpu().numpy().astype(np.float64)
    assert (np.abs(g - out) <= Ev).all() and int(stats["nonpos"].cpu()) == int((v <= 0).sum()) and (v == 0).sum() >= 4 and (v < 0).sum() >= 2


# ------------------------------------------------------------------------------------------------------------------------------ score
def test_score_within_the_propagated_bound_with_the_references_class(bt, cases, score_refs):
    for e in cases["score"]:
        low, res, ref = score_refs[e["name"]]
        got = bt.calculate_beauty_score(low, res)
        assert isinstance(got, float)
        if e["share"] > 0.99:
            assert got == 1.0 == e["score"] and ref["share"] > 0.99
            continue
        means, std, ocean = bt.beauty_features(dev(low)[None], dev(res)[None])
        assert tuple(means.shape) == (1, 4) and tuple(std.shape) == (1,) and ocean.dtype == torch.bool and not bool(ocean[0])
        assert (np.abs(means.cpu().numpy()[0].astype(np.float64) - ref["powers"]) <= ref["power_bounds"]).all(), e["name"]
        print(f"score {e['name']:14s} gpu {got:.9f} twin {ref['score']:.9f} reference {e['score']:.9f} bound {ref['score_bound']:.3e}")
        assert abs(got - ref["score"]) <= ref["score_bound"], (e["name"], got, ref["score"], ref["score_bound"])
        assert got == bt.score_from_features(means.cpu().numpy()[0].tolist(), float(std.cpu()[0]))
        assert bt.beauty_class(got) == bt.beauty_class(e["score"]), e["name"]
    ocean = bt.beauty_features(dev(score_refs["ocean995_64"][0]), dev(score_refs["ocean995_64"][1]))[2]
    assert bool(ocean[0]) and not bool(bt.beauty_features(dev(score_refs["ocean98_64"][0]), dev(score_refs["ocean98_64"][1]))[2][0])


def test_assign_beauty_scores_batches_by_shape_keeps_the_order_and_maps_nan_to_one(bt, cases, score_refs):
    groups = {}
    for e in cases["score"]:
        low, res, _ = score_refs[e["name"]]
        groups["512/0/" + e["name"]] = {"lowfreq": low, "residual": res}
    nan_res = score_refs["score_64"][1].copy()
    nan_res[5, 9] = np.nan
    groups["512/1/nan"] = {"lowfreq": score_refs["score_64"][0], "residual": nan_res}
    order = list(groups)[::-1]
    scores = bt.assign_beauty_scores({p: groups[p] for p in order})
    assert list(scores) == order and scores["512/1/nan"] == 1.0
    for e in cases["score"]:
        assert scores["512/0/" + e["name"]] == bt.calculate_beauty_score(*score_refs[e["name"]][:2]), e["name"]      # batched or alone: the same bits
    assert np.isnan(bt._scores(dev(score_refs["score_64"][0])[None], dev(nan_res)[None], None)[0])


# ------------------------------------------------------------------------------------------------------------------------------ determinism
def _everything(bt, inputs):
    x, low, res = inputs
    half, logabs = bt.fft2(x, spectrum=True, logabs=True)
    counts, means = bt.radial_bins(logabs, 7)
    decoded, stats = bt.decode_terrain(low, res, return_stats=True)
    feats = bt.beauty_features(low, res)
    return [torch.view_as_real(half), logabs, counts, means, decoded, stats["nonpos"], stats["mean"], stats["m2"], stats["std"], feats[0], feats[1]]


def test_two_runs_and_the_enqueue_only_mode_give_the_same_bits(bt, eng, planes, score_refs):
    low, res, _ = score_refs["score_256"]
    inputs = [dev(planes["terrain_256"])[None].repeat(2, 1, 1), dev(low)[None], dev(res)[None]]
    ref = _everything(bt, inputs)
    again = _everything(bt, inputs)
    for a, b in zip(ref, again):
        assert np.array_equal(bits(a), bits(b))
    s = torch.cuda.Stream()
    with eng.on_stream(s, asynchronous=True):
        x = [t.clone() for t in inputs]                   # produced on the caller's stream, consumed there without a host sync
        got = [t.clone() for t in _everything(bt, x)]     # read on that stream after the calls
    torch.cuda.current_stream().synchronize()
    for a, b in zip(got, ref):
        assert np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------------------ prepare_chunks
def test_prepare_chunks_with_scores_and_unchanged_without(bt):
    from terrain_diffusion_amd import dataset as ds
    t = twin.terrain(128, 128, 31, 0.75).astype(F)
    dem = t.copy()
    dem[40:50, 60:75] = np.nan
    base = (t * 0.5).astype(F)
    plain = ds.prepare_chunks(dem, base, 16, 2.0, 2, chunk_id="9")
    scored = ds.prepare_chunks(dem, base, 16, 2.0, 2, chunk_id="9", beauty_scores=True)
    # the default is the call as it was before the option existed: the device forms in the reference's order, key by key
    filled = ds.fill_voids(dem, base, 32, True)
    exact = ds.block_median(filled, 8)
    res, low = ds.laplacian_encode(filled, 16, 2.0)
    counts = ds.land_counts(low, 2).cpu().numpy().reshape(-1)
    assert len(plain) == len(scored) == 4
    for k, (p, s) in enumerate(zip(plain, scored)):
        i, j = divmod(k, 2)
        assert set(p) == {"residual", "lowfreq", "lowres_exact", "pct_land", "chunk_id", "subchunk_id"} and set(s) == set(p) | {"beauty_score"}
        want = {"residual": res[64 * i:64 * i + 64, 64 * j:64 * j + 64], "lowfreq": low[8 * i:8 * i + 8, 8 * j:8 * j + 8],
                "lowres_exact": exact[8 * i:8 * i + 8, 8 * j:8 * j + 8]}
        for key, w in want.items():
            assert np.array_equal(bits(p[key]), bits(w)) and np.array_equal(bits(s[key]), bits(w)), (k, key)
        assert p["pct_land"] == s["pct_land"] == float(counts[k]) / 64.0 and (p["chunk_id"], p["subchunk_id"]) == ("9", f"chunk_{i}_{j}") == (s["chunk_id"], s["subchunk_id"])
        assert isinstance(s["beauty_score"], float) and s["beauty_score"] == bt.calculate_beauty_score(s["lowfreq"], s["residual"])
    assert len({s["beauty_score"] for s in scored}) >= 2
    with pytest.raises(NotImplementedError, match="powers of two"):
        ds.prepare_chunks(dem[:96, :96], base[:96, :96], 12, 2.0, 1, beauty_scores=True)


# ------------------------------------------------------------------------------------------------------------------------------ the C ABI
def test_c_abi_argument_errors(bt, eng):
    st = C.c_void_p(eng.stream)
    l = bt.lib()
    dp = lambda t: C.c_void_p(t.data_ptr())
    x, out = torch.zeros(2, 16, 16, device="cuda"), torch.empty(2, 16, 16, device="cuda")
    half = torch.empty(2, 16, 9, 2, device="cuda")
    low = torch.zeros(2, 4, 4, device="cuda")
    i32, f64, f32 = (torch.empty(8, dtype=t, device="cuda") for t in (torch.int32, torch.float64, torch.float32))
    m = torch.zeros(16, 16, dtype=torch.uint8, device="cuda")
    host = torch.zeros(2, 16, 16)
    sized = [
        lambda: l.td_spectrum_fft2(st, dp(x), 2, 12, 16, dp(half), dp(out), 1),
        lambda: l.td_spectrum_fft2(st, dp(x), 2, 16, 4, dp(half), dp(out), 1),
        lambda: l.td_spectrum_fft2(st, dp(x), 1, 8192, 8, dp(half), dp(out), 1),
        lambda: l.td_spectrum_fft2(st, dp(x), 1, 16, 24, None, dp(out), 1),
    ]
    for k, f in enumerate(sized):
        assert f() == -3 and "power of two" in bt._LIB.error_text(), k
    bad = [
        lambda: l.td_spectrum_fft2(st, dp(x), 0, 16, 16, dp(half), dp(out), 1),
        lambda: l.td_spectrum_fft2(st, dp(x), 1025, 16, 16, dp(half), dp(out), 1),
        lambda: l.td_spectrum_fft2(st, None, 2, 16, 16, dp(half), dp(out), 1),
        lambda: l.td_spectrum_fft2(st, dp(x), 2, 16, 16, None, None, 1),
        lambda: l.td_spectrum_fft2(st, dp(host), 2, 16, 16, dp(half), dp(out), 1),
        lambda: l.td_spectrum_fft2(st, dp(x), 2, 16, 16, dp(half), dp(host), 1),
        lambda: l.td_spectrum_fft2(st, dp(x), 2, 16, 16, dp(half), dp(x), 1),
        lambda: l.td_spectrum_decode(st, dp(low), dp(x), 0, 16, 16, 4, 4, dp(out), dp(i32), dp(f64), dp(f64), dp(f32), 1),
        lambda: l.td_spectrum_decode(st, dp(low), dp(x), 2, 4097, 16, 4, 4, dp(out), dp(i32), dp(f64), dp(f64), dp(f32), 1),
        lambda: l.td_spectrum_decode(st, dp(low), dp(x), 2, 16, 16, 0, 4, dp(out), dp(i32), dp(f64), dp(f64), dp(f32), 1),
        lambda: l.td_spectrum_decode(st, dp(low), dp(x), 1, 1, 1, 4, 4, dp(out), dp(i32), dp(f64), dp(f64), dp(f32), 1),
        lambda: l.td_spectrum_decode(st, None, dp(x), 2, 16, 16, 4, 4, dp(out), dp(i32), dp(f64), dp(f64), dp(f32), 1),
        lambda: l.td_spectrum_decode(st, dp(low), dp(x), 2, 16, 16, 4, 4, dp(out), None, dp(f64), dp(f64), dp(f32), 1),
        lambda: l.td_spectrum_decode(st, dp(low), dp(host), 2, 16, 16, 4, 4, dp(out), dp(i32), dp(f64), dp(f64), dp(f32), 1),
        lambda: l.td_spectrum_decode(st, dp(low), dp(x), 2, 16, 16, 4, 4, dp(x), dp(i32), dp(f64), dp(f64), dp(f32), 1),
        lambda: l.td_spectrum_radial_bins(st, dp(x), dp(m), 2, 16, 16, 0, dp(i32), dp(f32), 1),
        lambda: l.td_spectrum_radial_bins(st, dp(x), dp(m), 2, 16, 16, 65, dp(i32), dp(f32), 1),
        lambda: l.td_spectrum_radial_bins(st, dp(x), dp(m), 2, 0, 16, 4, dp(i32), dp(f32), 1),
        lambda: l.td_spectrum_radial_bins(st, dp(x), None, 2, 16, 16, 4, dp(i32), dp(f32), 1),
        lambda: l.td_spectrum_radial_bins(st, dp(x), dp(m), 2, 16, 16, 4, dp(i32), dp(host), 1),
    ]
    for k, f in enumerate(bad):
        assert f() == -1 and bt._LIB.error_text().startswith("td_spectrum_"), k
    with pytest.raises(NotImplementedError):
        bt.fft2(torch.zeros(12, 16, device="cuda"))
    # a refused call leaves the library usable
    assert l.td_spectrum_fft2(st, dp(x), 2, 16, 16, dp(half), dp(out), 1) == 0
    assert float(half[0, 0, 0, 0]) == 0.0 and torch.isneginf(out).all()
