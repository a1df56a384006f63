"""The beauty score without a GPU: the bin map against the ring sizes the fixture records (tests/golden/beauty.npz), the host score arithmetic
against the reference's recorded score bit for bit, the class rule on its edges, the float64 twin (tests/_beauty_twin.py) against what the
reference recorded within the twin's stated bounds, the argument checks, which refuse before an engine exists, and the header against the
binding."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _beauty_twin as twin
from terrain_diffusion_amd import beauty as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def cases(golden):
    return json.loads(str(golden("beauty")["cases"]))


@pytest.fixture(scope="module")
def planes():
    return twin.spectrum_planes()


# ------------------------------------------------------------------------------------------------------------------------------ the fixture
def test_the_committed_cases_are_the_recorded_ones(golden, cases, planes):
    g = golden("beauty")
    assert [e["name"] for e in cases["spectrum"]] == [c[0] for c in twin.SPECTRUM_CASES] and tuple(cases["bins"]) == twin.BINS
    assert [e["name"] for e in cases["score"]] == [c[0] for c in twin.SCORE_CASES]
    shapes = {(e["H"], e["W"]) for e in cases["spectrum"]}
    assert {(8, 8), (16, 16), (64, 64), (256, 256), (8, 64), (128, 16), (4096, 8), (8, 4096), (1024, 1024)} <= shapes
    for e in cases["spectrum"]:
        x = planes[e["name"]]
        assert x.dtype == F and x.shape == (e["H"], e["W"]) and twin.crc(x) == e["crc"], e["name"]
        if x.size <= 4096:
            assert np.array_equal(x.view(np.uint32), g["in_" + e["name"]].view(np.uint32))
        assert 0.0 <= e["rho"] < 2e-7
    for e in cases["score"]:
        low, res = twin.score_inputs(e["name"])
        assert twin.crc(low, res) == e["crc"] and not 0.98 <= e["share"] <= 0.995, e["name"]
    assert sorted(round(e["share"], 2) for e in cases["score"])[-2:] == [0.98, 1.0]         # one either side of the ocean rule


def test_bin_map_ring_sizes_equal_the_recorded_ones(golden, cases):
    g = golden("beauty")
    for e in cases["spectrum"]:
        for bins in twin.BINS:
            m = bt.host_bin_map(e["H"], e["W"], bins)
            assert m.dtype == torch.uint8 and tuple(m.shape) == (e["H"], e["W"])
            got = np.bincount(m.numpy().ravel(), minlength=256)
            assert np.array_equal(got[:bins], g[f"counts{bins}_{e['name']}"]), (e["name"], bins)
            assert got[bins:255].sum() == 0 and got[255] == m.numel() - got[:bins].sum() > 0.15 * m.numel()      # the corners are in no ring
            # the package un-shifts the map where the twin shifts the spectrum: the same members
            shifted = np.fft.fftshift(m.numpy())
            for k, mask in enumerate(twin.bin_masks(e["H"], e["W"], bins)):
                assert np.array_equal(shifted == k, mask)
    # (0, 0) is DC, the centre of the shifted plane; (8, 8) is the shifted plane's corner (-1, -1), outside the unit circle
    assert int(bt.host_bin_map(16, 16, 4)[0, 0]) == 0 and int(bt.host_bin_map(16, 16, 4)[8, 8]) == bt.NO_BIN


def test_host_score_arithmetic_gives_the_recorded_score_bit_for_bit(golden, cases):
    g = golden("beauty")
    checked = 0
    for e in cases["score"]:
        if e["share"] > 0.99:
            assert e["score"] == 1.0
            continue
        f = g["features_" + e["name"]]
        got = bt.score_from_features(f[:4].tolist(), float(f[4]))
        assert isinstance(got, float) and np.float64(got).view(np.uint64) == np.float64(e["score"]).view(np.uint64), (e["name"], got, e["score"])
        assert float(f[4]) == e["std"]
        checked += 1
    assert checked == 4
    assert bt.COEFFICIENTS == twin.COEFFICIENTS and bt.INTERCEPT == twin.INTERCEPT and len(bt.COEFFICIENTS) == 7


def test_beauty_class_on_the_bucket_edges():
    want = {-3.0: 0, 0.4: 0, 1.0: 0, 1.49: 0, 1.5: 1, 1.51: 1, 2.49: 1, 2.5: 1, 2.51: 2, 3.5: 3, 3.51: 3, 4.49: 3, 4.5: 3, 4.51: 4, 5.0: 4, 5.5: 4, 9.0: 4}
    for score, cls in want.items():                        # Python rounds halves to even: 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, 4.5 -> 4
        assert bt.beauty_class(score) == cls == max(1, min(5, round(score))) - 1, score


# ------------------------------------------------------------------------------------------------------------------------------ the twin
def test_the_twin_agrees_with_the_recorded_reference_within_its_bounds(golden, cases, planes):
    g = golden("beauty")
    for e in cases["spectrum"]:
        x = planes[e["name"]]
        for bins in twin.BINS:
            counts, means, bounds = twin.bin_means(x, bins, rho=e["rho"])
            want = g[f"powers{bins}_{e['name']}"]
            assert np.array_equal(counts, g[f"counts{bins}_{e['name']}"])
            if e["kind"] == "flat":
                assert (want[counts > 0] == -np.inf).all() and (means[counts > 0] == -np.inf).all() and (want[counts == 0] == 0).all()
                continue
            # the reference sums its log|F| in fp32: half an ulp per term of the mean's magnitude, pairwise
            slack = 8.0 * twin.ulp32(np.abs(want).max())
            assert (np.abs(means - want) <= bounds + slack).all(), (e["name"], bins, means - want, bounds)
    for e in cases["score"]:
        low, res = twin.score_inputs(e["name"])
        ref = twin.score_ref(low, res, e["rho"])
        assert abs(ref["share"] - e["share"]) < 1e-6 and (ref["share"] > 0.99) == (e["score"] == 1.0 and e["share"] > 0.99)
        if e["share"] > 0.99:
            continue
        assert abs(ref["std"] - e["std"]) <= 64 * float(twin.ulp32(e["std"])) + ref["std_bound"]        # torch.std accumulates in fp32
        assert abs(ref["score"] - e["score"]) <= ref["score_bound"], (e["name"], ref["score"], e["score"], ref["score_bound"])
        assert abs(e["score"] - (np.floor(e["score"]) + 0.5)) > ref["score_bound"]            # the class does not hinge on the bound
        assert ref["score_bound"] < 1e-2


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_argument_checks_refuse_before_any_engine_is_touched(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(bt, "_engine_for", no_engine)
    for shape in ((12, 16), (16, 24), (4, 16), (16, 4), (8192, 8), (8, 8192)):
        x = torch.zeros(shape) if max(shape) <= 4096 else torch.zeros(1).expand(shape)
        if max(shape) > 4096:
            with pytest.raises(NotImplementedError, match="powers of two"):
                bt.radial_spectrum(x, 4)
            with pytest.raises(ValueError, match="limit"):
                bt.calculate_beauty_score(np.zeros((2, 2), F), x)
            continue
        with pytest.raises(NotImplementedError, match="powers of two"):
            bt.radial_spectrum(x, 4)
        with pytest.raises(NotImplementedError, match="powers of two"):
            bt.analyze_terrain_frequency(x.numpy(), 4)
        with pytest.raises(NotImplementedError, match="powers of two"):
            bt.calculate_beauty_score(np.zeros((2, 2), F), x.numpy())
        with pytest.raises(NotImplementedError, match="powers of two"):
            bt.assign_beauty_scores({"a": {"lowfreq": np.zeros((2, 2), F), "residual": x.numpy()}})
    with pytest.raises(ValueError, match="limit"):
        bt.decode_terrain(torch.zeros(2, 2), torch.zeros(1).expand(4097, 8))
    with pytest.raises(ValueError, match="one low band per residual plane"):
        bt.decode_terrain(torch.zeros(2, 4, 4), torch.zeros(3, 16, 16))
    with pytest.raises(ValueError, match="one low band per residual plane"):
        bt.beauty_features(torch.zeros(4, 4), torch.zeros(1, 16, 16))
    with pytest.raises(ValueError, match="one low band per residual plane"):
        bt.calculate_beauty_score(np.zeros((2, 4, 4), F), np.zeros((16, 16), F))
    for bad in (torch.zeros(5), torch.zeros(1, 2, 8, 8)):
        with pytest.raises(ValueError, match=r"\(H, W\) or \(B, H, W\)"):
            bt.radial_spectrum(bad, 4)
    for bins in (0, -1, 65, 255):
        with pytest.raises(ValueError, match=r"bins must be in 1 \.\. 64"):
            bt.radial_spectrum(torch.zeros(8, 8), bins)
    # the device forms take device tensors only
    with pytest.raises(ValueError, match="device tensor"):
        bt.decode_terrain(torch.zeros(2, 2), torch.zeros(16, 16))
    with pytest.raises(ValueError, match="device tensor"):
        bt.radial_spectrum(torch.zeros(16, 16), 4)
    with pytest.raises(ValueError, match="device tensor"):
        bt.radial_spectrum(np.zeros((16, 16), F), 4)
    with pytest.raises(ValueError, match="device tensor"):
        bt.beauty_features(torch.zeros(2, 2), torch.zeros(16, 16))
    with pytest.raises(ValueError, match=r"heightmap must be \(H, W\)"):
        bt.analyze_terrain_frequency(np.zeros((2, 8, 8), F), 4)


def test_prepare_chunks_option_is_keyword_only_and_off_by_default():
    import inspect
    from terrain_diffusion_amd import dataset as ds
    p = inspect.signature(ds.prepare_chunks).parameters["beauty_scores"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


# ------------------------------------------------------------------------------------------------------------------------------ the header
def test_header_entry_points_and_exports():
    import terrain_diffusion_amd as td
    import __graft_entry__ as ge
    text = open(os.path.join(ROOT, "include", "td_spectrum.h")).read()
    declared = set(re.findall(r"\b(td_spectrum_\w+)\s*\(", text))
    stated = {"td_spectrum_last_error", "td_spectrum_decode", "td_spectrum_fft2", "td_spectrum_radial_bins"}
    assert declared == set(bt.EXPORTS) == stated
    for name in stated - {"td_spectrum_last_error"}:
        params = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")
        assert len(params) == len(bt._SIGS[name][1]), name
        assert params[0].strip() == "void* hip_stream" and params[-1].strip() == "int synchronize", name
        for p, ctype in zip(params, bt._SIGS[name][1]):
            assert ("*" in p) == (ctype is bt._P), (name, p)
    for macro, value in (("MIN_SIDE", 8), ("MAX_SIDE", 4096), ("MAX_BATCH", 1024), ("MAX_BINS", 64), ("NO_BIN", 255)):
        assert re.search(rf"#define TD_SPECTRUM_{macro} {value}\b", text) and getattr(bt, macro) == value
    have = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", bt.LIB_PATH], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert stated <= have and not {n for n in have if n.startswith("td_") and n not in stated}
    assert not {n for n in subprocess.run(["nm", "-D", "--undefined-only", bt.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
                if "fft" in n.lower()}               # no rocFFT / hipFFT behind the C ABI
    bt.lib()     # binds every entry point
    for name in ("decode_terrain", "radial_spectrum", "beauty_features", "analyze_terrain_frequency", "calculate_beauty_score", "beauty_class",
                 "assign_beauty_scores"):
        assert getattr(td, name) is getattr(bt, name), name
    assert ge.SPECTRUM_LIBS == (("spectrum", "spectrum_csrc", "spectrum.hip", "td_spectrum.h", ("-ffp-contract=off",), "beauty"),)
    assert ge.ALL_SIDE_LIBS == ge.SIDE_LIBS + ge.DATA_LIBS + ge.SPECTRUM_LIBS and len(ge.ALL_SIDE_LIBS) == 9
    assert "spectrum" not in ge.SIDE_SHARED
    assert "PARITY-UNPINNED" in bt.__doc__ and "PARITY-UNPINNED" in twin.__doc__
