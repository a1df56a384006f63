"""Hydrology, host side (no GPU): the NumPy twin against every case recorded from the reference's postprocessing.py
(tests/golden/hydro.npz, tests/golden/make_hydro_golden.py), the fixtures' coverage of the branches, the C-ABI's exports, and the refusals
that come before any engine is touched."""
import json

import numpy as np
import pytest

import _hydro_twin as twin


def _cases(golden):
    g = golden("hydro")
    for c in json.loads(str(g["cases"])):
        yield c["name"], c["fn"], g[c["input"]], c["kwargs"], g


def test_twin_matches_every_recorded_case(golden):
    seen = {"fill": 0, "d8": 0, "acc": 0, "indicator": 0}
    for name, fn, z, kw, g in _cases(golden):
        if fn == "fill":
            got, _ = twin.fill(z, **kw)
            assert got.dtype == np.float32 and np.array_equal(got, g["out_" + name], equal_nan=True), name
            assert twin.fill_fixed_point_violations(z, g["out_" + name], **kw) == 0, name
        elif fn == "d8":
            r, k, s = twin.d8(z, **kw)
            assert np.array_equal(r, g["receiver_" + name]) and np.array_equal(k, g["kmax_" + name]) and np.array_equal(s, g["sink_" + name]), name
        elif fn == "acc":
            r, _, s = twin.d8(z)
            assert twin.uphill_edges(z, r, s) == 0, name
            assert np.array_equal(twin.accumulate(z, r, s), g["out_" + name]), name
            assert twin.accumulation_ok(z, r, s, g["out_" + name]), name
        else:
            r, _, s = twin.d8(z)
            assert np.array_equal(twin.indicator(twin.accumulate(z, r, s), kw.get("max_pool_kernel", 1)), g["out_" + name]), name
        seen[fn] += 1
    assert seen == {"fill": 13, "d8": 10, "acc": 9, "indicator": 7}


def test_recorded_cases_cover_the_branches(golden):
    c = {name: (fn, z, kw, g) for name, fn, z, kw, g in _cases(golden)}
    g = golden("hydro")
    assert str(g["numpy_version"]).split(".")[0] == "2"                      # NEP 50: fl32(tol), fl32(eps), fl32(nodata)
    raw = c["fill_raw"][1]
    assert np.isnan(raw).any() and (raw <= 0).any() and (raw > 0).any()
    out = g["out_fill_raw"]
    assert (out > raw).sum() > 50                                           # pits and basins raised
    assert not np.array_equal(out, g["out_fill_raw_conn4"]) and not np.array_equal(out, g["out_fill_raw_eps0"])
    assert not np.array_equal(out, g["out_fill_raw_eps001"])
    eps0 = g["out_fill_raw_eps0"]
    assert ((eps0 > raw) & (eps0 == np.roll(eps0, 1, axis=1))).any()      # eps 0: flat filled basins
    nod = c["fill_nodata"][1]
    on = nod == np.float32(c["fill_nodata"][2]["nodata"])
    assert on.any() and np.array_equal(g["out_fill_nodata"][on], nod[on]) and not np.array_equal(g["out_fill_nodata"], g["out_fill_small"])
    assert np.array_equal(g["out_fill_all_ocean"], c["fill_all_ocean"][1]) and (c["fill_all_ocean"][1] <= 0).all()
    assert (c["fill_all_land"][1] > 0).all() and (g["out_fill_all_land"] > c["fill_all_land"][1]).any()
    # d8: ocean centres, sinks without ocean (pits), land draining into ocean, border clamps, NaN neighbours
    z = c["d8_raw"][1]
    sink, kmax, rec = g["sink_d8_raw"], g["kmax_d8_raw"], g["receiver_d8_raw"]
    land = z > 0
    assert sink[~land].all() and (sink & land).any() and (~sink & land).any()
    assert (kmax >= 4).any() and len(np.unique(kmax)) == 8
    assert rec[0, 0] == 0 or kmax[0, 0] != 0
    assert not np.array_equal(g["receiver_d8_raw"], g["receiver_d8_raw_tol05"])
    assert not np.array_equal(g["sink_d8_filled"], sink)
    for name in ("t1x9", "t9x1", "t2x2", "t7x5"):
        assert c["d8_" + name][1].shape == {"t1x9": (1, 9), "t9x1": (9, 1), "t2x2": (2, 2), "t7x5": (7, 5)}[name]
    assert g["out_acc_raw"].max() > 100 and g["out_acc_filled"].max() > g["out_acc_raw"].max()
    # indicator: pooling on sizes that are not multiples of k
    assert raw.shape[0] % 2 and raw.shape[0] % 3 and raw.shape[1] % 3
    assert g["out_ind_raw_k2"].shape == (48, 65) and g["out_ind_raw_k3"].shape == (32, 43) and g["out_ind_small_k3"].shape == (21, 26)
    assert (g["out_ind_all_ocean"] == 0).all()


def test_hydro_library_exports_what_its_header_declares():
    import ctypes
    import os
    import re
    import __graft_entry__ as ge
    from terrain_diffusion_amd import hydrology
    ge.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ge.ROOT, "include", "td_hydro.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(td_[a-z0-9_]+)\s*\(", text))
    assert declared == set(hydrology.EXPORTS) == {"td_hydro_last_error", "td_hydro_d8", "td_hydro_accumulate", "td_hydro_indicator", "td_hydro_fill"}
    lib = ctypes.CDLL(hydrology.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name


def test_max_raise_and_negative_epsilon_are_refused():
    from terrain_diffusion_amd import fill_depressions_priority_flood
    h = np.full((8, 8), 5.0, np.float32)
    with pytest.raises(NotImplementedError, match="max_raise"):
        fill_depressions_priority_flood(h, max_raise=10.0)
    for eps in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            fill_depressions_priority_flood(h, epsilon=eps)


@pytest.mark.parametrize("shape", [(0, 8), (8, 0), (8,), (2, 3, 4)])
def test_bad_shapes_are_refused(shape):
    from terrain_diffusion_amd import d8_flow, fill_depressions_priority_flood, plot_flow_indicator
    z = np.ones(shape, np.float32)
    for fn in (d8_flow, fill_depressions_priority_flood, plot_flow_indicator):
        with pytest.raises(ValueError):
            fn(z)


def test_there_is_no_cpu_fallback(monkeypatch):
    """Without the library every call raises: nothing computes on the host."""
    from terrain_diffusion_amd import explorer, hydrology, minecraft, relief
    from terrain_diffusion_amd._lib import TdError
    for module in (relief, hydrology, minecraft, explorer):
        monkeypatch.setattr(module._LIB, "handle", None)
        monkeypatch.setattr(module._LIB, "path", "/nonexistent/" + module.LIB_PATH.rsplit("/", 1)[1])
        with pytest.raises(TdError, match="no CPU fallback"):
            module.lib()
    z = np.full((6, 7), 10.0, np.float32)
    rr, cc = np.zeros((6, 7), np.int64), np.zeros((6, 7), np.int64)
    calls = (lambda: hydrology.d8_flow(z), lambda: hydrology.flow_accumulation(z, rr, cc, np.ones((6, 7), bool)),
             lambda: hydrology.plot_flow_indicator(z), lambda: hydrology.fill_depressions_priority_flood(z))
    for call in calls:
        with pytest.raises(TdError):
            call()
