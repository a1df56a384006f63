"""The coarse-dataset preparation without a GPU: the NumPy twin (tests/_coarse_twin.py) against what the reference's own fill_oceans, torch and
NumPy recorded (tests/golden/coarse.npz), by the criteria the GPU tests hold the kernels to; the measured CG ratio behind CG_SLACK; the header
against the binding; the argument checks, which refuse before an engine exists; latitude_bands against hand-computed rows; the DATA_LIBS row."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _coarse_twin as twin
from terrain_diffusion_amd import coarse_dataset as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = twin.U


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


# ------------------------------------------------------------------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("w_out", twin.RESIZE_W_OUT)
def test_the_window_rule_is_torchs_area_interpolation(golden, w_out):
    x = twin.resize_input()
    want = golden("coarse")[f"resize_w{w_out}"]
    d64, bound = twin.area_resize_w(x, w_out)
    got = twin.area_resize_w_fp32(x, w_out)
    ok = ~np.isnan(d64)
    assert want.shape == (6, w_out) and same_nan(want, d64) and same_nan(got, d64) and 0 < (~ok).sum() < ok.size // 3
    assert (np.abs(want.astype(np.float64) - d64)[ok] <= bound[ok]).all() and (np.abs(got.astype(np.float64) - d64)[ok] <= bound[ok]).all()
    wins = twin.windows(1000, w_out)
    assert wins[0][0] == 0 and wins[-1][1] == 1000 and all(b > a for a, b in wins) and all(n[0] <= p[1] for p, n in zip(wins, wins[1:]))


def test_the_load_rules():
    x = np.array([[32768.0, 32767.0, -32768.0, 1.0e6, 1.0000001e6 * 1.001, -2.0e6, -9.0, 9.0, 0.0, np.nan]], F)
    assert np.isnan(twin.load_rule(x, 1)[0]).tolist() == [True] + [False] * 8 + [True]
    assert np.isnan(twin.load_rule(x, 2)[0]).tolist() == [False] * 4 + [True, True] + [False] * 3 + [True]
    assert np.array_equal(twin.load_rule(x, 3)[0, 6:9], np.array([-3.0, 3.0, 0.0], F)) and twin.load_rule(x, 0) is not None
    assert cd.LOAD_RULES == {None: 0, "none": 0, "int16_nodata": 1, "float_nodata": 2, "signed_sqrt": 3}


@pytest.mark.parametrize("t", twin.TILE_TS)
def test_the_twins_tile_statistics_against_numpys(golden, t):
    g = golden("coarse")
    x = twin.tile_input()
    got = twin.tile_stats(x, t)
    tl = twin.tiles_of(x, t).astype(np.float64)
    n = t * t
    mean_abs = twin.nan_mean_abs(tl)
    for k in ("mean", "nanmean"):
        want = g[f"tile_{k}_t{t}"]
        ok = ~np.isnan(want)
        assert want.shape == (70 // t, 101 // t) and same_nan(got[k], want)
        bound = n * U * mean_abs + U * np.abs(got[k].astype(np.float64))
        assert (np.abs(got[k].astype(np.float64) - want.astype(np.float64))[ok] <= bound[ok]).all(), (k, t)
    want = g[f"tile_quantile_t{t}"]
    ok = ~np.isnan(want)
    bound = 3 * U * np.maximum(np.abs(got["a"]), np.abs(got["b"]))
    assert same_nan(got["quantile"], want) and (np.abs(got["quantile"].astype(np.float64) - want.astype(np.float64))[ok] <= bound[ok]).all(), t
    assert np.isnan(want).any() and (t == 32 or ok.any())


@pytest.mark.parametrize("c", twin.CROP_CS)
def test_the_twins_crop_scores_bound_holds_torchs_outputs(golden, c):
    plane, mean0, std0, offsets = twin.crop_input()
    want, bound = twin.crop_scores(plane, mean0, std0, offsets[c], c)
    rec = golden("coarse")[f"crop_c{c}"].astype(np.float64)
    assert rec.shape == (6,) and (np.abs(rec - want) <= bound).all()
    assert (bound < 1e-4 * want).all() and (want > 0).all()          # the bound is a rounding bound, far below the scores themselves
    k, g = twin.torch_rank(0.9, c * c)
    assert 0 <= k < c * c - 1 and g.dtype == F and 0 <= float(g) < 1
    assert twin.torch_rank(0.9, 1024) == (920, F(F(0.9) * F(1023)) - F(920))


@pytest.mark.parametrize("name", list(twin.FILL_SEEDS))
def test_the_twins_fill_oceans_against_the_reference(golden, name):
    g = golden("coarse")
    names = json.loads(str(g["fill_names"]))
    assert names == list(twin.FILL_SEEDS) and json.loads(str(g["fill_raises"])) == {}
    a, kw = twin.fill_cases()[name]
    assert a.shape[0] <= 64 and a.shape[1] <= 160
    ref, ref_info = g["fill_out_" + name], g["fill_info_" + name]
    got, info = twin.fill_oceans(a, tol=twin.FILL_TOL, order="pairwise", **kw)
    land = ~np.isnan(a)
    assert info.tolist() == ref_info.tolist() and not np.isnan(got).any()
    assert np.array_equal(got[land].view(np.uint64), a[land].view(np.uint64))
    iters = int(info[0] + info[2])
    scale = 2.0 ** -52 * (float(np.abs(a[land]).max()) if land.any() else 1.0)
    err = float(np.max(np.abs(got - ref)))
    assert err <= twin.CG_MEASURED_RATIO * scale * iters if iters else err <= scale
    if info[3] == 0 and info[2] > 0:
        rn, thr5 = twin.residual_norm(a, ref)
        assert rn <= (1 + 1e-9) * max(twin.FILL_TOL, thr5)


def test_the_committed_fill_cases_cover_what_the_issue_lists(golden):
    g = golden("coarse")
    cases = twin.fill_cases()
    info = {n: g["fill_info_" + n].tolist() for n in cases}
    assert cases["c24"][0].shape == (24, 24) and cases["c37x83"][0].shape == (37, 83) and cases["c64x160"][0].shape == (64, 160)
    e = np.isnan(cases["edges"][0])
    assert e[0].all() and e[-1].all() and e[:, 0].all() and e[:, -1].all() and not e.all()
    lake = np.isnan(cases["lake"][0])
    assert lake.any() and not (lake[0].any() or lake[-1].any() or lake[:, 0].any() or lake[:, -1].any())
    assert np.isnan(cases["one_ocean"][0]).sum() == 1 and (~np.isnan(cases["one_land"][0])).sum() == 1
    assert np.isnan(cases["all_ocean"][0]).all() and not np.isnan(cases["no_ocean"][0]).any()
    assert (g["fill_out_all_ocean"] == 1e-9).all() and info["all_ocean"] == [0, 0, 0, 0]          # b = 0 on both levels, then the allclose rule
    assert np.array_equal(g["fill_out_no_ocean"], cases["no_ocean"][0]) and info["no_ocean"] == [0, 0, 0, 0]
    assert np.isnan(twin.block_nanmean(cases["blockless"][0], 8)).any() and not np.isnan(twin.block_nanmean(cases["blockless"][0], 8)).all()
    assert not np.isnan(twin.block_nanmean(cases["coarse_dry"][0], 8)).any() and info["coarse_dry"][:2] == [0, 0] and info["coarse_dry"][2] > 0
    assert cases["f1"][1] == {"multires_factor": 1} and cases["f4"][1] == {"multires_factor": 4} and info["f1"][2] == 0      # the coarse level IS the fine one
    assert cases["maxiter5"][1] == {"maxiter": 5} and info["maxiter5"] == [5, 5, 5, 5]
    assert info["c64x160"][0] > 0 and info["c64x160"][2] > 50
    # CG_SLACK is 8 times the measured ratio, and the measured ratio is the fixture's
    worst = float(g["fill_ratio_max"])
    assert g["fill_ratio"].shape == (len(cases), len(twin.ORDERS)) and len(twin.ORDERS) >= 3
    assert worst <= twin.CG_MEASURED_RATIO <= 1.3 * worst + 0.01 and twin.CG_SLACK == 8 * twin.CG_MEASURED_RATIO


def test_the_band_sized_case_is_not_a_coin_toss():
    a = twin.band_case()
    traces = ([], [])
    _, info = twin.fill_oceans(a, tol=twin.FILL_TOL, traces=traces)
    _, thr5 = twin.residual_norm(a, np.zeros_like(a))
    thr = max(twin.FILL_TOL, thr5)
    assert info[3] == 0 and len(traces[1]) == info[2] + 1
    assert all(abs(rn - thr) > 1e-6 * thr for rn in traces[1][-2:])
    for order in ("pairwise", "permuted"):
        assert twin.fill_oceans(a, tol=twin.FILL_TOL, order=order)[1].tolist() == info.tolist()


def test_zoom_and_block_mean_restatements():
    c = np.arange(12, dtype=np.float64).reshape(3, 4) ** 1.5
    assert np.array_equal(twin.zoom_linear(c, 3, 4), c)                          # factor 1: the identity
    z = twin.zoom_linear(c, 5, 7)
    assert z.shape == (5, 7) and np.array_equal(z[[0, 2, 4]][:, [0, 2, 4, 6]], c) and np.allclose(z[1, 0], (c[0, 0] + c[1, 0]) / 2)
    assert twin.zoom_linear(c[:1, :1], 4, 3).tolist() == [[0.0] * 3] * 4
    a = np.array([[1.0, np.nan, 3.0], [np.nan, np.nan, 5.0], [7.0, 8.0, np.nan]])
    m = twin.block_nanmean(a, 2)
    assert m.shape == (2, 2) and m[0, 0] == 1.0 and m[0, 1] == 4.0 and m[1, 0] == 7.5 and np.isnan(m[1, 1])


# ------------------------------------------------------------------------------------------------------------------------------ the module's host halves
def test_latitude_bands_against_hand_computed_rows():
    # ETOPO 2022 at 30 arc-seconds: 21600 rows from +90 to -90, 120 rows per degree
    start, end, bands = cd.latitude_bands(21600, 90.0, -90.0)
    assert (start, end) == (3600, 18000) and len(bands) == 9
    assert [b[:2] for b in bands] == [(0, 1600), (1600, 3200), (3200, 4800), (4800, 6400), (6400, 8000), (8000, 9600), (9600, 11200), (11200, 12800),
                                      (12800, 14400)]
    mids = [b[2] for b in bands]
    assert np.allclose(mids, [160 / 3, 40.0, 80 / 3, 40 / 3, 0.0, -40 / 3, -80 / 3, -40.0, -160 / 3], rtol=0, atol=1e-12)
    assert cd.band_width(43200, mids[1]) == round(43200 * np.cos(np.deg2rad(40.0))) == 33093 and cd.band_width(43200, 0.0) == 43200
    # rows that do not divide: np.linspace(0, 120, 10, dtype=int) truncates
    start, end, bands = cd.latitude_bands(180, 90.0, -90.0)
    assert (start, end) == (30, 150) and [b[0] for b in bands] + [bands[-1][1]] == [0, 13, 26, 40, 53, 66, 80, 93, 106, 120]
    assert bands[0][2] == 90.0 - (0 + 13 + 60) / 2 and bands[4][2] == 90.0 - (53 + 66 + 60) / 2
    # a raster that ends at -56 degrees: the slice stops at its last row
    start, end, bands = cd.latitude_bands(146, 90.0, -56.0)
    assert (start, end) == (30, 150) and bands[-1][1] == 116
    with pytest.raises(ValueError, match="top > bottom"):
        cd.latitude_bands(100, -90.0, 90.0)
    with pytest.raises(ValueError, match="fewer than 9 bands"):
        cd.latitude_bands(12, 90.0, -90.0)


def test_header_entry_points_and_exports():
    import terrain_diffusion_amd as td
    import __graft_entry__ as ge
    text = open(os.path.join(ROOT, "include", "td_coarse.h")).read()
    declared = set(re.findall(r"\b(td_coarse_\w+)\s*\(", text))
    stated = {"td_coarse_last_error", "td_coarse_area_resize_w", "td_coarse_tile_stats", "td_coarse_crop_scores", "td_coarse_fill_oceans",
              "td_coarse_fill_oceans_chunked"}
    assert declared == set(cd.EXPORTS) == stated
    import ctypes as C
    for name in stated - {"td_coarse_last_error"}:
        params = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")
        assert len(params) == len(cd._SIGS[name][1]), name
        assert params[0].strip() == "void* hip_stream" and params[-1].strip() == "int synchronize", name
        for p, ctype in zip(params, cd._SIGS[name][1]):
            assert ("*" in p) == (ctype is cd._P), (name, p)
            if "*" not in p:
                assert {"int": C.c_int, "double": C.c_double, "float": C.c_float}[p.split()[0]] is ctype, (name, p)
    for macro, value in (("MAX_WIDTH", 65536), ("MAX_TILE", 32), ("MAX_SIDE", 8192), ("MAX_FACTOR", 32), ("DEFAULT_CHUNK", 32)):
        assert re.search(rf"#define TD_COARSE_{macro} {value}\b", text) and getattr(cd, macro) == value
    have = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", cd.LIB_PATH], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert stated <= have and not {n for n in have if n.startswith("td_") and n not in stated}
    cd.lib()     # binds every entry point
    for name in ("area_resize_width", "tile_stats", "crop_scores", "fill_oceans_device", "fill_oceans", "latitude_bands", "build_coarse_bands"):
        assert getattr(td, name) is getattr(cd, name), name
    assert ge.DATA_LIBS == (("coarse", "coarse_csrc", "coarse.hip", "td_coarse.h", ("-ffp-contract=off",), "coarse_dataset"),)
    assert len(ge.SIDE_LIBS) == 7 and not {r[0] for r in ge.SIDE_LIBS} & {r[0] for r in ge.DATA_LIBS} and "coarse" not in ge.SIDE_SHARED
    deps = [os.path.relpath(d, ROOT) for d in ge.side_deps("coarse", "coarse_csrc", "td_coarse.h")]
    assert deps == ["terrain_diffusion_amd/coarse_csrc/coarse.hip", "terrain_diffusion_amd/coarse_csrc/coarse_kernels.hip", "include/td_coarse.h",
                    "terrain_diffusion_amd/side_csrc/td_side_host.h"]
    # the solver's launches are plain: no cooperative launch, no graph capture
    src = "".join(open(os.path.join(ROOT, "terrain_diffusion_amd", "coarse_csrc", f)).read() for f in ("coarse.hip", "coarse_kernels.hip"))
    for word in ("Cooperative", "cooperative_groups", "hipGraph", "StreamBeginCapture", "atomicAdd"):
        assert word not in src, word


def test_argument_checks_refuse_before_any_engine_is_touched(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(cd, "_engine_for", no_engine)
    x = np.zeros((12, 20), F)
    for w in (0, 21, -3):
        with pytest.raises(ValueError, match="w_out must be in"):
            cd.area_resize_width(x, w)
    with pytest.raises(ValueError, match="load_rule"):
        cd.area_resize_width(x, 10, "sqrt")
    with pytest.raises(ValueError, match="load_rule"):
        cd.area_resize_width(x, 10, 4)
    for bad in (np.zeros(5, F), np.zeros((2, 3, 4), F)):
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            cd.area_resize_width(bad, 1)
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            cd.tile_stats(bad, 1)
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            cd.crop_scores(bad, 0.0, 1.0, np.zeros((1, 2), np.int32), 3)
        with pytest.raises(ValueError, match="a must be a 2D array"):
            cd.fill_oceans(bad)
        with pytest.raises(ValueError, match="a must be a 2D array"):
            cd.fill_oceans_device(bad)
    with pytest.raises(ValueError, match="limit"):
        cd.area_resize_width(np.broadcast_to(F(0), (1, 65537)), 1)
    for t in (0, 13, 33):
        with pytest.raises(ValueError, match="t must be in"):
            cd.tile_stats(x, t)
    with pytest.raises(ValueError, match="q must be in"):
        cd.tile_stats(x, 4, 1.5)
    with pytest.raises(ValueError, match="stats must name"):
        cd.tile_stats(x, 4, stats=("median",))
    for c in (2, 13, 33):
        with pytest.raises(ValueError, match="c must be in"):
            cd.crop_scores(x, 0.0, 1.0, np.zeros((1, 2), np.int32), c)
    with pytest.raises(ValueError, match=r"offsets must be \(N, 2\)"):
        cd.crop_scores(x, 0.0, 1.0, np.zeros((2, 3), np.int32), 4)
    with pytest.raises(ValueError, match="integers"):
        cd.crop_scores(x, 0.0, 1.0, np.zeros((2, 2), F), 4)
    for off in ([[9, 0]], [[0, 17]], [[-1, 0]]):
        with pytest.raises(ValueError, match="leaves the 12 x 20 plane"):
            cd.crop_scores(x, 0.0, 1.0, np.array(off, np.int32), 4)
    a = np.zeros((12, 20))
    with pytest.raises(ValueError, match="multires_factor must be >= 1"):
        cd.fill_oceans(a, multires_factor=0)
    with pytest.raises(ValueError, match=r"multires_factor must be in 1 \.\. 32"):
        cd.fill_oceans(a, multires_factor=33)
    with pytest.raises(ValueError, match="tol"):
        cd.fill_oceans(a, tol=-1.0)
    with pytest.raises(ValueError, match="maxiter"):
        cd.fill_oceans(a, maxiter=0)
    with pytest.raises(ValueError, match="chunk"):
        cd.fill_oceans_device(a, chunk=0)
    with pytest.raises(ValueError, match="limit"):
        cd.fill_oceans_device(np.broadcast_to(0.0, (1, 8193)))
    with pytest.raises(NotImplementedError, match="anchors"):
        cd.fill_oceans(a, anchor_stride=8, anchor_strength=0.1)
    e = np.zeros((180, 400), F)
    with pytest.raises(ValueError, match="four climate rasters"):
        cd.build_coarse_bands(e, [e, e], 90.0, -90.0)
    with pytest.raises(ValueError, match="share one grid"):
        cd.build_coarse_bands(e, [e, e, e, e[:, :399]], 90.0, -90.0)
    with pytest.raises(ValueError, match="tile_px"):
        cd.build_coarse_bands(e, [e] * 4, 90.0, -90.0, tile_px=33)
    with pytest.raises(ValueError, match="hold no 26 x 26 tile"):
        cd.build_coarse_bands(e, [e] * 4, 90.0, -90.0)
