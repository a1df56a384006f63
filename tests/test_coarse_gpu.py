"""The coarse-dataset library on the GPU (include/td_coarse.h, coarse_csrc/coarse_kernels.hip) against the NumPy twin (tests/_coarse_twin.py)
and the fixture (tests/golden/coarse.npz: the reference's own fill_oceans, torch and NumPy on the committed cases): the area resize within
u (sum|x| + |mean|) of the float64 window mean and of torch's output, the tile statistics within 1 ulp of the twin and within the derived
bounds of NumPy's, the crop scores within the bound the twin derives, fill_oceans with the reference's iteration counts and within
CG_SLACK 2^-52 max|land| iterations of its output -- bit-identical between two calls, between chunk lengths and in the enqueue-only mode --,
build_coarse_bands against the same steps on the twin, and the C-ABI's refusals."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _coarse_twin as twin
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu
F = np.float32
U = twin.U


@pytest.fixture(scope="module")
def cd():
    from terrain_diffusion_amd import coarse_dataset
    assert torch.cuda.is_available()
    return coarse_dataset


@pytest.fixture(scope="module")
def eng():
    from terrain_diffusion_amd.engine import get_engine
    return get_engine("cuda")


@pytest.fixture(scope="module")
def fills():
    return twin.fill_cases()


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


# ------------------------------------------------------------------------------------------------------------------------------ area resize
@pytest.mark.parametrize("w_out", twin.RESIZE_W_OUT + (1000, 1, 3))
def test_area_resize_within_the_window_bound_of_float64_and_of_torch(cd, golden, w_out):
    x = twin.resize_input()
    d64, bound = twin.area_resize_w(x, w_out)
    got = cd.area_resize_width(x, w_out)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (x.shape[0], w_out)
    g = got.cpu().numpy()
    ok = ~np.isnan(d64)
    assert same_nan(g, d64) and (w_out == 1 or ok.sum() > ok.size // 2)
    ratio = np.abs(g.astype(np.float64) - d64)[ok] / bound[ok]
    print(f"\nresize 1000 -> {w_out}: worst err / bound vs float64 {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    assert np.array_equal(g, twin.area_resize_w_fp32(x, w_out), equal_nan=True)            # the sum from the left, restated
    if w_out in twin.RESIZE_W_OUT:
        want = golden("coarse")[f"resize_w{w_out}"]
        assert same_nan(g, want)
        r2 = np.abs(g.astype(np.float64) - want.astype(np.float64))[ok] / bound[ok]
        print(f"resize 1000 -> {w_out}: worst err / bound vs torch {r2.max():.3f}")
        assert r2.max() <= 1.0


@pytest.mark.parametrize("rule,name", [(1, "int16_nodata"), (2, "float_nodata"), (3, "signed_sqrt")])
def test_area_resize_load_rules(cd, rule, name):
    x = twin.resize_input()
    x[5, :40] = np.arange(-20, 20, dtype=F) * F(0.37)       # both signs and a zero for the square root
    d64, bound = twin.area_resize_w(x, 707, rule)
    g = cd.area_resize_width(torch.from_numpy(x).cuda(), 707, name).cpu().numpy()
    ok = ~np.isnan(d64)
    assert same_nan(g, d64) and int((~ok).sum()) > int(np.isnan(twin.area_resize_w(x, 707, 0)[0]).sum()) - (rule == 3)
    assert (np.abs(g.astype(np.float64) - d64)[ok] <= bound[ok]).all()
    assert np.array_equal(g, twin.area_resize_w_fp32(x, 707, rule), equal_nan=True)
    assert np.array_equal(cd.area_resize_width(x, 707, rule).cpu().numpy(), g, equal_nan=True)          # the rule by number


# ------------------------------------------------------------------------------------------------------------------------------ tile statistics
@pytest.mark.parametrize("t", twin.TILE_TS)
def test_tile_stats_within_one_ulp_of_the_twin_and_the_bounds_of_numpy(cd, golden, t):
    g = golden("coarse")
    x = twin.tile_input()
    want = twin.tile_stats(x, t)
    got = {k: v.cpu().numpy() for k, v in cd.tile_stats(x, t, twin.TILE_Q).items()}
    tl = twin.tiles_of(x, t).astype(np.float64)
    n = t * t
    assert set(got) == {"mean", "nanmean", "quantile"}
    for k in got:
        assert got[k].dtype == F and got[k].shape == (70 // t, 101 // t) and same_nan(got[k], want[k]) and same_nan(got[k], g[f"tile_{k}_t{t}"]), (k, t)
        ok = ~np.isnan(want[k])
        assert (np.abs(got[k].astype(np.float64) - want[k].astype(np.float64))[ok] <= twin.ulp(want[k])[ok]).all(), (k, t)
    mean_abs = twin.nan_mean_abs(tl)
    for k in ("mean", "nanmean"):
        ok = ~np.isnan(want[k])
        bound = n * U * mean_abs + U * np.abs(want[k].astype(np.float64))
        assert (np.abs(got[k].astype(np.float64) - g[f"tile_{k}_t{t}"].astype(np.float64))[ok] <= bound[ok]).all(), (k, t)
    ok = ~np.isnan(want["quantile"])
    bound = 3 * U * np.maximum(np.abs(want["a"]), np.abs(want["b"]))
    assert (np.abs(got["quantile"].astype(np.float64) - g[f"tile_quantile_t{t}"].astype(np.float64))[ok] <= bound[ok]).all(), t
    # tiles with a NaN, a tile without a value (t = 26 covers rows 26 .. 51), tiles with ties
    assert np.isnan(want["mean"]).any() and (t == 32 or not np.isnan(want["mean"]).all())
    if t == 26:
        assert np.isnan(got["nanmean"][1, 1]) and not np.isnan(got["nanmean"][0, 0])
    if t > 1:
        ties = np.array([len(np.unique(v)) < n for v in tl.reshape(-1, n)]).reshape(tl.shape[:2])
        assert (ties & ok).any()
    # a single output, another quantile
    one = cd.tile_stats(torch.from_numpy(x).cuda(), t, 0.5, stats=("quantile",))
    assert set(one) == {"quantile"}
    w5 = twin.tile_stats(x, t, 0.5)["quantile"]
    o = one["quantile"].cpu().numpy()
    assert same_nan(o, w5) and (np.abs(o.astype(np.float64) - w5)[~np.isnan(w5)] <= twin.ulp(w5)[~np.isnan(w5)]).all()


# ------------------------------------------------------------------------------------------------------------------------------ crop scores
@pytest.mark.parametrize("c", twin.CROP_CS)
def test_crop_scores_within_the_derived_bound(cd, golden, c):
    plane, mean0, std0, offsets = twin.crop_input()
    want, bound = twin.crop_scores(plane, mean0, std0, offsets[c], c)
    got = cd.crop_scores(plane, mean0, std0, offsets[c], c)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (len(offsets[c]),)
    g = got.cpu().numpy().astype(np.float64)
    ratio = np.abs(g - want) / bound
    print(f"\ncrop scores c = {c}: worst err / bound {ratio.max():.3f}; bound / score {np.max(bound / want):.2e}")
    assert np.isfinite(g).all() and (want > 0).all() and ratio.max() <= 1.0
    rec = golden("coarse")[f"crop_c{c}"].astype(np.float64)
    assert (np.abs(g - rec) <= 2 * bound).all()              # torch's recorded score sits inside the same bound of the float64 score
    # a crop with a NaN gives NaN; device offsets are not read back: a crop that leaves the plane gives NaN
    p2 = plane.copy()
    p2[1, 1] = np.nan
    off = torch.tensor([[0, 0], [plane.shape[0] - c + 1, 0], [-1, 4], [plane.shape[0] - c, plane.shape[1] - c]], dtype=torch.int32).cuda()
    s = cd.crop_scores(torch.from_numpy(p2).cuda(), mean0, std0, off, c).cpu().numpy()
    assert np.isnan(s[:3]).all() and abs(float(s[3]) - want[1]) <= bound[1]


# ------------------------------------------------------------------------------------------------------------------------------ fill_oceans
def check_fill(a, out, info, ref, ref_info, tol):
    land = ~np.isnan(a)
    assert out.dtype == np.float64 and out.shape == a.shape and not np.isnan(out).any()
    assert np.array_equal(out[land].view(np.uint64), a[land].view(np.uint64)), "land bits"
    assert info.tolist() == ref_info.tolist(), (info.tolist(), ref_info.tolist())
    iters = int(info[0] + info[2])
    if info[3] == 0 and info[2] > 0:
        rn, thr5 = twin.residual_norm(a, out)
        thr = max(tol, thr5)
        print(f"|b - A x| / threshold = {rn / thr:.4f}")
        assert rn <= (1 + 1e-9) * thr
    scale = 2.0 ** -52 * (float(np.abs(a[land]).max()) if land.any() else 1.0)
    err = float(np.max(np.abs(out - ref)))
    print(f"max|gpu - reference| = {err:.3e} = {err / (scale * max(iters, 1)):.3f} x 2^-52 max|land| iterations ({iters}); CG_SLACK {twin.CG_SLACK}")
    assert err <= twin.CG_SLACK * scale * iters if iters else err <= scale
    return err


@pytest.mark.parametrize("name", list(twin.FILL_SEEDS))
def test_fill_oceans_against_the_reference(cd, golden, fills, name):
    g = golden("coarse")
    assert name in json.loads(str(g["fill_names"])) and json.loads(str(g["fill_raises"])) == {}
    a, kw = fills[name]
    ref, ref_info = g["fill_out_" + name], g["fill_info_" + name]
    print(f"\n{name}: {a.shape}, {int(np.isnan(a).sum())} unknowns, reference info {ref_info.tolist()}")
    out, info = cd.fill_oceans_device(a, tol=twin.FILL_TOL, return_info=True, **kw)
    assert out.dtype == torch.float64 and out.is_cuda and info.dtype == torch.int32
    o = out.cpu().numpy()
    check_fill(a, o, info.cpu().numpy(), ref, ref_info, twin.FILL_TOL)
    if not np.isnan(a).any():
        assert np.array_equal(o.view(np.uint64), a.view(np.uint64))
    if np.isnan(a).all():
        assert (o == 1e-9).all()
    # the same bits on a second call, with chunk lengths 1 and 32, and in the enqueue-only mode
    for extra in ({}, {"chunk": 1}, {"chunk": 32}, {"enqueue_only": True}):
        o2, i2 = cd.fill_oceans_device(torch.from_numpy(a).cuda(), tol=twin.FILL_TOL, return_info=True, **kw, **extra)
        assert np.array_equal(o2.cpu().numpy().view(np.uint64), o.view(np.uint64)) and torch.equal(i2, info), (name, extra)


def test_fill_oceans_drop_in_and_a_band_sized_plane_against_the_twin(cd):
    a = twin.band_case()
    assert a.shape == (61, 1440) and 0.65 < np.isnan(a).mean() < 0.75
    traces = ([], [])
    want, want_info = twin.fill_oceans(a, tol=twin.FILL_TOL, traces=traces)
    got = cd.fill_oceans(a, tol=twin.FILL_TOL, maxiter=None, anchor_stride=None, anchor_strength=0.0, multires_factor=8)
    assert isinstance(got, np.ndarray)
    _, info = cd.fill_oceans_device(a, tol=twin.FILL_TOL, return_info=True)
    check_fill(a, got, info.cpu().numpy(), want, want_info, twin.FILL_TOL)
    assert want_info[0] > 0 and want_info[2] > 50
    # a device tensor as the input
    t = torch.from_numpy(a).cuda()
    assert np.array_equal(cd.fill_oceans_device(t, tol=twin.FILL_TOL).cpu().numpy().view(np.uint64), got.view(np.uint64))
    with pytest.raises(NotImplementedError, match="anchors"):
        cd.fill_oceans(a, anchor_stride=16, anchor_strength=0.01)


# ------------------------------------------------------------------------------------------------------------------------------ the bands
def test_build_coarse_bands_is_the_twins_steps(cd):
    """A small raster pair through build_coarse_bands against the same steps on the twin: the rows of latitude_bands, the float64 window means,
    the tile statistics, the twin's fill.  Tolerances: the resize bound carried through the tile mean (a mean of values each within its bound:
    the largest bound of the tile), the quantile likewise (1-Lipschitz), then the fill's bound on top of the land error (the solution of the
    Laplace system is an average of the land values: it moves by at most the largest land error)."""
    H, W, t = 180, 400, 5
    e = (twin._normal(7001, (H, W)) * F(900.0) + F(200.0)).astype(F)
    base = (twin._normal(7002, (H, W)) * F(8.0) + F(15.0)).astype(F)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sea = np.cos(jj / 23.0 + ii / 40.0) < -0.2              # slanted stripes of sea about 50 columns wide: whole tiles without a value in every band
    layers = [base.copy(), base * F(0.5), base + F(3.0), base * F(2.0)]
    for l in layers:
        l[sea] = F(-3.4e38)                                 # WorldClim's float no-data value
    out = cd.build_coarse_bands(e, layers, 90.0, -90.0, tile_px=t)
    start, end, bands = cd.latitude_bands(H, 90.0, -90.0)
    assert (start, end) == (30, 150) and len(bands) == 9 and set(out) == {f"gan_band_{i}" for i in range(9)} | {"means", "stds", "band_weights"}
    flat = []
    for i, (r0, r1, mid) in enumerate(bands):
        w = cd.band_width(W, mid)
        band = out[f"gan_band_{i}"]
        assert band.dtype == np.float64 and band.shape == (6, (r1 - r0) // t, w // t)
        d64, bnd = twin.area_resize_w(e[start + r0:start + r1], w, 3)
        st = twin.tile_stats(d64.astype(F), t)
        tol_tile = twin.tiles_of(bnd, t).max(-1) + 2 * U * np.abs(twin.tiles_of(d64, t)).max(-1)
        assert (np.abs(band[0] - st["mean"]) <= tol_tile).all() and (np.abs(band[1] - (st["mean"].astype(np.float64) - st["quantile"])) <= 3 * tol_tile).all()
        for k, layer in enumerate(layers):
            d64, bnd = twin.area_resize_w(layer[start + r0:start + r1], w, 2)
            nm = twin.tile_stats(d64.astype(F), t)["nanmean"].astype(np.float64)
            assert np.isnan(nm).any() and not np.isnan(nm).all()
            want, info = twin.fill_oceans(nm, tol=cd.FILL_TOL)
            land = ~np.isnan(nm)
            land_tol = float(np.nanmax(twin.tiles_of(bnd, t)[land]) + 2 * U * np.nanmax(np.abs(twin.tiles_of(d64, t)[land])))
            assert (np.abs(band[k + 2] - want)[land] <= land_tol).all()
            # off the land the two CG runs start from land values that differ by land_tol: both end below the same stop threshold of the
            # same system up to that, so they agree to the threshold's own scale, 1e-5 |b| spread over the unknowns -- stated loosely as
            # 1e-3 of the land's range, which a wrong fill (zeros, the mean, an unconverged start) misses by orders of magnitude
            assert np.abs(band[k + 2] - want).max() <= 1e-3 * float(np.ptp(nm[land]))
        flat.append(band.reshape(6, -1))
    allb = np.concatenate(flat, 1)
    assert np.allclose(out["means"], allb.mean(1), rtol=1e-6, atol=0) and np.allclose(out["stds"], allb.std(1), rtol=1e-5, atol=0)
    widths = np.zeros(50)
    widths[:9] = [(r1 - r0) // t for r0, r1, _ in bands]
    assert out["band_weights"].dtype == F and np.array_equal(out["band_weights"], widths.astype(F) / np.sum(widths).astype(F))
    # an int16 layer takes the int16 rule
    r = cd.area_resize_width(np.array([[5, 32767, -32768, 7]], np.int16), 4, "int16_nodata").cpu().numpy()
    assert r.tolist() == [[5.0, 32767.0, -32768.0, 7.0]]


# ------------------------------------------------------------------------------------------------------------------------------ the C-ABI
def test_the_c_abi_refuses_bad_arguments(cd, eng):
    lib = cd.lib()
    st = C.c_void_p(eng.stream)
    x = torch.zeros((8, 16), dtype=torch.float32, device="cuda")
    o = torch.zeros((8, 16), dtype=torch.float32, device="cuda")
    a = torch.zeros((8, 16), dtype=torch.float64, device="cuda")
    b = torch.zeros((8, 16), dtype=torch.float64, device="cuda")
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    off = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    host = np.zeros((8, 16), F)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    hp = C.c_void_p(host.ctypes.data)

    def refused(rc, text):
        assert rc == -1 and text in cd._LIB.error_text(), (rc, cd._LIB.error_text())
    refused(lib.td_coarse_area_resize_w(st, p(x), 0, 16, 8, 0, p(o), 1), "H >= 1")
    refused(lib.td_coarse_area_resize_w(st, p(x), 8, 16, 17, 0, p(o), 1), "W_out <= W_in")
    refused(lib.td_coarse_area_resize_w(st, p(x), 8, 16, 8, 4, p(o), 1), "load_rule")
    refused(lib.td_coarse_area_resize_w(st, None, 8, 16, 8, 0, p(o), 1), "null buffer")
    refused(lib.td_coarse_area_resize_w(st, hp, 8, 16, 8, 0, p(o), 1), "device buffers only")
    refused(lib.td_coarse_area_resize_w(st, p(x), 8, 16, 8, 0, p(x), 1), "overlaps")
    refused(lib.td_coarse_tile_stats(st, p(x), 8, 16, 9, 0.05, p(o), None, None, 1), "1 <= t <= min(32, Hs, Ws)")
    refused(lib.td_coarse_tile_stats(st, p(x), 8, 16, 0, 0.05, p(o), None, None, 1), "1 <= t <= min(32, Hs, Ws)")
    refused(lib.td_coarse_tile_stats(st, p(x), 8, 16, 2, 1.5, p(o), None, None, 1), "0 <= q <= 1")
    refused(lib.td_coarse_tile_stats(st, p(x), 8, 16, 2, 0.05, None, None, None, 1), "no output")
    refused(lib.td_coarse_tile_stats(st, p(x), 8, 16, 2, 0.05, None, hp, None, 1), "device buffers only")
    refused(lib.td_coarse_crop_scores(st, p(x), 8, 16, 0.0, 1.0, p(off), 1, 2, p(o), 1), "3 <= c")
    refused(lib.td_coarse_crop_scores(st, p(x), 8, 16, 0.0, 1.0, p(off), 1, 9, p(o), 1), "3 <= c")
    refused(lib.td_coarse_crop_scores(st, p(x), 8, 16, 0.0, 1.0, p(off), 0, 3, p(o), 1), "1 <= N")
    refused(lib.td_coarse_crop_scores(st, p(x), 8, 16, 0.0, 1.0, None, 1, 3, p(o), 1), "null buffer")
    refused(lib.td_coarse_fill_oceans(st, p(a), 8, 8193, 1e-6, 0, 8, p(b), p(info), 1), "1 <= H, W <= 8192")
    refused(lib.td_coarse_fill_oceans(st, p(a), 8, 16, 1e-6, 0, 33, p(b), p(info), 1), "multires_factor")
    refused(lib.td_coarse_fill_oceans(st, p(a), 8, 16, 1e-6, 0, 0, p(b), p(info), 1), "multires_factor")
    refused(lib.td_coarse_fill_oceans(st, p(a), 8, 16, -1.0, 0, 8, p(b), p(info), 1), "tol")
    refused(lib.td_coarse_fill_oceans(st, p(a), 8, 16, float("nan"), 0, 8, p(b), p(info), 1), "tol")
    refused(lib.td_coarse_fill_oceans(st, p(a), 8, 16, 1e-6, -1, 8, p(b), p(info), 1), "maxiter")
    refused(lib.td_coarse_fill_oceans(st, p(a), 8, 16, 1e-6, 0, 8, p(b), None, 1), "null buffer")
    refused(lib.td_coarse_fill_oceans(st, hp, 8, 16, 1e-6, 0, 8, p(b), p(info), 1), "device buffers only")
    refused(lib.td_coarse_fill_oceans(st, p(a), 8, 8, 1e-6, 0, 8, C.c_void_p(a.data_ptr() + 64), p(info), 1), "overlaps")
    refused(lib.td_coarse_fill_oceans_chunked(st, p(a), 8, 16, 1e-6, 0, 8, 0, p(b), p(info), 1), "chunk")
    assert lib.td_coarse_fill_oceans(st, p(a), 8, 16, 1e-6, 0, 8, p(a), p(info), 1) == 0 and info.cpu().tolist() == [0, 0, 0, 0]      # in place, no ocean
