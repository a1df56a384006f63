"""Explorer views, host side (no GPU): the NumPy twin (tests/_explorer_twin.py) against every case recorded from the reference's own explorer
routes and sampler (tests/golden/explorer.npz, tests/golden/make_explorer_golden.py), the package's colour tables, the C-ABI's entry points,
the PNG encoder and the refusals that come before any launch."""
import json
import math
import os
import random
import re

import numpy as np
import pytest
import torch

import _explorer_twin as twin

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def index(g):
    return json.loads(str(g["cases"]))


def luts(g):
    return {n: g["lut_" + n] for n in ("viridis", "terrain", "RdBu_r")}


def filters_of(view):
    return {int(k): tuple(v) for k, v in view["filters"].items()}


def json_equal(a, b):
    """Equality of parsed JSON with NaN equal to NaN."""
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(json_equal(a[k], b[k]) for k in a)
    if isinstance(a, list) and isinstance(b, list):
        return len(a) == len(b) and all(json_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b and type(a) is type(b)


def recorded_json(g, key):
    return json.loads(bytes(g[key]).decode())


def stats_as_json(stats):
    """What jsonify + a JSON parser make of coarse_stats' dict (integer keys become strings)."""
    return json.loads(json.dumps(stats))


def check_log1p_image(got, want, margin, name):
    """Channel-4 images: log1pf may differ by 1 ulp between libraries, so a pixel within 4 ulp of a table boundary may take the neighbouring
    entry; every other pixel matches exactly, and such pixels are at most 1e-3 of the image."""
    exempt = margin <= 4
    assert exempt.sum() <= 1e-3 * exempt.size, (name, int(exempt.sum()))
    assert np.array_equal(got[~exempt], want[~exempt]), (name, int((got != want).any(-1).sum()))


def check_relief_image(got, want, name):
    """Relief images, from the relief tests' bound (_relief_twin.compare: 1e-4 everywhere, 0.025 on at most 1e-3 of the pixels): 1e-4 * 255
    moves a byte by at most one level, 0.025 * 255 = 6.4 by at most 7; alpha is 255."""
    d = np.abs(got[..., :3].astype(np.int64) - want[..., :3].astype(np.int64)).max(-1)
    assert d.max() <= 7 and (d > 1).sum() <= 1e-3 * d.size, (name, int(d.max()), int((d > 1).sum()))
    assert np.all(got[..., 3] == 255) and np.all(want[..., 3] == 255), name


def check_coarse_case(g, c, image, stats, data):
    """One recorded coarse case against image(view) -> (rgba8, headers), stats() and data(); shared with the GPU test."""
    block = g["coarse_" + c["name"]]
    for v in c["views"]:
        img, hdr = image(v)
        want = g["img_" + v["key"]]
        assert img.dtype == np.uint8 and img.shape == want.shape, v["key"]
        if v["channel"] == 4:
            margin = twin.coarse_image(block, 4, g["lut_viridis"], filters_of(v))[2]
            check_log1p_image(img, want, margin, v["key"])
        else:
            assert np.array_equal(img, want), (v["key"], int((img != want).any(-1).sum()))
        assert hdr == json.loads(str(g["hdr_" + v["key"]])), v["key"]
    assert json_equal(stats_as_json(stats()), recorded_json(g, "stats_" + c["name"])), c["name"]
    if "data_" + c["name"] in g.files:
        assert json_equal(json.loads(json.dumps(data())), recorded_json(g, "data_" + c["name"])), c["name"]


def test_twin_channels_are_bit_equal_to_torch_on_the_cpu(golden):
    g = golden("explorer")
    for c in index(g)["coarse"]:
        block = torch.from_numpy(g["coarse_" + c["name"]])
        want = (block[:-1] / (block[-1:] + 1e-8)).numpy()
        want[:2] = np.sign(want[:2]) * np.square(want[:2])
        assert np.array_equal(twin.channels(block.numpy()).view(np.uint32), want.view(np.uint32)), c["name"]
    block = torch.from_numpy(g["land_coarse"])
    assert np.array_equal(twin.channels(block.numpy(), n_signed_sq=0, eps=0.0).view(np.uint32), (block[:-1] / block[-1:]).numpy().view(np.uint32))


def test_twin_matches_every_recorded_coarse_case(golden):
    g = golden("explorer")
    cs = index(g)["coarse"]
    assert [c["name"] for c in cs] == ["odd", "nan", "one", "const", "default"]
    for c in cs:
        block = g["coarse_" + c["name"]]
        check_coarse_case(g, c, lambda v: twin.coarse_image(block, v["channel"], g["lut_viridis"], filters_of(v))[:2],
                          lambda: twin.coarse_stats(block), lambda: twin.coarse_data(block, c["box"]))


def test_recorded_coarse_cases_cover_the_edges(golden):
    g = golden("explorer")
    cs = {c["name"]: c for c in index(g)["coarse"]}
    assert g["coarse_odd"].shape == (7, 41, 37) and g["coarse_one"].shape == (7, 1, 1) and g["coarse_default"].shape == (7, 100, 100)
    assert {v["channel"] for v in cs["odd"]["views"]} == set(range(6))
    assert np.isnan(g["coarse_nan"]).any() and np.all(g["img_nan_ch0"][0, 0] == 0)            # a NaN pixel is transparent black
    for k in ("one_ch0", "const_ch3"):                                                     # vmax == vmin: vmax = vmin + 1
        h = json.loads(str(g["hdr_" + k]))
        assert math.isclose(float(h["X-Vmax"]) - float(h["X-Vmin"]), 1.0, abs_tol=2e-3), k
    base, dimmed, same = g["img_odd_f_none"], g["img_odd_f_all"], g["img_odd_f_p5_ignored"]
    assert np.array_equal(base, same) and np.all(dimmed[..., :3] <= base[..., :3]) and (dimmed[..., :3] < base[..., :3]).any()
    assert np.array_equal(dimmed[..., 3], base[..., 3])
    part = (g["img_odd_f_both"] != base).any(-1)
    assert 0 < part.sum() < part.size


def test_twin_matches_every_recorded_detail_case(golden):
    g = golden("explorer")
    kinds = set()
    for c in index(g)["detail"]:
        n = c["name"]
        elev = g["elev_" + n]
        clim = g["climate_" + n] if "climate_" + n in g.files else None
        assert (clim is not None) == c["has_climate"]
        for mode in c["modes"]:
            img, kind, _ = twin.detail_image(elev, clim, mode, luts(g), c["native_resolution"])
            want = g[f"png_{n}_{mode}"]
            kinds.add((mode, kind))
            if kind == "relief":
                check_relief_image(img, want, (n, mode))
            else:
                assert np.array_equal(img, want), (n, mode, int((img != want).any(-1).sum()))
        if "raw_" + n in g.files:
            assert twin.raw_tile(elev, None if clim is None else clim[0]) == bytes(g["raw_" + n]), n
            assert json.loads(str(g["rawhdr_" + n])) == {"X-Height": "64", "X-Width": "64", "X-Has-Temp": "1" if c["has_climate"] else "0"}
    assert kinds == {("elevation", "elevation"), ("temperature", "temperature"), ("temperature", "relief"), ("relief", "relief")}
    assert np.isnan(g["elev_nan"]).any() and np.all(g["elev_ocean"] < 0)
    e16 = np.frombuffer(bytes(g["raw_raw"])[:2 * 64 * 64], "<i2").reshape(64, 64)
    assert e16[0, :8].tolist() == [32767, -32768, 32767, -32768, -1, -1, 7, 0] and e16[1, :4].tolist() == [32767, -32768, -4, 32767]
    assert len(g["raw_raw"]) == 6 * 64 * 64 and len(g["raw_raw_noclim"]) == 2 * 64 * 64


def test_twin_matches_every_recorded_land_case_and_the_fp32_mean_matters(golden):
    g = golden("explorer")
    block = g["land_coarse"]
    cases = index(g)["land"]
    assert len(cases) == 20
    for c in cases:
        n = c["name"]
        random.seed(int(g["seed"]))
        picks = twin.sample_land_tiles(block, c["window"], c["detail_size"], c["min_land_frac"], c["n_samples"])
        assert picks == [tuple(t) for t in g["picks_" + n].tolist()], n
        full = twin.sample_land_tiles(block, c["window"], c["detail_size"], c["min_land_frac"], 10 ** 9)
        assert full == [tuple(t) for t in g["full_" + n].tolist()], n
        if c["detail_size"] == 256:
            assert full == []
    # half 5, 0.7: a window of exactly 70 land cells has the fp32 mean 0.699999988 < 0.7; an exact-fraction comparison would let it in
    elev_m = twin.channels(block, eps=0.0)[0]
    want = [(-12 + p // 24, -12 + p % 24) for p in twin.land_tiles(elev_m, 5, 0.7).tolist()]
    exact = [(-12 + p // 24, -12 + p % 24) for p in twin.land_tiles(elev_m, 5, 0.7, exact=True).tolist()]
    assert want == [tuple(t) for t in g["full_d2560_f07"].tolist()] and exact != want and set(want) < set(exact)
    for c in index(g)["info"]:
        info = twin.climate_info(g["info_coarse_" + c["name"]])
        assert [info[k] for k in ("temp", "temp_std", "precip", "precip_cv")] == g["info_" + c["name"]].tolist()


def test_colour_tables_equal_the_recorded_ones_and_matplotlib(golden):
    from terrain_diffusion_amd import explorer as ex
    g = golden("explorer")
    for n in ("viridis", "terrain", "RdBu_r"):
        t = ex.colormap_lut(n)
        assert t.dtype == np.float32 and t.shape == (256, 3) and np.array_equal(t.view(np.uint32), g["lut_" + n].view(np.uint32)), n
    with pytest.raises(ValueError):
        ex.colormap_lut("magma")
    mpl = pytest.importorskip("matplotlib")
    for n in ("viridis", "terrain", "RdBu_r"):
        assert np.array_equal(ex.colormap_lut(n), mpl.colormaps[n](np.arange(256))[:, :3].astype(F)), n


def test_twin_normalisation_and_lookup_equal_matplotlib():
    mpl = pytest.importorskip("matplotlib")
    rng = np.random.default_rng(5)
    for k, name in enumerate(("viridis", "terrain", "RdBu_r") * 4):
        d = (rng.standard_normal((23, 19)) * 10.0 ** rng.integers(-2, 4)).astype(F)
        if k % 2:
            d[rng.integers(0, 23, 5), rng.integers(0, 19, 5)] = np.nan
        vmin, vmax = twin.view_range(d)
        want = mpl.colormaps[name](mpl.colors.Normalize(vmin=vmin, vmax=vmax)(d)).astype(F)
        got, _ = twin.lookup(twin.normalize(d, vmin, vmax), mpl.colormaps[name](np.arange(256))[:, :3].astype(F))
        assert np.array_equal(got, want), name


def test_header_entry_points_and_exports():
    import terrain_diffusion_amd as td
    from terrain_diffusion_amd import explorer as ex
    text = open(os.path.join(ROOT, "include", "td_explorer.h")).read()
    declared = set(re.findall(r"\b(td_explorer_\w+)\s*\(", text))
    stated = {"td_explorer_last_error", "td_explorer_channels", "td_explorer_colorize", "td_explorer_quantize", "td_explorer_raw",
              "td_explorer_land_tiles"}
    assert declared == set(ex.EXPORTS) == stated
    assert (ex.MAX_PIXELS, ex.MAX_SIDE, ex.MAX_FILTERS, ex.MAX_CHANNELS, ex.MAX_HALF) == (1 << 26, 1 << 16, 8, 8, 2047)
    for k, v in (("TD_EXPLORER_MAX_PIXELS", "(1 << 26)"), ("TD_EXPLORER_MAX_FILTERS", "8"), ("TD_EXPLORER_MAX_HALF", "2047")):
        assert re.search(rf"#define {k} {re.escape(v)}", text), k
    for name in ("coarse_channels", "colorize", "relief_rgba8", "raw_tile", "land_tiles", "coarse_image", "coarse_stats", "coarse_data",
                 "detail_image", "detail_raw", "sample_land_tiles", "get_coarse_climate_info", "png_bytes"):
        assert getattr(td, name) is getattr(ex, name), name
    assert ex.CHANNEL_NAMES == twin.CHANNEL_NAMES and ex.FILTERABLE == twin.FILTERABLE


def test_the_package_imports_neither_matplotlib_nor_pil():
    import subprocess
    import sys
    code = "import sys; import terrain_diffusion_amd.explorer; assert not ({'matplotlib', 'PIL'} & set(sys.modules)), 'imported'"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


def test_png_bytes_round_trips_through_a_zlib_decode(golden):
    from terrain_diffusion_amd.explorer import png_bytes
    g = golden("explorer")
    for img in (g["img_odd_f_both"], g["img_nan_ch0"], g["img_one_ch0"], np.arange(3 * 5 * 4, dtype=np.uint8).reshape(3, 5, 4)):
        data = png_bytes(img)
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and np.array_equal(twin.decode_png(data), img)
        assert np.array_equal(twin.decode_png(png_bytes(torch.from_numpy(img.copy()))), img)
    pil = pytest.importorskip("PIL.Image")
    import io
    assert np.array_equal(np.array(pil.open(io.BytesIO(png_bytes(g["img_odd_ch2"])))), g["img_odd_ch2"])
    for bad in (np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 4), F), np.zeros((0, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            png_bytes(bad)


class _NoWorld:
    native_resolution, seed = 90.0, 1

    def get(self, *a, **k):
        raise AssertionError("world.get must not be called for a refused request")


def test_refusals_before_any_launch():
    from terrain_diffusion_amd import explorer as ex
    z = lambda *s: np.zeros(s, F)
    for fn in (lambda: ex.coarse_channels(z(7, 4)), lambda: ex.coarse_channels(z(1, 4, 4)), lambda: ex.coarse_channels(z(10, 4, 4)),
               lambda: ex.coarse_channels(z(7, 0, 4)), lambda: ex.coarse_channels(z(7, 4, 4), n_signed_sq=7),
               lambda: ex.coarse_channels(z(7, 4, 4), eps=-1.0),
               lambda: ex.colorize(z(4), "viridis"), lambda: ex.colorize(z(4, 4), "magma"), lambda: ex.colorize(z(4, 4), z(255, 3)),
               lambda: ex.colorize(z(4, 4), "viridis", vmin=0.0), lambda: ex.colorize(z(4, 4), "viridis", vmin=1.0, vmax=1.0),
               lambda: ex.colorize(z(4, 4), "viridis", vmin=0.0, vmax=float("inf")),
               lambda: ex.colorize(z(4, 4), "viridis", filters=[(z(4, 4), 0.0, None)] * 9),
               lambda: ex.colorize(z(4, 4), "viridis", filters=[(z(4, 5), 0.0, None)]),
               lambda: ex.relief_rgba8(z(4, 4, 4)), lambda: ex.relief_rgba8(z(4, 4)),
               lambda: ex.raw_tile(z(4, 4, 1)), lambda: ex.raw_tile(z(4, 4), z(4, 5)),
               lambda: ex.land_tiles(z(8, 8), -1, 0.5), lambda: ex.land_tiles(z(8, 8), 5, 0.5), lambda: ex.land_tiles(z(8, 8), 2048, 0.5),
               lambda: ex.land_tiles(z(8, 8), 2, float("nan")), lambda: ex.land_tiles(z(8), 2, 0.5)):
        with pytest.raises(ValueError):
            fn()
    assert ex.resolved_range(2.0, 2.0) == (2.0, 3.0) and ex.resolved_range(1.0, 2.5) == (1.0, 2.5)
