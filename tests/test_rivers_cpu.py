"""River maps, host side (no GPU): the NumPy twin (tests/_rivers_twin.py) against every case recorded from the reference's get_relief_map and
smooth_river_bumps (tests/golden/rivers.npz, tests/golden/make_rivers_golden.py), the product's biome palette against the recorded one, the
fixtures' coverage of the branches, the C-ABI's exports, the build's staleness rule for the kernels libtd_rivers.so shares with
libtd_relief.so, and the refusals that come before any engine is touched."""
import json

import numpy as np
import pytest

import _rivers_twin as twin

RIVER = np.array([0.100, 0.450, 0.850], np.float32)


def _cases(golden, fn):
    g = golden("rivers")
    for c in json.loads(str(g["cases"])):
        if c["fn"] == fn:
            kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in c["kwargs"].items()}
            yield c, g[c["input"]], kw, g["out_" + c["name"]], g


def _overlays(c, g):
    return {k: g[v] for k, v in c.get("overlays", {}).items()}


def _off_one_factor(shaded, base):
    """how far (n, 3) `shaded` is from `base` times ONE shading factor per pixel (read off the strongest channel)"""
    k = base.argmax(axis=1)[:, None]
    m = np.take_along_axis(shaded, k, 1) / np.take_along_axis(base, k, 1)
    return float(np.abs(shaded - base * m).max())


def test_palette_equals_the_recorded_one(golden):
    from terrain_diffusion_amd import rivers
    want = golden("rivers")["biome_palette"]
    assert rivers.BIOME_PALETTE_U8.shape == (31, 3) and rivers.BIOME_PALETTE_U8.dtype == np.uint8
    got = rivers.biome_palette()
    assert got.dtype == np.float32 == want.dtype and np.array_equal(got, want)
    assert np.array_equal(twin.palette(rivers.BIOME_PALETTE_U8), want)


def test_twin_matches_every_recorded_relief_case(golden):
    pal = golden("rivers")["biome_palette"]
    n = 0
    for c, elev, kw, want, g in _cases(golden, "relief"):
        got = twin.relief(elev, pal=pal, **_overlays(c, g), **kw)
        assert np.array_equal(np.isnan(got), np.isnan(want)), c["name"]
        msg = twin.compare(got, want, tol=5e-5, step_frac=0.0)
        assert msg is None, (c["name"], msg)
        n += 1
    assert n == 17


def test_twin_without_overlays_is_the_relief_twin():
    import _relief_twin as rt
    e = twin.land_and_sea(40, 56, 5)
    e[3:6, 7:20] = np.nan
    for kw in ({}, dict(vmin=100.0, vmax=900.0, relief=0.7)):
        assert np.array_equal(twin.relief(e, **kw), rt.relief(e, **kw), equal_nan=True)


def test_recorded_relief_cases_cover_the_branches(golden):
    g = golden("rivers")
    assert str(g["numpy_version"]).split(".")[0] == "2"                      # NEP 50: flow > fl32(threshold), fp32 river blend
    c = {c["name"]: (elev, kw, out, _overlays(c, g)) for c, elev, kw, out, g in _cases(golden, "relief")}
    shapes = {elev.shape for elev, *_ in c.values()}
    assert shapes == {(160, 224), (64, 80), (7, 5), (2, 9)}
    thresholds = {kw.get("flow_threshold", 7) for _, kw, _, ov in c.values() if "flow" in ov}
    assert thresholds == {7, 3, 2.5}
    river_rgb = lambda shaded: np.float32(0.25) * shaded + np.float32(0.75) * RIVER
    for name in ("flow_small", "biome_flow_canvas"):
        e, kw, out, ov = c[name]
        river = ov["flow"] > np.float32(kw.get("flow_threshold", 7))
        # a river pixel on land: bluer than any shaded land can make it (0.75 * 0.85 in the blue channel), and not the ocean ramp
        on_land = river & (e >= 0)
        assert on_land.sum() > 20 and (out[on_land][:, 2] >= 0.75 * 0.85 - 1e-4).all(), name
        assert (np.abs(out[on_land] - river_rgb(np.zeros(3, np.float32))) < 0.2501).all(), name
        # a river pixel overwritten by ocean: the ramp's colour, whatever the flow
        drowned = river & (e < 0)
        t = np.clip(-e[drowned] / np.float32(10000), 0, 1) ** np.float32(0.7)
        ramp = (1 - t)[:, None] * np.array([0.68, 0.88, 1.00], np.float32) + t[:, None] * np.array([0.00, 0.10, 0.45], np.float32)
        assert drowned.sum() > 20 and np.abs(out[drowned] - ramp).max() < 5e-5, name
    # thresholds: flows are integers, 3 and 2.5 both draw flow 3 ... but only 2.5 draws it for "> 3"
    e, _, _, ov = c["flow_small"]
    assert np.array_equal(ov["flow"], np.round(ov["flow"])) and (ov["flow"] == 3).any() and (ov["flow"] == 7).any() and (ov["flow"] == 8).any()
    # a river pixel on NaN stays NaN (positive median: no ocean colour replaces it)
    e, kw, out, ov = c["nan_pos_median"]
    river = ov["flow"] > np.float32(kw["flow_threshold"])
    assert np.nanmedian(e) > 0 and (river & np.isnan(e)).sum() > 5 and np.isnan(out[river & np.isnan(e)]).all()
    assert np.isnan(e[0, 0]) and np.isnan(e[-1, 17])
    e, kw, out, ov = c["nan_neg_median"]
    assert np.isnan(e).any() and np.nanmedian(e) < 0 and not np.isnan(out).any()   # the ocean colour replaces the NaN, river or not
    assert ((ov["flow"] > np.float32(kw["flow_threshold"])) & np.isnan(e)).any()
    e, kw, out, ov = c["all_ocean_flow"]
    assert (e < 0).all() and (ov["flow"] > 7).sum() > 20
    assert (out[..., 2] >= 0.45 - 1e-4).all() and (out[..., 0] <= 0.68 + 1e-4).all()   # the ramp everywhere, no river blue
    # biome: id 0 keeps the colormap, ids below 0 too, ids above 30 take entry 30
    e, kw, out, ov = c["biome_small"]
    b = ov["biome"]
    assert b.dtype == np.int32 and b.min() == -2 and b.max() == 34
    import _relief_twin as rt
    plain = rt.relief(e)
    land = e >= 0
    for ids in (b == 0, b < 0):
        assert (ids & land).sum() > 10 and np.abs(out[ids & land] - plain[ids & land]).max() < 5e-5
    painted = (b > 0) & land
    assert painted.sum() > 100 and np.abs(out[painted] - plain[painted]).max() > 0.05
    pal = g["biome_palette"]
    hi = (b > 30) & land
    assert hi.sum() > 10 and _off_one_factor(out[hi], np.broadcast_to(pal[30], out[hi].shape)) < 5e-5
    # rgb given: the picture is the caller's colour times the shading, whatever vmin / vmax say
    e, kw, out, ov = c["rgb_biome_small"]
    assert ov["rgb"].shape == (64, 80, 3) and ov["rgb"].dtype == np.float32 and "vmin" in kw
    keep = (ov["biome"] <= 0) & (e >= 0)
    assert keep.sum() > 10 and _off_one_factor(out[keep], ov["rgb"][keep]) < 5e-5
    assert "rgb" in c["rgb_flow_small"][3] and "flow" in c["rgb_flow_small"][3]


def test_twin_matches_every_recorded_smoothing_case(golden):
    """The fp32 twin under the GPU test's own bound (numpy's exp on both sides here), D64 reproducing the recorded e_ref, and the bound's
    margin: at most 1e-3 of what the smoothing moves."""
    n, seen = 0, set()
    for c, h, kw, want, g in _cases(golden, "smooth"):
        name = c["name"]
        d64, got = twin.smooth_d64(h, **kw), twin.smooth(h, **kw)
        assert got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(want), np.isnan(h)), name
        e_ref = float(np.nanmax(np.abs(want.astype(np.float64) - d64)))
        assert abs(e_ref - c["e_ref"]) <= 1e-9 + 1e-6 * c["e_ref"], (name, e_ref, c["e_ref"])   # float64 exp may differ in its last place
        tol = 4 * c["e_ref"] + twin.ulp32(np.nanmax(np.abs(h)))
        assert np.nanmax(np.abs(got.astype(np.float64) - d64)) <= tol, name
        moved = float(np.nanmax(np.abs(want - h)))
        if kw.get("iterations", 3) > 0:
            assert tol <= 1e-3 * moved, (name, tol, moved)
        else:
            assert np.array_equal(want, h, equal_nan=True), name
        seen.add((h.shape, kw.get("iterations", 3), bool(np.isnan(h).any())))
        n += 1
    assert n == 17
    assert {s for s, _, _ in seen} == {(160, 224), (64, 80), (7, 5), (2, 9)} and {i for _, i, _ in seen} == {0, 1, 3, 8}
    assert {nan for _, _, nan in seen} == {False, True}


def test_smoothing_wraps_around_the_image_but_its_gradient_does_not():
    h = twin.land_and_sea(12, 9, 3, sea=0.0)
    up = h.copy()
    up[-1] += np.float32(100.0)
    a, b = twin.smooth(h, iterations=1), twin.smooth(up, iterations=1)
    assert not np.array_equal(a[0], b[0])                                    # row 0's upper neighbour is the last row
    assert np.array_equal(a[2:-3], b[2:-3])
    flat = np.full((6, 7), 5.0, np.float32)
    flat[-1] = 9.0
    one = twin.smooth(flat, iterations=1)
    # row 0: one-sided gradient 0 -> weight 1, Laplacian (9 - 5): moved by exactly 0.3 * 4 in fp32
    assert np.array_equal(one[0], np.full(7, np.float32(5.0) + np.float32(0.3) * np.float32(4.0), np.float32))


def test_rivers_library_exports_what_its_header_declares():
    import ctypes
    import os
    import re
    import __graft_entry__ as ge
    from terrain_diffusion_amd import rivers
    ge.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ge.ROOT, "include", "td_rivers.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(td_[a-z0-9_]+)\s*\(", text))
    assert declared == set(rivers.EXPORTS) == {"td_rivers_last_error", "td_rivers_relief", "td_rivers_smooth"}
    lib = ctypes.CDLL(rivers.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name


def test_the_c_abi_refuses_shapes_counts_and_null_buffers_before_any_hip_call():
    """these refusals come before the first HIP call, so they hold on a host without a GPU (host pointers and aliasing: tests/test_rivers_gpu.py)"""
    import ctypes as C
    import __graft_entry__ as ge
    from terrain_diffusion_amd import rivers
    ge.build()
    lib = rivers.lib()
    buf = (C.c_float * 256)()
    p, null = C.cast(buf, C.c_void_p), None
    relief = lambda H, W, rl, e=p: lib.td_rivers_relief(None, e, H, W, p, p, rl, p, 5, 315.0, 90.0, 1.0, 0, 0.0, 0.0, 0, 0.0, null, null, null, null, 7.0, p, 1)
    smooth = lambda H, W, it, h=p: lib.td_rivers_smooth(None, h, H, W, 50.0, 0.3, it, p, 1)
    for call, word in ((lambda: relief(1, 8, 24), "2 <= H"), (lambda: relief(8, (1 << 20) + 1, 24), "2 <= H"), (lambda: relief(8, 8, 65), "radius"),
                       (lambda: relief(8, 8, 24, null), "null"), (lambda: smooth(1, 8, 3), "2 <= H"), (lambda: smooth(8, 1, 3), "2 <= H"),
                       (lambda: smooth(1 << 16, 1 << 15, 3), "2^31"), (lambda: smooth(8, 8, 65), "iterations"), (lambda: smooth(8, 8, -1), "iterations"),
                       (lambda: smooth(8, 8, 3, null), "null")):
        assert call() < 0 and word in rivers._LIB.error_text(), word


def test_build_counts_the_shared_relief_sources_among_the_rivers_librarys():
    import os
    import __graft_entry__ as ge
    rows = {name: (sub, header) for name, sub, _, header, *_ in ge.SIDE_LIBS}
    assert "rivers" in rows and [m for *_, m in ge.SIDE_LIBS].count("rivers") == 1
    rel = lambda files: {os.path.relpath(f, ge.ROOT) for f in files}
    rivers, relief = rel(ge.side_deps("rivers", *rows["rivers"])), rel(ge.side_deps("relief", *rows["relief"]))
    csrc = "terrain_diffusion_amd/"
    assert {csrc + "rivers_csrc/rivers.hip", csrc + "rivers_csrc/rivers_kernels.hip", csrc + "relief_csrc/relief_kernels.hip",
            csrc + "relief_csrc/relief_host.h", csrc + "side_csrc/td_side_host.h", "include/td_rivers.h"} <= rivers
    assert not any("rivers" in f for f in relief) and csrc + "relief_csrc/relief_kernels.hip" in relief


def test_biome_ids_of_every_dtype():
    """the int32 ids the kernel takes: clip(id, 0, 30) survives for every integer type (the unsigned ones too), a floating image is truncated
    toward zero and its NaN counts as 0"""
    import torch
    from terrain_diffusion_amd.rivers import _biome_ids
    cpu = torch.device("cpu")
    clip = lambda t: t.clamp(0, 30).tolist()
    ids = np.array([[0, 1, 30, 31, 34, 127]])
    for dt in (np.uint8, np.int8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64):
        got = _biome_ids(ids.astype(dt), cpu)
        assert got.dtype == torch.int32 and clip(got) == [[0, 1, 30, 30, 30, 30]], dt
    assert clip(_biome_ids(torch.from_numpy(ids.astype(np.uint8)), cpu)) == [[0, 1, 30, 30, 30, 30]]
    wide = np.array([[-2 ** 40, -2, -1, 0, 7, 2 ** 40]])
    assert clip(_biome_ids(wide, cpu)) == [[0, 0, 0, 0, 7, 30]]
    assert clip(_biome_ids(np.array([[True, False]]), cpu)) == [[1, 0]]
    f = np.array([[np.nan, -0.9, 0.9, 1.0, 2.99, 30.5, 1e20, -1e20, np.inf]])
    for dt in (np.float32, np.float64):
        assert clip(_biome_ids(f.astype(dt), cpu)) == [[0, 0, 0, 1, 2, 30, 30, 0, 30]], dt


def test_package_level_surface():
    import terrain_diffusion_amd as td
    from terrain_diffusion_amd import relief, rivers
    assert td.get_relief_map is relief.get_relief_map                        # the refusing one stays the package's
    for name in ("relief_overlay_map", "smooth_bumps", "river_relief_map", "smooth_river_bumps"):
        assert getattr(td, name) is getattr(rivers, name)


@pytest.fixture
def no_engine(monkeypatch):
    """any attempt to reach an engine fails the test"""
    from terrain_diffusion_amd import _plumbing, rivers

    def boom(*a, **k):
        raise AssertionError("an engine was touched before the arguments were checked")
    monkeypatch.setattr(rivers, "engine_for", boom)
    monkeypatch.setattr(_plumbing, "get_engine", boom)


@pytest.mark.parametrize("shape", [(1, 8), (8, 1), (1, 1), (8,), (2, 3, 4)])
def test_images_below_2x2_are_refused(no_engine, shape):
    from terrain_diffusion_amd import rivers
    z = np.ones(shape, np.float32)
    for fn in (lambda: rivers.get_relief_map(z, None, None, None), lambda: rivers.relief_overlay_map(z), lambda: rivers.smooth_river_bumps(z),
               lambda: rivers.smooth_bumps(z), lambda: rivers.river_relief_map(z)):
        with pytest.raises(ValueError):
            fn()


def test_mismatched_overlays_and_iterations_are_refused(no_engine):
    from terrain_diffusion_amd import rivers
    e = np.ones((8, 9), np.float32)
    for flow in (np.zeros((9, 8), np.float32), np.zeros((8, 9, 1), np.float32), np.zeros(72, np.float32)):
        with pytest.raises(ValueError, match="flow"):
            rivers.get_relief_map(e, None, None, flow)
        with pytest.raises(ValueError, match="flow"):
            rivers.relief_overlay_map(e, flow=flow)
    for rgb in (np.zeros((8, 9), np.float32), np.zeros((8, 9, 4), np.float32), np.zeros((9, 8, 3), np.float32)):
        with pytest.raises(ValueError, match="rgb"):
            rivers.get_relief_map(e, None, None, None, rgb=rgb)
        with pytest.raises(ValueError, match="rgb"):
            rivers.relief_overlay_map(e, rgb=rgb)
    with pytest.raises(ValueError, match="biome"):
        rivers.relief_overlay_map(e, biome=np.zeros((9, 8), np.int32))         # the device form refuses; only the drop-in ignores it
    for it in (-1, 65, 1000, 2.5):
        with pytest.raises(ValueError, match="iterations"):
            rivers.smooth_river_bumps(e, iterations=it)
        with pytest.raises(ValueError, match="iterations"):
            rivers.smooth_bumps(e, iterations=it)
