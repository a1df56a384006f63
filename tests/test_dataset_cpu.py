"""The dataset preparation without a GPU: the NumPy twin (tests/_dataset_twin.py) against what SciPy, NumPy and the reference's own
calculate_stats_welford recorded (tests/golden/dataset.npz); the twin's statement of the kernels' capped void search against its exact one; the
header against the binding; RunningStats against the twin's loop; the argument checks, which refuse before an engine exists; and the sub-chunk
boxes against the reference's index arithmetic."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _dataset_twin as twin
from terrain_diffusion_amd import dataset as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def summation_bound(n):
    """relative worst-case bound of a float64 sum of n terms, with a factor 4 for the few operations around it"""
    return 4.0 * n * 2.0 ** -53


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def stats_keys():
    return [(name, tag, pct) for name in ("residual", "climate") for tag, pct in (("p0", 0.0), ("p4", 0.4))]


# ------------------------------------------------------------------------------------------------------------------------------ the fixture
def test_the_twins_distance_transform_is_scipys_bit_for_bit(golden):
    g = golden("dataset")
    names = json.loads(str(g["void_names"]))
    cases = twin.void_cases()
    assert names == [n for n in cases if n != "all_void_30x40"] and len(names) == 7
    for name in names:
        mask = np.isnan(cases[name][0])
        assert np.array_equal(mask, g["void_mask_" + name].astype(bool)), name
        got, want = twin.edt(mask), g["void_edt_" + name]
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, int((got != want).sum()))
    hole = g["void_edt_hole_150x170"]
    assert hole.max() > 32 and ((hole > 0) & (hole < 32)).sum() > 1000      # voids beyond the radius, and many inside it


@pytest.mark.parametrize("radius", [1, 5, 32, 64])
def test_the_capped_search_of_the_kernels_gives_the_exact_fill(radius):
    """Only d < radius matters: column distances capped at radius and a row pass over |dx| < radius give every void pixel the alpha of the
    exact distance transform, bit for bit in the stored value."""
    for name, (dem, base) in twin.void_cases().items():
        exact, voids = twin.fill_voids(dem, base, radius)
        capped = twin.fill_voids_capped(dem, base, radius)
        assert np.array_equal(exact.view(np.uint32), capped.view(np.uint32)), (name, radius)
        assert voids == int(np.isnan(dem).sum()) and not np.isnan(exact).any()
        valid = ~np.isnan(dem)
        assert np.array_equal(exact[valid].view(np.uint32), dem[valid].view(np.uint32))
    dem, base = twin.void_cases()["all_void_30x40"]
    assert np.array_equal(twin.fill_voids(dem, base, radius)[0].view(np.uint32), base.view(np.uint32))        # elevation_dataset.py:233


def test_the_twins_block_median_is_np_median_of_every_block(golden):
    g = golden("dataset")
    x = twin.median_input()
    assert np.array_equal(x.view(np.uint32), g["median_in"].view(np.uint32))
    for r in twin.MEDIAN_RS:
        got, want = twin.block_median(x, r), g[f"median_r{r}"]
        assert got.shape == want.shape == (96 // r, 192 // r) and got.dtype == F
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), r
        assert int(np.isnan(want).sum()) == 1                                  # the block with the NaN, and only that one
    # the even rule is fp32(a + b) * 0.5f: a pair whose sum rounds
    pair = np.array([[1.0, F(1.0) + F(2.0 ** -23)]], F)
    assert twin.block_median(np.tile(pair, (2, 1)), 2)[0, 0] == (pair[0, 0] + pair[0, 1]) * F(0.5)
    blocks = twin.blocks_of(x[:, 96:], 8)
    assert (np.array([len(np.unique(b)) for b in blocks.reshape(-1, 64)]) < 40).all()         # repeated values inside every block of the right half


def test_the_twins_welford_loop_against_the_reference_outputs(golden):
    g = golden("dataset")
    info = json.loads(str(g["stats"]))
    group = twin.stats_group()
    assert twin.group_crc(group) == info["crc"] and len(group) == info["chunks"] == 5
    assert group["0"]["chunk_0_0"]["residual"].array.size == info["n"] == 65536
    bound = summation_bound(info["n"]) * info["chunks"]
    g64 = twin.cast_group(group, np.float64)
    for name, tag, pct in stats_keys():
        m64, s64 = g[f"stats_{name}_f64_{tag}_means"], g[f"stats_{name}_f64_{tag}_stds"]
        m32, s32 = g[f"stats_{name}_f32_{tag}_means"], g[f"stats_{name}_f32_{tag}_stds"]
        means, stds = twin.welford(g64, name, pct)
        assert np.shape(means) == m64.shape and rel(means, m64) <= bound and rel(stds, s64) <= bound, (name, tag)
        # fed with float32 the reference's 2-D path subtracts and multiplies in float32 (means = 0.0 keeps data - means float32): its own distance
        # from its float64 run is what a float32-fed loop is held to
        means, stds = twin.welford(group, name, pct)
        assert rel(means, m64) <= rel(m32, m64) + bound and rel(stds, s64) <= rel(s32, s64) + bound, (name, tag)
    d = max(rel(g["stats_residual_f32_p0_means"], g["stats_residual_f64_p0_means"]), rel(g["stats_residual_f32_p0_stds"], g["stats_residual_f64_p0_stds"]))
    assert 1e-9 < d < 1e-6                                  # a float32 effect, far above the float64 bound
    assert d > 100 * bound and rel(g["stats_climate_f32_p0_stds"], g["stats_climate_f64_p0_stds"]) <= bound      # the 3-D path is float64 either way


# ------------------------------------------------------------------------------------------------------------------------------ the module's host halves
def test_running_stats_fed_with_summaries_is_the_twins_loop():
    group = twin.cast_group(twin.stats_group(), np.float64)
    bound = summation_bound(65536) * len(group)
    for name, planes in (("residual", None), ("climate", 3)):
        for pct in (0.0, 0.4):
            rs = ds.RunningStats(planes)
            for c in group:
                d = group[c]["chunk_0_0"][name]
                if d.attrs["pct_land"] >= pct:
                    rs.update(*twin.moments(d.array))
            means, stds = rs.result()
            wm, wsd = twin.welford(group, name, pct)
            assert np.shape(means) == np.shape(wm) and rel(means, wm) <= bound and rel(stds, wsd) <= bound, (name, pct)
    rs = ds.RunningStats(3)
    assert rs.update(0, np.zeros(3), np.zeros(3)) is rs and rs.count == 0                      # an empty chunk changes nothing
    with pytest.raises(ValueError, match="planes"):
        rs.update(5, np.zeros(2), np.zeros(2))
    one = ds.RunningStats().update(4, 2.5, 5.0).result()
    assert one == (2.5, np.sqrt(5.0 / 3.0)) and isinstance(one[0], np.float64)


def test_mask_voids_is_the_references_two_rules():
    import torch
    a = np.array([[-1000.5, -1000.0, 0.0, 12.0], [-32768.0, 5.5, -0.0, 3000.0]], np.float64)
    merit, cop = ds.mask_voids(a, "merit"), ds.mask_voids(a, "copernicus")
    assert merit.dtype == cop.dtype == F
    assert np.array_equal(np.isnan(merit), a < -1000) and np.array_equal(np.isnan(cop), a == 0.0)
    assert np.array_equal(merit[~np.isnan(merit)], a[a >= -1000].astype(F)) and np.array_equal(cop[~np.isnan(cop)], a[a != 0].astype(F))
    t = ds.mask_voids(torch.from_numpy(a), "merit")
    assert t.dtype == torch.float32 and np.array_equal(t.numpy(), merit, equal_nan=True)
    with pytest.raises(ValueError, match="merit"):
        ds.mask_voids(a, "srtm")


@pytest.mark.parametrize("num_chunks", [1, 2, 3])
@pytest.mark.parametrize("edge_margin", [0, 4])
def test_sub_chunk_boxes_equal_the_references_index_arithmetic(num_chunks, edge_margin):
    for highres_size, lowres_size in ((512, 64), (96, 12), (4096, 512), (70, 35)):
        if 2 * edge_margin >= lowres_size - num_chunks:
            continue
        margin, boxes = ds.chunk_boxes(highres_size, lowres_size, num_chunks, edge_margin)
        want_margin, want = twin.reference_boxes(highres_size, lowres_size, num_chunks, edge_margin)
        assert margin == want_margin == edge_margin * (highres_size // lowres_size) and boxes == want
        assert [b[0] for b in boxes] == [f"chunk_{i}_{j}" for i in range(num_chunks) for j in range(num_chunks)]
        side = (lowres_size - 2 * edge_margin) // num_chunks
        assert all(b[2][1] - b[2][0] == side == b[2][3] - b[2][2] for b in boxes)           # the sub-chunk td_dataset_land_counts counts over
    assert ds.chunk_boxes(4096, 512, 2, 4)[1][3] == ("chunk_1_1", (2016, 4032, 2016, 4032), (252, 504, 252, 504))


def test_header_entry_points_and_exports():
    import terrain_diffusion_amd as td
    import __graft_entry__ as ge
    text = open(os.path.join(ROOT, "include", "td_dataset.h")).read()
    declared = set(re.findall(r"\b(td_dataset_\w+)\s*\(", text))
    stated = {"td_dataset_last_error", "td_dataset_fill_voids", "td_dataset_block_median", "td_dataset_residual", "td_dataset_land_counts",
              "td_dataset_moments"}
    assert declared == set(ds.EXPORTS) == stated
    # every prototype's parameter count is the binding's: the stream first, `synchronize` last
    for name in stated - {"td_dataset_last_error"}:
        params = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")
        assert len(params) == len(ds._SIGS[name][1]), name
        assert params[0].strip() == "void* hip_stream" and params[-1].strip() == "int synchronize", name
        for p, ctype in zip(params, ds._SIGS[name][1]):
            assert ("*" in p) == (ctype is ds._P), (name, p)
    for macro, value in (("MAX_SIDE", 16384), ("MAX_RADIUS", 64), ("MAX_BLOCK", 32), ("MAX_CHUNKS", 64), ("MAX_PLANES", 1024)):
        assert re.search(rf"#define TD_DATASET_{macro} {value}\b", text) and getattr(ds, macro) == value
    assert re.search(r"#define TD_DATASET_MAX_ELEMENTS \(1 << 30\)", text) and ds.MAX_ELEMENTS == 1 << 30
    have = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", ds.LIB_PATH], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert stated <= have and not {n for n in have if n.startswith("td_") and n not in stated}
    ds.lib()     # binds every entry point
    for name in ("fill_voids", "block_median", "laplacian_encode", "land_share", "moments", "mask_voids", "prepare_chunks", "prepare_and_encode",
                 "RunningStats", "calculate_stats_welford"):
        assert getattr(td, name) is getattr(ds, name), name
    rows = {name: (sub, main, header, flags, module) for name, sub, main, header, flags, module in ge.SIDE_LIBS}
    assert rows["dataset"] == ("dataset_csrc", "dataset.hip", "td_dataset.h", ("-ffp-contract=off",), "dataset") and len(ge.SIDE_LIBS) == 7
    assert "dataset" not in ge.SIDE_SHARED                   # the void search has kernels of its own
    for phrase in ("PARITY-UNPINNED",):
        assert phrase in ds.__doc__ and phrase in twin.__doc__


def test_argument_checks_refuse_before_any_engine_is_touched(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(ds, "_engine_for", no_engine)
    x = np.zeros((12, 20), F)
    for r in (5, 7, 8):
        with pytest.raises(ValueError, match="does not divide"):
            ds.block_median(x, r)
    for r in (0, -1, 33):
        with pytest.raises(ValueError, match=r"r must be in 1 \.\. 32"):
            ds.block_median(x, r)
    for radius in (0, -3, 65):
        with pytest.raises(ValueError, match=r"radius must be in 1 \.\. 64"):
            ds.fill_voids(x, x, radius)
    with pytest.raises(ValueError, match="one shape"):
        ds.fill_voids(x, np.zeros((20, 12), F))
    for bad in (np.zeros(5, F), np.zeros((2, 3, 4), F)):
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            ds.fill_voids(bad, bad)
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            ds.block_median(bad, 1)
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            ds.laplacian_encode(bad, 4, 2.0)
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            ds.land_share(bad, 1)
    with pytest.raises(ValueError, match="limit"):
        ds.block_median(np.zeros((1, 16385), F), 1)
    with pytest.raises(ValueError, match="extrapolate=True"):
        ds.laplacian_encode(x, 4, 2.0, extrapolate=True)
    for mode in ("nearest", "bicubic", 3):
        with pytest.raises(ValueError, match="only bilinear"):
            ds.laplacian_encode(x, 4, 2.0, interp_mode=mode)
    with pytest.raises(ValueError, match="sigma must be positive"):
        ds.laplacian_encode(x, 4, 0.0)
    with pytest.raises(ValueError, match="low band"):
        ds.laplacian_encode(x, 0, 2.0)
    for nc in (0, 13, 65):
        with pytest.raises(ValueError, match="num_chunks must be in"):
            ds.land_share(x, nc)
    with pytest.raises(ValueError, match="at least one value"):
        ds.moments(np.zeros((3, 0, 4), F))
    with pytest.raises(ValueError, match="beyond the library's limit"):
        ds.moments(np.broadcast_to(F(0), (1025, 2, 2)))
    sq = np.zeros((96, 96), F)
    with pytest.raises(ValueError, match="square"):
        ds.prepare_chunks(x, x, 4, 2.0)
    with pytest.raises(ValueError, match="both are at highres_size"):
        ds.prepare_chunks(sq, np.zeros((48, 48), F), 12, 2.0)
    with pytest.raises(ValueError, match="multiple of lowres_size"):
        ds.prepare_chunks(sq, sq, 36, 2.0)
    with pytest.raises(ValueError, match="edge_margin"):
        ds.prepare_chunks(sq, sq, 12, 2.0, edge_margin=6)
    with pytest.raises(ValueError, match="num_chunks"):
        ds.prepare_chunks(sq, sq, 12, 2.0, num_chunks=5, edge_margin=4)
    with pytest.raises(ValueError, match="block median's limit"):
        ds.prepare_chunks(sq, sq, 2, 2.0)
    assert ds._lowres_size(100, 60, 30) == (50, 30) and ds._lowres_size(60, 100, 30) == (30, 50) and ds._lowres_size(60, 100, (7, 9)) == (7, 9)


def test_the_residual_bound_is_tight_enough_to_bite():
    """The bound E of twin.residual_ref on an fp32 emulation of the kernel's expression (every product and sum rounded on its own): it holds,
    it is within a factor 3 of the worst error seen, and an emulation with one tap's weight off by one ulp misses it."""
    rng = np.random.default_rng(5)
    low = (rng.standard_normal((12, 20)) * 30).astype(F)
    x = (rng.standard_normal((96, 160)) * 30).astype(F)

    def emu(nudge=False):
        i0, i1, wy0, wy1 = twin.bilinear_taps(12, 96)
        j0, j1, wx0, wx1 = twin.bilinear_taps(20, 160)
        if nudge:
            wx1 = np.nextafter(wx1, F(2)) + F(2.0 ** -20)
        a, b, c, d = low[i0][:, j0], low[i0][:, j1], low[i1][:, j0], low[i1][:, j1]
        top = (wx0[None] * a).astype(F) + (wx1[None] * b).astype(F)
        bot = (wx0[None] * c).astype(F) + (wx1[None] * d).astype(F)
        up = (wy0[:, None] * top).astype(F) + (wy1[:, None] * bot).astype(F)
        return (x - up).astype(F)
    ref, E = twin.residual_ref(x, low)
    worst = float((np.abs(emu().astype(np.float64) - ref) / E).max())
    assert 1 / 3 < worst <= 1.0, worst
    assert float((np.abs(emu(True).astype(np.float64) - ref) / E).max()) > 1.0
