"""The explorer twin (tests/_explorer_twin.py) held to the operator definitions -- matplotlib's Normalize, colormap call and imsave, NumPy's
comparisons with Python-float bounds, torch's division and mean on the CPU, np.floor / np.clip -- on exactly the inputs of
tests/_explorer_shapes.py that tests/test_explorer_ops_gpu.py holds the kernels to; and the proof that those inputs are sharp: eight wrong
variants of the operations, each a few lines here, differ from the twin on them, and four of the eight pass every recorded case of
tests/golden/explorer.npz."""
import io

import numpy as np
import pytest
import torch

import _explorer_shapes as shapes
import _explorer_twin as twin
import test_explorer_cpu as cpu

F = np.float32
EXPLICIT = [(vmin, vmax, shapes.colour_field(vmin, vmax, seed)) for seed, (vmin, vmax) in enumerate(shapes.RANGES)]


def _words(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ the inputs are what they say
def test_the_inputs_hold_the_edges_they_are_built_for():
    for vmin, vmax, d in EXPLICIT:
        assert d.size % 256 and d.shape[0] >= 37 and d.shape[1] >= 67
        x = twin.normalize(d, vmin, vmax)
        xa = x * F(256)
        assert (xa == 256).any() and (xa < 0).any() and (xa > 256).any() and np.isnan(xa).any() and np.isinf(d).sum() >= 2
        assert float(F(vmin)) != vmin and float(F(vmax)) != vmax and (d == F(vmin)).any() and (d == F(vmax)).any()
        idx = np.where(np.isnan(xa), -1, np.clip(np.where(np.isnan(xa), 0, xa), 0, 255)).astype(int)
        assert set(range(256)) <= set(idx.ravel().tolist())                       # every table entry is used
        margin = twin.lookup(x, np.zeros((256, 3), F))[1]
        assert (margin == 0).sum() >= 100                                         # pixels exactly on a boundary between two entries
    d = shapes.implicit_field()
    assert (twin.lookup(twin.normalize(d, *twin.view_range(d)), np.zeros((256, 3), F))[1] == 0).sum() >= 100
    assert twin.view_range(shapes.constant_field()) == (float(F(7.3)), float(F(7.3)) + 1) and np.isnan(shapes.all_nan_field()).all()
    for plane, lo, hi in shapes.filter_planes():
        ok = twin.passes(plane, lo, hi)
        assert plane.shape == shapes.COLOUR_SHAPE and 0.5 * ok.size < ok.sum() < ok.size and np.isnan(plane).any() and np.isinf(plane).sum() >= 2
        for b in (lo, hi):
            if b is not None and np.isfinite(b):
                assert (plane == F(b)).any() and (plane == np.nextafter(F(b), F(np.inf))).any() and (plane == np.nextafter(F(b), -F(np.inf))).any()
    every = np.logical_and.reduce([twin.passes(*f) for f in shapes.filter_planes()])
    assert 0.25 * every.size < every.sum() < 0.75 * every.size
    assert len(shapes.filter_planes()) == 8 and any(float(F(lo)) != lo for _, lo, _ in shapes.filter_planes() if lo is not None)
    for name, shape, _ in shapes.CHANNEL_CASES:
        s = shapes.channel_sums(name)
        assert s.shape == shape and s.dtype == F
        with np.errstate(all="ignore"):
            q = twin.channels(s, n_signed_sq=0, eps=0.0)
            sq = twin.channels(s, n_signed_sq=shape[0] - 1, eps=0.0)
        tiny = np.finfo(F).tiny
        assert np.isnan(q).any() and np.isinf(q).any() and ((sq != 0) & (np.abs(sq) < tiny)).any() and (np.isinf(sq) & ~np.isinf(q)).any()
        assert (s[-1] == 0).any() and (s[-1] < 0).any() and np.isnan(s[-1]).any() and ((s[-1] != 0) & (np.abs(s[-1]) < tiny)).any()
    big = shapes.channel_sums("stride")
    assert big[0].size > shapes.CHANNELS_GRID_PIXELS and np.isnan(big[-1].ravel()[shapes.CHANNELS_GRID_PIXELS:]).any()
    rgb = shapes.quantize_rgb()
    assert rgb.shape == (33, 31, 3) and set(range(256)) <= set(twin.quantize(rgb).ravel().tolist())
    assert (np.isnan(rgb).sum(-1) == 1).sum() >= 3 and np.isin(shapes.quantize_steps(), rgb).all() and np.isinf(rgb).sum() >= 2
    for shape in shapes.RAW_SHAPES:
        e, t = shapes.raw_tile(shape)
        assert e.shape == t.shape == shape and e.size % 2 == 1 and (e.size < 256 or e.size % 256)
    e, t = shapes.raw_tile((255, 257))
    assert np.isin(_words(shapes.RAW_ELEV_EDGES), _words(e)).all() and np.isin(shapes.RAW_TEMP_WORDS, _words(t)).all()
    assert ((e > -1) & (e < 0)).sum() > 1000 and e.size > 256
    blocks = {n: -(-shapes.land_plane(n).size // 256) for n in ("blocks_1024", "blocks_1025", "blocks_2080")}
    assert blocks == {"blocks_1024": 1024, "blocks_1025": 1025, "blocks_2080": 2080}
    for n in blocks:
        (_, half, (frac,)), e = shapes.LAND_CASES[n], shapes.land_plane(n)
        assert 0.25 <= len(twin.land_tiles(e, half, frac)) / shapes.land_capacity(e.shape, half) <= 0.75, n
    assert shapes.land_plane("blocks_1025").shape[0] == 5 and shapes.land_plane("blocks_2080").shape == (1024, 520)
    for n, (_, half, _) in shapes.LAND_CASES.items():
        e = shapes.land_plane(n)
        assert half <= 64 and e.size <= 550000
    assert shapes.land_capacity((40, 130), 20) == 0 == shapes.land_capacity((130, 40), 20) and shapes.land_capacity((41, 130), 20) == 90
    sub = shapes.land_plane("subnormal")
    assert set(_words(sub).ravel().tolist()) == set(_words(np.array([1e-40, -0.0, 0.0, -1e-40, np.nan], F)).tolist())


# ----------------------------------------------------------------------------------------------------------------------- twin against matplotlib
def test_twin_colours_equal_matplotlib_on_every_colour_field():
    mpl = pytest.importorskip("matplotlib")
    fields = [(d, vmin, vmax) for vmin, vmax, d in EXPLICIT]
    fields += [(d,) + twin.view_range(d) for d in (shapes.implicit_field(), shapes.constant_field(), shapes.all_nan_field())]
    compared = 0
    for d, vmin, vmax in fields:
        for name in ("viridis", "terrain", "RdBu_r"):
            with np.errstate(all="ignore"):
                want = mpl.colormaps[name](mpl.colors.Normalize(vmin=vmin, vmax=vmax)(d)).astype(F)
            got, _ = twin.lookup(twin.normalize(d, vmin, vmax), mpl.colormaps[name](np.arange(256))[:, :3].astype(F))
            assert np.array_equal(_words(got), _words(want)), (name, vmin, vmax, int((got != want).any(-1).sum()))
            compared += d.size
    assert compared == 18 * 2479


def test_twin_quantize_equals_what_imsave_writes():
    mpl = pytest.importorskip("matplotlib")
    pytest.importorskip("PIL.Image")
    mpl.use("Agg")
    import matplotlib.pyplot as plt
    rgb = shapes.quantize_rgb()
    inside = np.where((rgb >= 0) & (rgb <= 1), rgb, F(0.5))                 # imsave refuses floats outside [0, 1]
    assert np.isin(shapes.quantize_steps()[(shapes.quantize_steps() >= 0) & (shapes.quantize_steps() <= 1)], inside).all()
    rgba = np.concatenate([inside, np.ones(rgb.shape[:2] + (1,), F)], axis=-1)
    buf = io.BytesIO()
    plt.imsave(buf, rgba, format="png")
    wrote = twin.decode_png(buf.getvalue())
    assert np.array_equal(wrote, twin.quantize(rgba)) and np.array_equal(wrote, twin.relief_rgba8(inside))


def test_twin_filter_is_numpys_comparison_with_the_python_float_bound():
    """server.py: `mask &= ch_data >= lo` on an fp32 array with lo = request.args.get(..., type=float)."""
    for plane, lo, hi in shapes.filter_planes():
        want = np.ones(plane.shape, bool)
        with np.errstate(invalid="ignore"):
            if lo is not None:
                want &= plane >= lo
            if hi is not None:
                want &= plane <= hi
        assert np.array_equal(twin.passes(plane, lo, hi), want), (lo, hi)


def test_twin_alone_stays_under_the_log1p_cap():
    d = shapes.precip_field()
    shown = twin.display(d, True)
    margin = twin.lookup(twin.normalize(shown, *twin.view_range(shown)), np.zeros((256, 3), F))[1]
    assert (margin <= 4).sum() <= 1e-3 * margin.size, int((margin <= 4).sum())
    assert (d < 0).sum() > 100 and np.isnan(d).sum() == 2


# ------------------------------------------------------------------------------------------------------------------------------ twin against torch
def test_twin_channels_are_bit_equal_to_torch_on_the_new_sums():
    for name, shape, signed in shapes.CHANNEL_CASES:
        block = torch.from_numpy(shapes.channel_sums(name).copy())
        for eps in shapes.CHANNEL_EPS:
            for k in signed:
                want = block[:-1] / (block[-1:] + eps) if eps else block[:-1] / block[-1:]
                want[:k] = torch.sign(want[:k]) * torch.square(want[:k])
                got = twin.channels(block.numpy(), n_signed_sq=k, eps=eps)
                want = want.numpy()
                assert np.array_equal(np.isnan(got), np.isnan(want)), (name, eps, k)
                assert np.array_equal(_words(got)[~np.isnan(got)], _words(want)[~np.isnan(want)]), (name, eps, k)


def _double_loop(elev_m, half, min_land_frac):
    """random_sampler.sample_land_tiles' search, literally."""
    land_mask = (torch.from_numpy(np.array(elev_m)) > 0).float()
    H, W = land_mask.shape
    out = []
    for i in range(half, H - half):
        for j in range(half, W - half):
            if land_mask[i - half:i + half, j - half:j + half].mean().item() >= min_land_frac:
                out.append(i * W + j)
    return np.array(out, np.int64)


def test_twin_land_tiles_equal_the_literal_double_loop():
    for name in shapes.LAND_SMALL:
        _, half, fracs = shapes.LAND_CASES[name]
        e = shapes.land_plane(name)
        for frac in fracs:
            assert np.array_equal(twin.land_tiles(e, half, frac), _double_loop(e, half, frac)), (name, frac)
    for name, frac in shapes.LAND_ON_THE_BOUNDARY:       # on the boundary: the fp32 mean and the exact fraction fall on different sides
        e, half = shapes.land_plane(name), shapes.LAND_CASES[name][1]
        a, b = twin.land_tiles(e, half, frac), twin.land_tiles(e, half, frac, exact=True)
        assert {len(a), len(b)} == {0, shapes.land_capacity(e.shape, half)}, (name, len(a), len(b))
    for name in ("half_64_at_050", "half_64_at_075"):    # met exactly: every position at the fraction, none one ulp above it
        _, half, (frac, above) = shapes.LAND_CASES[name]
        e = shapes.land_plane(name)
        assert len(twin.land_tiles(e, half, frac)) == shapes.land_capacity(e.shape, half) == 72 * 132 and float(F(frac)) == frac
        assert len(twin.land_tiles(e, half, above)) == 0
        for i, j in ((64, 64), (100, 131), (135, 195)):
            assert (e[i - 64:i + 64, j - 64:j + 64] > 0).mean() == frac
    full = twin.land_tiles(shapes.land_plane("all_land"), 3, 1.0)
    assert np.array_equal(full, (np.arange(3, 20)[:, None] * 37 + np.arange(3, 34)[None, :]).ravel())
    assert len(twin.land_tiles(shapes.land_plane("all_land"), 3, shapes.UP)) == 0 == len(twin.land_tiles(shapes.land_plane("all_sea"), 3, 0.5))


def test_twin_compaction_in_rounds_is_the_ascending_index_list():
    for name in ("blocks_1024", "blocks_1025", "blocks_2080", "subnormal"):
        _, half, fracs = shapes.LAND_CASES[name]
        e = shapes.land_plane(name)
        want = twin.land_tiles(e, half, fracs[0])
        valid = np.zeros(e.size, bool)
        valid[want] = True
        idx, count = twin.compact(valid.reshape(e.shape))
        assert count == len(want) and np.array_equal(idx, want), name


def test_twin_raw_tiles_are_floor_clip_and_the_temperature_bytes():
    for shape in shapes.RAW_SHAPES:
        e, t = shapes.raw_tile(shape)
        with np.errstate(invalid="ignore"):
            body = np.clip(np.floor(np.where(np.isnan(e), F(0), e)), -32768, 32767).astype("<i2").tobytes()
        assert twin.raw_tile(e) == body and len(body) == 2 * e.size
        assert twin.raw_tile(e, t) == body + t.tobytes() and len(twin.raw_tile(e, t)) == 6 * e.size
        assert np.array_equal(np.frombuffer(twin.raw_tile(e, t)[2 * e.size:], np.uint32), _words(t).ravel())
    first = np.frombuffer(twin.raw_tile(*shapes.raw_tile((17, 15)))[:34], "<i2").tolist()
    assert first == [-1, 32767, -32768, 0, -1, 0, 32767, -32768, 32767, -32768, -1, 0, 32767, -32768, -4, 32767, 0]


# ------------------------------------------------------------------------------------------------------------------------------------ sharpness
LOOKUP, NORMALIZE, LAND, RELIEF = twin.lookup, twin.normalize, twin.land_tiles, twin.relief_rgba8


def _lookup_without_the_256_case(x, lut):
    """matplotlib's order is `xa[xa == N] = N - 1`, then `over = xa >= N`: without the first line x == 1 is over the range.  The over colour is
    a row of its own (here: black), as it is once set_over is used; with the default over colour, which is row 255, and so with a kernel that
    clamps at xa >= 256, the line changes nothing."""
    rgba, margin = LOOKUP(x, lut)
    with np.errstate(invalid="ignore"):
        rgba[x * F(256) == 256, :3] = 0
    return rgba, margin


def _normalize_with_fp32_vmin(d, vmin, vmax):
    return NORMALIZE(d, float(F(vmin)), vmax)


def _passes_strictly_above(plane, lo, hi):
    mask = np.ones(np.shape(plane), bool)
    with np.errstate(invalid="ignore"):
        if lo is not None:
            mask &= np.asarray(plane, F) > F(lo)
        if hi is not None:
            mask &= np.asarray(plane, F) <= F(hi)
    return mask


def _raw_truncated(elev, temp=None):
    with np.errstate(invalid="ignore"):
        e = np.clip(np.trunc(np.asarray(elev, F)), -32768, 32767)
    return np.where(np.isnan(e), 0, e).astype("<i2").tobytes() + (np.asarray(temp).astype("<f4").tobytes() if temp is not None else b"")


def _relief_rounded(rgb):
    """ex_quantize_kernel alone (the relief image); the colour kernel's channels keep the truncation."""
    out = RELIEF(rgb)
    with np.errstate(invalid="ignore"):
        c = np.rint(np.clip(np.asarray(rgb, F), 0, 1) * F(255))
    out[..., :3] = np.where(np.isnan(c), 0, c).astype(np.uint8)
    return out


def _land_inclusive_columns(elev_m, half, min_land_frac, exact=False):
    land = (np.asarray(elev_m, F) > 0).astype(np.int64)
    H, W = land.shape
    out = []
    for i in range(half, H - half) if half else ():
        for j in range(half, W - half):
            c = land[i - half:i + half, j - half:j + half + 1].sum()
            if float(F(c) / F(4 * half * half)) >= min_land_frac:
                out.append(i * W + j)
    return np.array(out, np.int64)


def _land_exact(elev_m, half, min_land_frac, exact=False):
    return LAND(elev_m, half, min_land_frac, exact=True)


def _offsets_dropping_the_carry(counts, round_size=1024):
    """Each round starts from the sum of the round before it alone: right for two rounds, wrong from the third on."""
    counts = np.asarray(counts, np.int64)
    out, carry = np.zeros(counts.size, np.int64), 0
    for base in range(0, counts.size, round_size):
        part = counts[base:base + round_size]
        out[base:base + round_size] = carry + np.cumsum(part) - part
        carry = int(part.sum()) + (carry if base == 0 else 0)
    return out, int(counts.sum())


def _land_through_the_dropped_carry(elev_m, half, min_land_frac, exact=False):
    valid = np.zeros(np.asarray(elev_m).size, bool)
    valid[LAND(elev_m, half, min_land_frac, exact)] = True
    return twin.compact(valid.reshape(np.shape(elev_m)), offsets=_offsets_dropping_the_carry)[0]


def _colour_views(luts):
    out = [twin.colorize(d, luts["terrain"], vmin=vmin, vmax=vmax)[0] for vmin, vmax, d in EXPLICIT]
    vmin, vmax, d = EXPLICIT[0]
    fl = shapes.filter_planes()
    return out + [twin.colorize(d, luts["viridis"], vmin=vmin, vmax=vmax, filters=f)[0] for f in (fl,) + tuple((f,) for f in fl)]


def _raw_views():
    return [twin.raw_tile(*shapes.raw_tile(s)) for s in shapes.RAW_SHAPES]


def _relief_views():
    return [twin.relief_rgba8(shapes.quantize_rgb())]


def _land_views(names):
    return [twin.land_tiles(shapes.land_plane(n), shapes.LAND_CASES[n][1], f) for n in names for f in shapes.LAND_CASES[n][2]]


# (kernel, variant): the attribute of the twin it replaces, the variant, the views of the new inputs it must change, the recorded-case tests
VARIANTS = {
    ("colour", "no xa == 256 -> 255 case"): ("lookup", _lookup_without_the_256_case, "colour", ("coarse", "detail")),
    ("colour", "vmin rounded to fp32 before the subtraction"): ("normalize", _normalize_with_fp32_vmin, "colour", ("coarse", "detail")),
    ("colour", "filter > for >="): ("passes", _passes_strictly_above, "colour", ("coarse",)),
    ("raw", "truncation for floor"): ("raw_tile", _raw_truncated, "raw", ("detail",)),
    ("quantize", "round-to-nearest for truncation"): ("relief_rgba8", _relief_rounded, "relief", ("detail",)),
    ("land", "window [j - half, j + half] inclusive"): ("land_tiles", _land_inclusive_columns, "land_small", ("land",)),
    ("land", "exact fraction for the fp32 mean"): ("land_tiles", _land_exact, "land_small", ("land",)),
    ("land", "a scan that drops the carry after the second 1024 blocks"): ("land_tiles", _land_through_the_dropped_carry, "land_blocks", ("land",)),
}
ONLY_THE_NEW_INPUTS_CATCH = {("colour", "vmin rounded to fp32 before the subtraction"), ("colour", "filter > for >="),
                             ("quantize", "round-to-nearest for truncation"), ("land", "a scan that drops the carry after the second 1024 blocks")}


def _same(a, b):
    return all((x == y) if isinstance(x, bytes) else np.array_equal(x, y) for x, y in zip(a, b))


def test_eight_wrong_variants_fail_the_new_inputs_and_four_pass_every_recorded_case(golden, monkeypatch):
    """Each wrong variant replaces one function of the twin.  All eight change what the twin gives on the new inputs.  On the recorded cases
    of explorer.npz (the twin's own tests of tests/test_explorer_cpu.py, run with the variant in place):

      caught by the recorded cases already      no xa == 256 -> 255 case (every implicit range has its maximum at x == 1; only where the over
                                                colour is not row 255: see _lookup_without_the_256_case), truncation for floor (-0.25 and
                                                -3.75 are recorded), the inclusive window, the exact fraction (the 70-of-100 windows)
      pass every recorded case, fail the new    vmin rounded to fp32 (a recorded range is the field's own, so fp32 already), filter > for >= (no
                                                recorded bound is met exactly), round-to-nearest in the relief quantisation (relief images are
                                                compared within one level), the dropped carry (no recorded plane has more than 1024 blocks)"""
    luts = cpu.luts(golden("explorer"))
    views = {"colour": lambda: _colour_views(luts), "raw": _raw_views, "relief": _relief_views,
             "land_small": lambda: _land_views(("seven_in_ten", "twentyfive_in_36", "one_row", "subnormal")),
             "land_blocks": lambda: _land_views(("blocks_1024", "blocks_1025", "blocks_2080"))}
    right = {k: fn() for k, fn in views.items()}
    recorded = {"coarse": cpu.test_twin_matches_every_recorded_coarse_case, "detail": cpu.test_twin_matches_every_recorded_detail_case,
                "land": cpu.test_twin_matches_every_recorded_land_case_and_the_fp32_mean_matters}
    for fn in recorded.values():
        fn(golden)
    only_new = set()
    for key, (attr, wrong, view, tests) in VARIANTS.items():
        with monkeypatch.context() as m:
            m.setattr(twin, attr, wrong)
            assert not _same(views[view](), right[view]), ("the new inputs do not catch", key)
            try:
                for t in tests:
                    recorded[t](golden)
                only_new.add(key)
            except AssertionError:
                pass
    assert only_new == ONLY_THE_NEW_INPUTS_CATCH and len(only_new) >= 4, sorted(only_new)
    wrong = [twin.land_tiles(shapes.land_plane(n), 2, 0.5) for n in ("blocks_1024", "blocks_1025")]
    with monkeypatch.context() as m:                       # the dropped carry shows at three rounds only: one and two rounds stay right
        m.setattr(twin, "land_tiles", _land_through_the_dropped_carry)
        assert _same([twin.land_tiles(shapes.land_plane(n), 2, 0.5) for n in ("blocks_1024", "blocks_1025")], wrong)
