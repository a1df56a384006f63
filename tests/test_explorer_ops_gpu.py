"""Every explorer kernel (explorer_csrc/explorer_kernels.hip) held to the twin (tests/_explorer_twin.py) element by element on the inputs of
tests/_explorer_shapes.py, which tests/test_explorer_ops_cpu.py holds to matplotlib, NumPy and torch: the colour kernel under explicit ranges
whose ends are no fp32 numbers, under its own range and under eight filters; the strided channel kernel past its first sweep; the quantiser at
every k / 255; raw tiles with odd pixel counts; the land-tile search at 1024, 1025 and 2080 blocks, at capacity 0, full to capacity and with
window counts that meet the threshold exactly.  Everything is exact (the log1p view within check_log1p_image's exemption), and every call runs
twice on the same device input."""
import numpy as np
import pytest
import torch

import _explorer_shapes as shapes
import _explorer_twin as twin
import test_explorer_cpu as cpu
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def ex():
    from terrain_diffusion_amd import explorer
    assert torch.cuda.is_available()
    return explorer


@pytest.fixture(scope="module")
def tables(golden):
    """name or (256, 3) table as colorize takes it -> the table the twin takes."""
    seeded = np.random.default_rng(9).random((256, 3)).astype(F)
    return [(n, lut) for n, lut in cpu.luts(golden("explorer")).items()] + [(seeded, seeded)]


def _up(a):
    return torch.from_numpy(np.array(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _twice(fn):
    """fn() -> tuple of device tensors, run twice on the same input: the first result as numpy arrays, the second equal to it byte for byte."""
    a = [_np(t) for t in fn()]
    b = [_np(t) for t in fn()]
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    return a


def _pixels_differ(got, want):
    return int((got != want).any(-1).sum())


def test_colorize_explicit_range(ex, tables):
    compared = 0
    for seed, (vmin, vmax) in enumerate(shapes.RANGES):
        d = shapes.colour_field(vmin, vmax, seed)
        dev = _up(d)
        for cmap, lut in tables:
            img, lo, hi = _twice(lambda: ex.colorize(dev, cmap, vmin=vmin, vmax=vmax))
            want = twin.colorize(d, lut, vmin=vmin, vmax=vmax)[0]
            assert img.shape == d.shape + (4,) and img.dtype == np.uint8
            assert np.array_equal(img, want), (vmin, vmax, _pixels_differ(img, want))
            assert lo.dtype == F and (float(lo), float(hi)) == (float(F(vmin)), float(F(vmax)))
            compared += d.size
    assert compared == 12 * 2479


def test_colorize_implicit_range(ex, tables):
    d = shapes.implicit_field()
    dev = _up(d)
    for cmap, lut in tables:
        img, lo, hi = _twice(lambda: ex.colorize(dev, cmap))
        want, vmin, vmax, _ = twin.colorize(d, lut)
        assert np.array_equal(img, want), _pixels_differ(img, want)
        assert (float(lo), float(hi)) == twin.nan_range(d) == (vmin, vmax)
    d = shapes.constant_field()
    img, lo, hi = _twice(lambda: ex.colorize(_up(d), "terrain"))
    want, vmin, vmax, _ = twin.colorize(d, tables[1][1])
    assert tables[1][0] == "terrain" and vmax == vmin + 1 and np.array_equal(img, want)
    assert np.array_equal(img, twin.colorize(d, tables[1][1], vmin=vmin, vmax=vmin + 1)[0])
    assert (float(lo), float(hi)) == twin.nan_range(d) and ex.resolved_range(lo, hi) == (vmin, vmax)
    img, lo, hi = _twice(lambda: ex.colorize(_up(shapes.all_nan_field()), "viridis"))
    assert not img.any() and np.isnan(lo) and np.isnan(hi)


def test_colorize_filters_all_eight_and_each_alone(ex, tables):
    (vmin, vmax), (cmap, lut) = shapes.RANGES[0], tables[0]
    d = shapes.colour_field(vmin, vmax, 0)
    dev = _up(d)
    host = shapes.filter_planes()
    device = [(_up(p), lo, hi) for p, lo, hi in host]
    plain = twin.colorize(d, lut, vmin=vmin, vmax=vmax)[0]
    for pick in [tuple(range(8))] + [(k,) for k in range(8)]:
        img, _, _ = _twice(lambda: ex.colorize(dev, cmap, vmin=vmin, vmax=vmax, filters=[device[k] for k in pick]))
        want = twin.colorize(d, lut, vmin=vmin, vmax=vmax, filters=[host[k] for k in pick])[0]
        assert np.array_equal(img, want), (pick, _pixels_differ(img, want))
        assert 0 < _pixels_differ(want, plain) < d.size
    img, lo, hi = _twice(lambda: ex.colorize(_up(shapes.implicit_field()), cmap, filters=device[:3]))     # the filters behind the device-side range
    assert np.array_equal(img, twin.colorize(shapes.implicit_field(), lut, filters=host[:3])[0])


def test_colorize_log1p(ex, tables):
    d = shapes.precip_field()
    cmap, lut = tables[0]
    img, lo, hi = _twice(lambda: ex.colorize(_up(d), cmap, log1p=True))
    want, vmin, vmax, margin = twin.colorize(d, lut, log1p=True)
    print(f"log1p view: {int((margin <= 4).sum())} of {margin.size} pixels within 4 ulp of a table boundary (cap {1e-3 * margin.size:.1f}); "
          f"{_pixels_differ(img, want)} pixels differ from the twin")
    cpu.check_log1p_image(img, want, margin, "precip")
    for got, w in ((float(lo), vmin), (float(hi), vmax)):
        assert abs(got - w) <= float(np.spacing(F(w))), (got, w)


@pytest.mark.parametrize("name,shape,signed", shapes.CHANNEL_CASES, ids=[c[0] for c in shapes.CHANNEL_CASES])
def test_coarse_channels(ex, name, shape, signed):
    sums = shapes.channel_sums(name)
    dev = _up(sums)
    compared = 0
    for eps in shapes.CHANNEL_EPS:
        for k in signed:
            planes, minmax = _twice(lambda: ex.coarse_channels(dev, n_signed_sq=k, eps=eps))
            want = twin.channels(sums, n_signed_sq=k, eps=eps)
            assert planes.shape == want.shape and planes.dtype == F
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(planes), nan), (name, eps, k)
            same = (planes.view(np.uint32) == want.view(np.uint32)) | nan
            first = same.reshape(shape[0] - 1, -1)[:, :shapes.CHANNELS_GRID_PIXELS]
            rest = same.reshape(shape[0] - 1, -1)[:, shapes.CHANNELS_GRID_PIXELS:]
            assert first.all(), (name, eps, k, "first sweep", int((~first).sum()))
            assert rest.all(), (name, eps, k, "flat index 262144 and above", int((~rest).sum()))
            for c in range(shape[0] - 1):
                lo, hi = twin.nan_range(want[c])
                got = minmax[c].tolist()
                assert (np.isnan(got[0]) and np.isnan(got[1])) if np.isnan(lo) else got == [lo, hi], (name, eps, k, c, got, lo, hi)    # either zero
            compared += want.size
    assert compared == 2 * len(signed) * sums[:-1].size
    if name == "stride":
        assert sums[0].size - shapes.CHANNELS_GRID_PIXELS == 8256
        allnan = np.array(sums)
        allnan[3] = np.nan
        _, minmax = _twice(lambda: ex.coarse_channels(_up(allnan)))
        assert np.isnan(minmax[3]).all() and not np.isnan(minmax[[0, 1, 2, 4, 5]]).any()


def test_relief_rgba8(ex):
    rgb = shapes.quantize_rgb()
    dev = _up(rgb)
    (img,) = _twice(lambda: (ex.relief_rgba8(dev),))
    want = twin.relief_rgba8(rgb)
    assert img.shape == (33, 31, 4) and np.array_equal(img, want), _pixels_differ(img, want)
    assert (img[..., 3] == 255).all()


@pytest.mark.parametrize("shape", shapes.RAW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_raw_tile(ex, shape):
    e, t = shapes.raw_tile(shape)
    de, dt = _up(e), _up(t)
    n = e.size
    assert np.array_equal(_np(dt).view(np.uint32), t.view(np.uint32))         # the upload kept the NaN payloads
    (body,) = _twice(lambda: (ex.raw_tile(de),))
    assert body.dtype == np.uint8 and body.size == 2 * n and body.tobytes() == twin.raw_tile(e)
    (body,) = _twice(lambda: (ex.raw_tile(de, dt),))
    assert body.size == 6 * n and body.tobytes() == twin.raw_tile(e, t), int((body != np.frombuffer(twin.raw_tile(e, t), np.uint8)).sum())


@pytest.mark.parametrize("name", list(shapes.LAND_CASES))
def test_land_tiles(ex, name):
    _, half, fracs = shapes.LAND_CASES[name]
    e = shapes.land_plane(name)
    dev = _up(e)
    cap = shapes.land_capacity(e.shape, half)
    for frac in fracs:
        idx, count = _twice(lambda: _counted(ex.land_tiles(dev, half, frac)))
        want = twin.land_tiles(e, half, frac)
        assert idx.dtype == np.int32 and int(count[0]) == len(want), (name, frac, int(count[0]), len(want))
        assert np.array_equal(idx, want), (name, frac)
        raw_idx, _ = ex.land_tiles(dev, half, frac)
        assert raw_idx.numel() == cap, (name, raw_idx.numel(), cap)
    if name in ("no_rows", "no_columns"):                  # 2 half == H or W: no position, no index buffer, count 0
        assert cap == 0 and raw_idx.numel() == 0 and int(count[0]) == 0
    if name == "all_land":
        assert len(twin.land_tiles(e, half, 1.0)) == cap == 17 * 31


def _counted(result):
    """(idx, count) -> (idx[:count], count): the slots past the count are not written."""
    idx, count = result
    return idx[:int(count)], count


def test_enqueue_only_on_a_caller_stream_gives_the_synchronous_result(ex):
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    _, half, (frac,) = shapes.LAND_CASES["blocks_2080"]
    dev = [_up(shapes.land_plane("blocks_2080")), _up(shapes.channel_sums("stride"))]

    def views(land, sums):
        idx, count = ex.land_tiles(land, half, frac)
        planes, minmax = ex.coarse_channels(sums, n_signed_sq=2, eps=1e-8)
        return [idx, count, planes, minmax]
    ref = views(*dev)
    s = torch.cuda.Stream()
    with eng.on_stream(s, asynchronous=True):
        x = [t * 1.0 for t in dev]                       # produced on the caller's stream, consumed there without a host sync
        got = [t.clone() for t in views(*x)]             # read on that stream after the calls
    torch.cuda.current_stream().synchronize()
    n = int(ref[1])
    assert int(got[1]) == n == len(twin.land_tiles(shapes.land_plane("blocks_2080"), half, frac))
    assert np.array_equal(_np(got[0][:n]), _np(ref[0][:n]))
    for a, b in zip(got[2:], ref[2:]):
        assert _np(a).tobytes() == _np(b).tobytes()
