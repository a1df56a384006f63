"""The custom-map import on the GPU (include/td_custom.h, custom_csrc/custom_kernels.hip): the rasteriser, the nearest-valid fill and the int16
export bit for bit against the NumPy twin (tests/_custom_twin.py) and against every fill recorded from the reference's fill_nodata
(tests/golden/custom.npz), determinism, the enqueue-only stream mode, the C-ABI's refusals, the Azgaar drop-ins against the twin, and the
import -> export round trip on a stub world and on a WorldPipeline with the tiny synthetic models."""
import ctypes as C

import numpy as np
import pytest
import torch

import _custom_twin as twin
import test_custom_cpu as cpu
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def cw():
    from terrain_diffusion_amd import custom_world
    assert torch.cuda.is_available()
    return custom_world


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check_raster(cw, xy, offsets, values, shape, fill, what):
    got = cw.rasterize_cells(xy, offsets, values, shape, fill)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == tuple(shape)
    want = twin.rasterize(xy, offsets, values, shape, fill)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (what, int((bits(got.cpu().numpy()) != bits(want)).sum()))
    return want


def values_for(n):
    return (np.arange(n, dtype=F) * F(0.37) - F(11)).astype(F)


# ------------------------------------------------------------------------------------------------------------------------------ rasteriser
@pytest.mark.parametrize("n_sites,shape", [(400, (96, 160)), (5000, (97, 131)), (30, (2, 300)), (5, (1, 1))])
def test_voronoi_cells_against_the_twin(cw, n_sites, shape):
    H, W = shape
    sites, vertices, rings = twin.voronoi_cells(n_sites, W, H, seed=n_sites)
    xy, offsets = twin.csr_of(vertices, rings)
    want = check_raster(cw, xy, offsets, values_for(n_sites), shape, np.nan, shape)
    assert not np.isnan(want).any()          # the cells tile the raster: nothing is left to the fill


def star(n_vertices, cx, cy, r_out, r_in):
    a = np.arange(n_vertices) * (2 * np.pi / n_vertices) + 0.1
    r = np.where(np.arange(n_vertices) % 2 == 0, r_out, r_in)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1)


def csr(rings):
    rings = [np.asarray(r, np.float64).reshape(-1, 2) for r in rings]
    return np.concatenate(rings), np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)


def test_hand_made_polygons_against_the_twin(cw):
    square = lambda x0, y0, x1, y1: [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]
    concave = [[5, 5], [45, 5], [45, 40], [25, 15], [5, 40]]                       # a notch from below
    three = [square(10.2, 8.7, 50.4, 30.1), concave, [[20.5, 2.5], [60.5, 20.5], [18.5, 38.5]]]
    cases = {
        # the later polygon wins: both orders, with values that tell the polygons apart
        "overlap": (three, (48, 70), -1.0),
        "overlap_reversed": (three[::-1], (48, 70), -1.0),
        # partly outside on every side, wholly outside, and one that covers the raster
        "outside": ([square(-20, -20, 7.5, 9.5), square(30, 20, 90, 90), square(-50, 3, -1, 9), square(3, 41, 9, 80), square(100, 0, 120, 10),
                     [[-1e3, -1e3], [1e3, -1e3], [0, 14]]], (40, 36), np.nan),
        "covers_all": ([square(-5, -5, 500, 500)], (33, 65), 0.0),
        # a 300-vertex star: a ring far beyond 64 vertices, on a raster large enough that several waves share its bounding box
        "star": ([star(300, 75.3, 70.8, 69.0, 30.0)], (150, 151), np.nan),
        # a ring of 2 vertices burns nothing; neither does an empty one; the triangle behind them does
        "two_vertices": ([[[1, 1], [30, 30]], np.zeros((0, 2)), [[2, 2], [20, 3], [4, 25]]], (32, 32), -9999.0),
        # a bounding box wider than 64 pixels on a width that is no multiple of 64
        "wide": ([[[3.2, 1.1], [193.7, 4.4], [150.0, 8.8], [10.0, 6.0]]], (10, 200), np.nan),
        # coordinates beyond the bounding-box shortcut, and not finite: the whole raster is tested, as the twin does
        "wild": ([[[-1e12, 3], [20.5, 3.3], [20.5, 30]], [[5, 5], [np.nan, 9], [9, 25], [30, 8]], [[2, 2], [np.inf, 2], [2, 20]], square(40, 5, 50, 15)],
                 (36, 60), np.nan),
        # 1 x 1: the centre (0.5, 0.5) inside, and just outside
        "one_pixel_in": ([[[0.2, 0.2], [0.9, 0.3], [0.4, 0.9]]], (1, 1), np.nan),
        "one_pixel_out": ([[[0.6, 0.6], [0.9, 0.6], [0.7, 0.9]]], (1, 1), -3.0),
    }
    for name, (rings, shape, fill) in cases.items():
        xy, offsets = csr(rings)
        want = check_raster(cw, xy, offsets, values_for(len(rings)) + F(100), shape, fill, name)
        if name == "overlap":
            assert set(np.unique(want).tolist()) == {-1.0, *(values_for(3) + F(100)).tolist()}
        if name == "one_pixel_in":
            assert want[0, 0] == values_for(1)[0] + F(100)
        if name in ("one_pixel_out",):
            assert want[0, 0] == F(fill)
    # n = 0: all fill, with and without arrays
    for fill in (np.nan, 2.5):
        got = cw.rasterize_cells(np.zeros((0, 2)), [0], [], (7, 9), fill).cpu().numpy()
        assert np.array_equal(bits(got), bits(np.full((7, 9), fill, F)))
    # device inputs give the host inputs' bits
    xy, offsets = csr(three)
    a = cw.rasterize_cells(xy, offsets, values_for(3), (48, 70), np.nan)
    b = cw.rasterize_cells(torch.from_numpy(xy).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(values_for(3)).cuda(), (48, 70), np.nan)
    assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))


# ------------------------------------------------------------------------------------------------------------------------------ nearest fill
def test_every_recorded_fill_through_fill_nearest_and_fill_nodata(cw, golden):
    g = golden("custom")
    n = 0
    for name, a, nodata, want in cpu.fill_cases(g):
        got = cw.fill_nearest(a, nodata)
        assert got.dtype == torch.float32 and got.is_cuda
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (name, "fill_nearest")
        drop = cw.fill_nodata(a, nodata)
        assert isinstance(drop, np.ndarray) and drop.dtype == F and np.array_equal(bits(drop), bits(want)), (name, "fill_nodata")
        if name == "no_hole":
            assert drop is a
        out, index = cw.fill_nearest(torch.from_numpy(a).cuda(), nodata, return_index=True)
        assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy(), twin.fill_sources(a, nodata)), name
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))
        n += 1
    assert n == 8


def chunk_cases():
    """Widths around CW_FILL_CHUNK = 1024, the columns of the column plane that cw_fill_rows_kernel stages in LDS at a time: 1025 is the
    smallest width with a second chunk."""
    rng = np.random.default_rng(77)
    # three valid pixels: every hole scans the whole row of column distances, across the chunk boundary, in both directions
    a = np.full((3, 1025), np.nan, F)
    a[0, 2], a[1, 500], a[2, 1024] = 1.0, 2.0, 3.0
    yield "three_valid_1025", a, np.nan
    # holes whose search radius straddles the boundary: scattered holes, a block of them over columns 1000..1050, and an empty column 1024
    b = (rng.integers(0, 1000, (10, 1100))).astype(F)
    b[rng.random(b.shape) < 0.5] = -9999.0
    b[2:9, 1000:1051] = -9999.0
    b[:, 1024] = -9999.0
    yield "straddle_1100", b, -9999.0
    c = np.arange(2 * 1024, dtype=F).reshape(2, 1024)
    c[:, 1:1023] = np.nan
    yield "exactly_1024", c, np.nan


def test_fill_across_the_column_chunk_and_the_index_plane(cw):
    for name, a, nodata in chunk_cases():
        src = twin.fill_sources(a, nodata)
        out, index = cw.fill_nearest(a, nodata, return_index=True)
        assert np.array_equal(index.cpu().numpy(), src), name
        assert np.array_equal(bits(out.cpu().numpy()), bits(a.reshape(-1)[src])), name
    # -0.0 and inf are values and travel as bits: (0, 1) is tied between columns 0 and 2 and takes column 0's -0.0, (1, 1) is nearest to (1, 2)
    v = np.array([[-0.0, np.nan, 5.0], [np.nan, np.nan, np.inf]], F)
    got = cw.fill_nearest(v).cpu().numpy()
    assert np.array_equal(bits(got), bits(np.array([[-0.0, -0.0, 5.0], [-0.0, np.inf, np.inf]], F)))
    assert np.array_equal(bits(got), bits(twin.fill_nearest(v)))
    # a NaN is invalid under a sentinel too; the sentinel is compared in float32
    s = np.array([[1.0, np.nan, -9999.0, 4.0]], F)
    assert cw.fill_nearest(s, -9999.0).cpu().tolist() == [[1.0, 1.0, 4.0, 4.0]]
    assert np.array_equal(bits(cw.fill_nearest(s).cpu().numpy()), bits(np.array([[1.0, 1.0, -9999.0, 4.0]], F)))
    for empty, nodata in ((np.full((5, 7), np.nan, F), np.nan), (np.full((1, 1), -9999.0, F), -9999.0)):
        with pytest.raises(ValueError, match="no valid pixel"):
            cw.fill_nearest(empty, nodata)
        with pytest.raises(ValueError, match="no valid pixel"):
            cw.fill_nodata(empty, nodata)


# ------------------------------------------------------------------------------------------------------------------------------ int16 export
def elevations():
    rng = np.random.default_rng(9)
    edge = [0.5, -0.5, 0.999, -0.999, 32767.5, -32767.5, 40000.0, -40000.0, np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0, -1.0, 32767.0, -32768.0,
            32766.999, -32768.5, 1e-30, -1e-30, 3.4e38, -3.4e38]
    return np.concatenate([np.array(edge, F), (rng.standard_normal(10000) * 20000).astype(F)])


def test_elevation_int16_clips_then_truncates(cw):
    e = elevations()
    want = twin.elev_int16(e)
    assert want[:11].tolist() == [0, 0, 0, 0, 32767, -32767, 32767, -32768, 32767, -32768, 0]
    assert not np.array_equal(want, np.clip(np.floor(np.nan_to_num(e)), -32768, 32767).astype(np.int16))     # not explorer.raw_tile's floor
    got = cw.elevation_int16(e)
    assert got.dtype == torch.int16 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    d = torch.from_numpy(e).cuda()
    for view in (d[1:], d[: e.size - 1], d[3:10], d[:1], d[:4], d[: 4 * 2500].reshape(100, 100), d[:0]):      # unaligned starts, odd tails, a plane, nothing
        got = cw.elevation_int16(view)
        assert tuple(got.shape) == tuple(view.shape) and np.array_equal(got.cpu().numpy(), twin.elev_int16(view.cpu().numpy())), tuple(view.shape)


# ------------------------------------------------------------------------------------------------------------------------------ the library as a whole
def _everything(cw, golden, inputs=None):
    g = golden("custom")
    if inputs is None:
        sites, vertices, rings = twin.voronoi_cells(400, 160, 96, seed=400)
        xy, offsets = twin.csr_of(vertices, rings)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        inputs = [up(xy), up(offsets), up(values_for(400)), up(g["fill_in_scattered_nan"]), up(elevations())]
    xy, offsets, values, holes, elev = inputs
    raster = cw.rasterize_cells(xy, offsets, values, (96, 160), np.nan)
    out, index, valid = cw._fill(cw._engine_for(holes, None)[0], holes.device, holes, float("nan"), True)
    return inputs, [raster, out, index, valid, cw.elevation_int16(elev)]


def test_two_runs_are_bit_identical(cw, golden):
    inputs, a = _everything(cw, golden)
    _, b = _everything(cw, golden, inputs)
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)
    assert int(a[3]) == int((~np.isnan(golden("custom")["fill_in_scattered_nan"])).sum())


def test_enqueue_only_on_a_caller_stream_gives_the_synchronous_result(cw, golden):
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    inputs, ref = _everything(cw, golden)
    s = torch.cuda.Stream()
    with eng.on_stream(s, asynchronous=True):
        x = [t.clone() for t in inputs]                   # produced on the caller's stream, consumed there without a host sync
        got = [t.clone() for t in _everything(cw, golden, x)[1]]   # read on that stream after the calls
    torch.cuda.current_stream().synchronize()
    for a, b in zip(got, ref):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


def test_c_abi_argument_errors(cw):
    from terrain_diffusion_amd._lib import TdError
    from terrain_diffusion_amd.engine import get_engine
    st = C.c_void_p(get_engine("cuda").stream)
    l = cw.lib()
    dp = lambda t: C.c_void_p(t.data_ptr())
    xy = torch.tensor([[0.0, 0.0], [6.0, 0.0], [0.0, 6.0]], dtype=torch.float64, device="cuda")
    off, val = torch.tensor([0, 3], dtype=torch.int32, device="cuda"), torch.ones(1, device="cuda")
    plane, out = torch.zeros(8, 8, device="cuda"), torch.empty(8, 8, device="cuda")
    idx, cnt = torch.empty(8, 8, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    q = torch.empty(64, dtype=torch.int16, device="cuda")
    host, hostd, hosti = torch.zeros(8, 8), torch.zeros(3, 2, dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
    big = 16385
    bad = [
        lambda: l.td_custom_rasterize(st, dp(xy), 3, dp(off), dp(val), 1, 0, 8, 0.0, dp(out), 1),
        lambda: l.td_custom_rasterize(st, dp(xy), 3, dp(off), dp(val), 1, 8, big, 0.0, dp(out), 1),
        lambda: l.td_custom_rasterize(st, dp(xy), 3, dp(off), dp(val), 1, big, 8, 0.0, dp(out), 1),
        lambda: l.td_custom_rasterize(st, dp(xy), 3, dp(off), dp(val), -1, 8, 8, 0.0, dp(out), 1),
        lambda: l.td_custom_rasterize(st, dp(xy), -3, dp(off), dp(val), 1, 8, 8, 0.0, dp(out), 1),
        lambda: l.td_custom_rasterize(st, dp(xy), 3, dp(off), dp(val), 1, 8, 8, 0.0, None, 1),
        lambda: l.td_custom_rasterize(st, None, 3, dp(off), dp(val), 1, 8, 8, 0.0, dp(out), 1),
        lambda: l.td_custom_rasterize(st, dp(xy), 3, None, dp(val), 1, 8, 8, 0.0, dp(out), 1),
        lambda: l.td_custom_rasterize(st, dp(xy), 3, dp(off), None, 1, 8, 8, 0.0, dp(out), 1),
        lambda: l.td_custom_rasterize(st, dp(hostd), 3, dp(off), dp(val), 1, 8, 8, 0.0, dp(out), 1),
        lambda: l.td_custom_rasterize(st, dp(xy), 3, dp(hosti), dp(val), 1, 8, 8, 0.0, dp(out), 1),
        lambda: l.td_custom_rasterize(st, dp(xy), 3, dp(off), dp(val), 1, 8, 8, 0.0, dp(host), 1),
        lambda: l.td_custom_rasterize(st, C.c_void_p(xy.data_ptr() + 8), 2, dp(off), dp(val), 1, 8, 8, 0.0, dp(out), 1),
        lambda: l.td_custom_fill_nearest(st, dp(plane), 0, 8, 0.0, dp(out), None, dp(cnt), 1),
        lambda: l.td_custom_fill_nearest(st, dp(plane), 8, big, 0.0, dp(out), None, dp(cnt), 1),
        lambda: l.td_custom_fill_nearest(st, dp(plane), big, 8, 0.0, dp(out), None, dp(cnt), 1),
        lambda: l.td_custom_fill_nearest(st, None, 8, 8, 0.0, dp(out), None, dp(cnt), 1),
        lambda: l.td_custom_fill_nearest(st, dp(plane), 8, 8, 0.0, None, None, dp(cnt), 1),
        lambda: l.td_custom_fill_nearest(st, dp(plane), 8, 8, 0.0, dp(out), None, None, 1),
        lambda: l.td_custom_fill_nearest(st, dp(host), 8, 8, 0.0, dp(out), None, dp(cnt), 1),
        lambda: l.td_custom_fill_nearest(st, dp(plane), 8, 8, 0.0, dp(host), None, dp(cnt), 1),
        lambda: l.td_custom_fill_nearest(st, dp(plane), 8, 8, 0.0, dp(out), dp(hosti), dp(cnt), 1),
        lambda: l.td_custom_fill_nearest(st, dp(plane), 8, 8, 0.0, dp(out), dp(idx), dp(hosti), 1),
        lambda: l.td_custom_fill_nearest(st, dp(plane), 8, 8, 0.0, dp(plane), None, dp(cnt), 1),
        lambda: l.td_custom_fill_nearest(st, dp(plane), 4, 8, 0.0, C.c_void_p(plane.data_ptr() + 64), None, dp(cnt), 1),
        lambda: l.td_custom_elev_int16(st, dp(plane), -1, dp(q), 1),
        lambda: l.td_custom_elev_int16(st, dp(plane), (1 << 30) + 1, dp(q), 1),
        lambda: l.td_custom_elev_int16(st, None, 64, dp(q), 1),
        lambda: l.td_custom_elev_int16(st, dp(plane), 64, None, 1),
        lambda: l.td_custom_elev_int16(st, dp(host), 64, dp(q), 1),
        lambda: l.td_custom_elev_int16(st, dp(plane), 64, dp(host), 1),
        lambda: l.td_custom_elev_int16(st, dp(plane), 8, C.c_void_p(q.data_ptr() + 1), 1),
    ]
    for k, fn in enumerate(bad):
        with pytest.raises(TdError):
            cw.check(fn())
        assert l.td_custom_last_error().decode().startswith("td_custom_"), k
    # what is allowed: no polygon without arrays, nothing to convert without buffers; offsets outside xy burn nothing
    cw.check(l.td_custom_rasterize(st, None, 0, None, None, 0, 8, 8, 7.0, dp(out), 1))
    assert bool((out == 7.0).all())
    cw.check(l.td_custom_elev_int16(st, None, 0, None, 1))
    for o in ([0, 4], [-1, 3], [3, 0]):
        cw.check(l.td_custom_rasterize(st, dp(xy), 3, dp(torch.tensor(o, dtype=torch.int32, device="cuda")), dp(val), 1, 8, 8, 7.0, dp(out), 1))
        assert bool((out == 7.0).all()), o


# ------------------------------------------------------------------------------------------------------------------------------ drop-ins and round trips
def test_azgaar_layers_and_rasterize_layer_against_the_twin(cw):
    m = twin.synthetic_azgaar_map()
    layers, geo = cw.azgaar_layers(m)
    want, (out_h, out_w) = twin.azgaar_layers(m, cw.BIOME_VARIABILITY)
    assert (geo["out_h"], geo["out_w"]) == (out_h, out_w) == (78, 144) and list(layers) == list(cw.LAYERS)
    for name in cw.LAYERS:
        assert layers[name].dtype == F and layers[name].shape == (78, 144) and np.array_equal(bits(layers[name]), bits(want[name])), name
        assert np.isfinite(layers[name]).all() and not (layers[name] == F(-9999.0)).any()
    assert layers["heightmap"].min() < 0 < layers["heightmap"].max() and len(np.unique(layers["temperature_std"])) > 5
    # the same through a file, with another scale and ocean curve
    import json
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".json") as f:
        json.dump(m, f)
        f.flush()
        layers2, geo2 = cw.azgaar_layers(f.name, scale=250.0, ocean_max_depth=6000.0, ocean_power=1.0)
    want2, shape2 = twin.azgaar_layers(m, cw.BIOME_VARIABILITY, 250.0, 6000.0, 1.0)
    assert (geo2["out_h"], geo2["out_w"]) == shape2 and all(np.array_equal(bits(layers2[k]), bits(want2[k])) for k in cw.LAYERS)
    # rasterize_layer, the reference's signature
    gv = {v["i"]: v["p"] for v in m["grid"]["vertices"]}
    fn = lambda c: float(c["temp"]) if "temp" in c else None
    got = cw.rasterize_layer(m["grid"]["cells"], gv, geo["scale_x"], geo["scale_y"], (78, 144), fn, "float32", -9999.0)
    assert isinstance(got, np.ndarray) and got.dtype == F and (got == F(-9999.0)).any()
    assert np.array_equal(bits(got), bits(twin.rasterize(*twin._csr(m["grid"]["cells"], gv, geo["scale_x"], geo["scale_y"], fn), (78, 144), -9999.0)))


def stub_elevation(i1, j1, i2, j2):
    """Metres from the absolute pixel only (so that every chunking reads the same world): beyond the int16 range on both sides, fractions on
    both sides of zero, a NaN in every 256 x 256 cell."""
    ii, jj = np.meshgrid(np.arange(i1, i2, dtype=np.float64), np.arange(j1, j2, dtype=np.float64), indexing="ij")
    e = 36000.0 * np.sin(ii / 97.0) * np.cos(jj / 131.0) + 0.37 * np.sin(ii * 0.7 + jj * 0.3)
    e = e.astype(F)
    e[(ii % 256 == 3) & (jj % 256 == 5)] = np.nan
    return e


class StubWorld:
    def __init__(self):
        self.boxes = []

    def get(self, i1, j1, i2, j2, with_climate=True):
        assert with_climate is False
        self.boxes.append((i1, j1, i2, j2))
        return {"elev": torch.from_numpy(stub_elevation(i1, j1, i2, j2)).cuda(), "climate": None}


def test_export_elevation_on_a_stub_world_is_the_twins_loop(cw):
    world = StubWorld()
    got = cw.export_elevation(world, 3, 2, chunk_size=512)
    assert isinstance(got, np.ndarray) and got.dtype == np.int16 and got.shape == (768, 512)
    assert world.boxes == [(16384, 16384, 16896, 16896), (16896, 16384, 17152, 16896)] == [b for _, _, b in twin.export_boxes(3, 2, 512)]
    assert np.array_equal(got, twin.export_elevation(stub_elevation, 3, 2, 512))
    assert got.min() == -32768 and got.max() == 32767 and got[3, 5] == 0
    world = StubWorld()
    assert np.array_equal(cw.export_elevation(world, 3, 2, chunk_size=256), got) and len(world.boxes) == 6


@pytest.fixture(scope="module")
def models():
    import terrain_diffusion_amd as td
    from oracle.unet import COARSE_CONFIG, DECODER_CONFIG, synth_state_dict, tiny_config
    bcfg = tiny_config(64, 1)
    ms = [td.EDMUnet2D(**c, dtype="fp32").load_state_dict(synth_state_dict(c, seed=s)) for c, s in ((COARSE_CONFIG, 1), (bcfg, 2), (DECODER_CONFIG, 3))]
    yield ms
    for m in ms:
        m.close()


def test_import_and_export_on_a_world_pipeline(cw, models):
    """azgaar_layers -> import_conditioning -> export_elevation for a map of one conditioning cell, with the tiny synthetic models."""
    import terrain_diffusion_amd as td
    m = twin.synthetic_azgaar_map(n_grid=40, n_pack=30, lat=(10.0, 10.9), lon=(20.0, 20.9))
    layers, geo = cw.azgaar_layers(m)
    assert (geo["out_h"], geo["out_w"]) == (1, 1)
    make = lambda: td.WorldPipeline.from_models(*models, seed=4242, decoder_tile_size=64, decoder_tile_stride=48, latents_batch_size=16).bind()
    w = make()
    try:
        plain = cw.export_elevation(w, 1, 1)
    finally:
        w.close()
    w = make()
    try:
        assert cw.import_conditioning(w, layers) == (1, 1)
        assert sorted(w.custom_conditioning_imports) == [0, 1, 2, 3, 4] and w.custom_conditioning_imports[0].shape == (129, 129)
        assert w.custom_conditioning_import_origins[2] == (0, 0) and w.custom_conditioning_default_values == {0: -1000.0}
        assert np.array_equal(w.custom_conditioning_imports[2], np.full((129, 129), layers["temperature_std"][0, 0] * F(100.0), F))
        got = cw.export_elevation(w, 1, 1)
        (_, _, box), = cw.export_boxes(1, 1)
        elev = w.get(*box, with_climate=False)["elev"]          # what the export converted: served again from the world's tiles
        assert bool(torch.isfinite(elev).all()) and np.array_equal(got, twin.elev_int16(elev.cpu().numpy()))
    finally:
        w.close()
    assert got.dtype == np.int16 and got.shape == (256, 256) and plain.shape == (256, 256)
    assert got.min() < got.max() and not np.array_equal(got, plain)
