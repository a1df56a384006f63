"""The custom-map import without a GPU: the NumPy twin (tests/_custom_twin.py) against what was recorded from the reference
(tests/golden/custom.npz: fill_nodata, h_to_meters, the two tables) and against a reference-free statement of the rasteriser's partition (the
nearest site of a Voronoi diagram); the module's host halves (h_to_meters, the biome table, load_and_pad, the output geometry, the export's
boxes) against the twin and hand-made cases; the header against the binding; and the argument checks, which refuse before an engine exists."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _custom_twin as twin
from terrain_diffusion_amd import custom_world as cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def fill_cases(g):
    for c in json.loads(str(g["cases"])):
        yield c["name"], g["fill_in_" + c["name"]], (np.nan if c["nodata"] is None else c["nodata"]), g["fill_out_" + c["out"]]


def test_the_twins_fill_equals_every_recorded_fill_nodata_output(golden):
    """Exact: a disagreement on a tie would mean the (column, row) tie rule of include/td_custom.h is wrong."""
    g = golden("custom")
    names = []
    for name, a, nodata, want in fill_cases(g):
        got = twin.fill_nearest(a, nodata)
        assert got.dtype == F and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, int((got != want).sum()))
        names.append(name)
    assert names == ["scattered_nan", "scattered_sentinel", "s7x5", "s1x9", "s33x1", "lines", "single", "no_hole"]
    # the fixtures do hold ties, and the other order (row first) would fail them
    a = g["fill_in_scattered_nan"]
    H, W = a.shape
    bad = np.isnan(a)
    vr, vc = np.nonzero(~bad)
    hr, hc = np.nonzero(bad)
    d = (hr[:, None] - vr[None]) ** 2 + (hc[:, None] - vc[None]) ** 2
    tied = (d == d.min(1, keepdims=True)).sum(1) > 1
    assert tied.mean() > 0.3
    row_first = a[vr[d.argmin(1)], vc[d.argmin(1)]]          # np.nonzero lists row-major: the first minimum is the smallest row
    assert (row_first != g["fill_out_scattered_nan"][bad]).sum() > 100


@pytest.mark.parametrize("n_sites,shape", [(400, (96, 160)), (5000, (97, 131))])
def test_the_twins_rasteriser_partitions_a_voronoi_diagram_by_nearest_site(n_sites, shape):
    """The all_touched=False partition, stated without a reference: on the cells of a Voronoi diagram every pixel belongs to the cell of the
    site nearest to its centre, and to that cell only."""
    H, W = shape
    sites, vertices, rings = twin.voronoi_cells(n_sites, W, H, seed=n_sites)
    xy, offsets = twin.csr_of(vertices, rings)
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    nearest = ((px[..., None] - sites[:, 0]) ** 2 + (py[..., None] - sites[:, 1]) ** 2).argmin(-1)
    own = twin.owners(xy, offsets, shape)
    assert np.array_equal(own, nearest)
    covered = np.zeros(shape, np.int32)
    for p in range(n_sites):
        covered += twin.owners(xy[offsets[p]:offsets[p + 1]], [0, offsets[p + 1] - offsets[p]], shape) >= 0
    assert covered.min() == 1 and covered.max() == 1
    values = np.arange(n_sites, dtype=F) * F(0.5) - F(7)
    assert np.array_equal(twin.rasterize(xy, offsets, values, shape, np.nan), values[nearest])


def test_h_to_meters_and_the_tables_equal_the_recorded_ones(golden):
    g = golden("custom")
    for row, want in zip(g["h_in"], g["h_out"]):
        h = int(row[0]) if row[0] == int(row[0]) else float(row[0])
        for fn in (cw.h_to_meters, twin.h_to_meters):
            got = fn(h, *row[1:])
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (row, got, want)
    table = np.array(cw.BIOME_VARIABILITY, np.float64)
    assert table.shape == (13, 2) and table.tobytes() == g["biome_variability"].tobytes()
    assert [n.replace(".tif", "") for n in g["channel_names"].tolist()] == list(cw.LAYERS) == list(twin.LAYERS)
    for name, ch, scale, default in zip(cw.LAYERS, g["channel_index"], g["channel_scale"], g["channel_default"]):
        assert cw.CHANNELS[name] == (int(ch), float(scale), None if np.isnan(default) else float(default))
    assert json.loads(str(g["constants"])) == {"PADDING": cw.PADDING, "PIXELS_PER_CELL": cw.PIXELS_PER_CELL}
    assert (twin.PADDING, twin.PIXELS_PER_CELL) == (cw.PADDING, cw.PIXELS_PER_CELL)


def test_load_and_pad_on_hand_made_cases():
    a = np.array([[1.0, -9999.0, 3.0], [np.inf, -np.inf, np.nan]], np.float64)
    want = np.array([[1.0, -1000.0, 3.0], [-1000.0, -1000.0, -1000.0]], F)
    got = cw.load_and_pad(a, -9999.0, 1.0, -1000.0, padding=2)
    assert got.dtype == F and got.shape == (6, 7)
    assert np.array_equal(got[2:4, 2:5], want)
    assert np.array_equal(got, np.pad(want, 2, mode="edge"))
    assert np.array_equal(got[:2, :2], np.full((2, 2), 1.0, F)) and np.array_equal(got[4:, 5:], np.full((2, 2), -1000.0, F))
    # no default: non-finite -> 0; scale 100 in float32; the sentinel is only a sentinel when it is passed
    got = cw.load_and_pad(a, None, 100.0, None, padding=1)
    assert np.array_equal(got[1:3, 1:4], np.array([[100.0, -999900.0, 300.0], [0.0, 0.0, 0.0]], F))
    b = np.array([[0.1, 0.7]], F)
    assert np.array_equal(cw.load_and_pad(b, None, 100.0, None, padding=0), b * F(100.0))
    assert cw.load_and_pad(np.zeros((2, 3)), None, 1.0, None).shape == (2 + 128, 3 + 128)
    rng = np.random.default_rng(1)
    c = rng.standard_normal((5, 4)).astype(F)
    c[1, 2], c[3, 0] = np.nan, -9999.0
    for nodata, scale, default in ((None, 1.0, None), (-9999.0, 100.0, None), (-9999.0, 1.0, -1000.0)):
        assert np.array_equal(cw.load_and_pad(c, nodata, scale, default), twin.load_and_pad(c, nodata, scale, default))


def test_output_geometry_rounds_as_python_does():
    # exact halves: 1 degree of latitude in pixels of 222.64 km is 0.5 pixel, round(0.5) = 0 -> max(1, 0) = 1; in pixels of 44.528 km it is
    # 2.5 pixels, and Python rounds the half to the even 2 (np.round-half-up would give 3); 7 degrees are 17.5 -> 18
    for dlat, scale, pixels, want in ((1.0, 222.64, 0.5, 1), (1.0, 44.528, 2.5, 2), (7.0, 44.528, 17.5, 18)):
        assert dlat * 111.32 / scale == pixels
        geo = cw.output_geometry({"latN": dlat / 2, "latS": -dlat / 2, "lonW": 0.0, "lonE": 3.0}, 100.0, 50.0, scale=scale)
        assert geo["out_h"] == want and (geo["out_h"], geo["out_w"]) == twin.output_shape({"latN": dlat / 2, "latS": -dlat / 2, "lonW": 0.0, "lonE": 3.0}, scale)
        assert geo["scale_x"] == geo["out_w"] / 100.0 and geo["scale_y"] == want / 50.0
        assert geo["pixel_lon"] == 3.0 / geo["out_w"] and geo["pixel_lat"] == dlat / want
    m = twin.synthetic_azgaar_map()
    geo = cw.output_geometry(m["mapCoordinates"], m["info"]["width"], m["info"]["height"], 100.0)
    assert (geo["out_h"], geo["out_w"]) == twin.output_shape(m["mapCoordinates"], 100.0) == (78, 144)


def test_cells_csr_skips_what_the_reference_skips():
    verts = {0: [0, 0], 1: [4, 0], 2: [4, 4], 3: [0, 4]}
    cells = [{"v": [0, 1, 2], "x": 1.5}, {"v": [0, 1, 9], "x": 2.0}, {"v": [1, 2, 3], "x": float("nan")}, {"v": [0, 2, 3]}, {"v": [3, 2, 1, 0], "x": 7}]
    xy, offsets, values = cw.cells_csr(cells, verts, 0.5, 2.0, lambda c: c.get("x"))
    assert offsets.tolist() == [0, 3, 7] and values.tolist() == [1.5, 7.0] and xy.dtype == np.float64 and offsets.dtype == np.int32
    assert xy.tolist() == [[0, 0], [2, 0], [2, 8], [0, 8], [2, 8], [2, 0], [0, 0]]
    exy, eoff, evals = cw.cells_csr([], verts, 1.0, 1.0, lambda c: 1.0)
    assert exy.shape == (0, 2) and eoff.tolist() == [0] and evals.shape == (0,)


def test_export_boxes_are_the_references():
    assert cw.export_boxes(3, 2, 512) == [(0, 0, (16384, 16384, 16896, 16896)), (512, 0, (16896, 16384, 17152, 16896))]
    for H, W, chunk in ((3, 2, 512), (1, 1, 2048), (5, 7, 768), (9, 17, 2048)):
        assert [(r, c, b) for r, c, b in cw.export_boxes(H, W, chunk)] == [(ci * 256, cj * 256, b) for ci, cj, b in twin.export_boxes(H, W, chunk)]


def test_header_entry_points_and_exports():
    import terrain_diffusion_amd as td
    text = open(os.path.join(ROOT, "include", "td_custom.h")).read()
    declared = set(re.findall(r"\b(td_custom_\w+)\s*\(", text))
    stated = {"td_custom_last_error", "td_custom_rasterize", "td_custom_fill_nearest", "td_custom_elev_int16"}
    assert declared == set(cw.EXPORTS) == stated
    assert re.search(r"#define TD_CUSTOM_MAX_SIDE 16384\b", text) and cw.MAX_SIDE == 16384
    assert re.search(r"#define TD_CUSTOM_MAX_ELEMENTS \(1 << 30\)", text) and cw.MAX_ELEMENTS == 1 << 30
    have = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", cw.LIB_PATH], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert stated <= have and not {n for n in have if n.startswith("td_") and n not in stated}
    cw.lib()     # binds every entry point
    for name in ("rasterize_cells", "fill_nearest", "elevation_int16", "h_to_meters", "fill_nodata", "rasterize_layer", "azgaar_layers",
                 "load_and_pad", "import_conditioning", "export_elevation"):
        assert getattr(td, name) is getattr(cw, name), name
    for phrase in ("all_touched=False", "not compared with GDAL", "REFUSED"):
        assert phrase in text and phrase in cw.__doc__, phrase


def test_argument_checks_refuse_before_any_engine_is_touched(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(cw, "_engine_for", no_engine)

    class World:
        def get(self, *a, **k):
            raise AssertionError("the world was read")
        set_custom_conditioning_import = get
    for chunk in (500, 0, -256, 257):
        with pytest.raises(ValueError, match="multiple of 256"):
            cw.export_elevation(World(), 2, 2, chunk_size=chunk)
    with pytest.raises(ValueError, match="empty map"):
        cw.export_elevation(World(), 0, 2)
    with pytest.raises(ValueError, match="no layer"):
        cw.import_conditioning(World(), {})
    with pytest.raises(ValueError, match="no layer"):
        cw.import_conditioning(World(), {"elevation": np.zeros((2, 2))})
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        cw.import_conditioning(World(), {"temperature": np.zeros(4)})
    with pytest.raises(ValueError, match="one shape"):
        cw.import_conditioning(World(), {"heightmap": np.zeros((3, 4)), "precipitation": np.zeros((4, 3))})
    for bad in (np.zeros(5, F), np.zeros((2, 3, 4), F)):
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            cw.fill_nearest(bad)
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            cw.fill_nodata(bad, -9999.0)
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            cw.load_and_pad(bad, None, 1.0, None)
    with pytest.raises(ValueError, match="limit"):
        cw.fill_nearest(np.zeros((1, 16385), F))
    for dtype in ("float64", "uint8", np.int16, "no such type"):
        with pytest.raises(ValueError, match="float32"):
            cw.rasterize_layer([], {}, 1.0, 1.0, (4, 4), lambda c: 1.0, dtype, 0.0)
    tri = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 2.0]])
    for xy, offsets, values, shape in ((tri, [0, 3], [1.0], (4,)), (tri, [0, 3], [1.0], (0, 4)), (tri, [0, 3], [1.0], (4, 16385)),
                                       (tri.reshape(-1), [0, 3], [1.0], (4, 4)), (tri, [0, 3], [1.0, 2.0], (4, 4)), (tri, [[0, 3]], [1.0], (4, 4)),
                                       (tri, [0, 4], [1.0], (4, 4)), (tri, [0, 3, 2], [1.0, 2.0], (4, 4)), (tri, [-1, 3], [1.0], (4, 4))):
        with pytest.raises(ValueError):
            cw.rasterize_cells(xy, offsets, values, shape, 0.0)
    # nothing invalid: the drop-in hands the input back, as the reference does, and needs no GPU for it
    a = np.ones((3, 3), F)
    assert cw.fill_nodata(a, -9999.0) is a and cw.fill_nodata(a, float("nan")) is a
