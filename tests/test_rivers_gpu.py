"""River maps on the GPU (include/td_rivers.h, libtd_rivers.so): every case recorded from the reference's get_relief_map with overlays and its
smooth_river_bumps (tests/golden/rivers.npz), the overlay-free render against libtd_relief.so bit for bit (the proof that the two libraries
share their arithmetic), one larger canvas against the NumPy twin (tests/_rivers_twin.py), the wrap of the smoothing stencil, determinism,
host vs device input, the enqueue-only stream mode, the device-resident chain against its pieces, and the C-ABI's refusals."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _rivers_twin as twin
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def rivers(td):
    from terrain_diffusion_amd import rivers as r
    return r


def _cases(golden, fn):
    g = golden("rivers")
    for c in json.loads(str(g["cases"])):
        if c["fn"] == fn:
            kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in c["kwargs"].items()}
            yield c, g[c["input"]], kw, g["out_" + c["name"]], {k: g[v] for k, v in c.get("overlays", {}).items()}


def test_every_recorded_relief_case_through_get_relief_map(rivers, golden):
    n = 0
    for c, elev, kw, want, ov in _cases(golden, "relief"):
        got = rivers.get_relief_map(elev, None, ov.get("biome"), ov.get("flow"), rgb=ov.get("rgb"), **kw)
        assert got.dtype == np.float32 and got.shape == want.shape, c["name"]
        msg = twin.compare(got, want)
        assert msg is None, (c["name"], msg)
        n += 1
    assert n == 17


@pytest.mark.parametrize("name", ["default", "params", "narrow_31x97", "tiny_2x9", "nan_pos_median", "nan_neg_median", "explicit_range"])
def test_without_overlays_the_picture_is_the_relief_librarys_bit_for_bit(td, rivers, golden, name):
    """160 x 224 crosses the 64-row and 128-column tiles; 31 x 97 and 2 x 9 fold the blur's reflection; NaN fills; an explicit range."""
    g = golden("relief")
    c = next(c for c in json.loads(str(g["cases"])) if c["name"] == name)
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in c["kwargs"].items()}
    e = g[c["input"]]
    want = td.get_relief_map(e, None, None, None, **kw)
    got = rivers.get_relief_map(e, None, None, None, **kw)
    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32))   # NaN payloads included
    dev = rivers.relief_overlay_map(torch.from_numpy(e).cuda(), **kw)
    assert torch.equal(dev.view(torch.int32), td.relief_map(torch.from_numpy(e).cuda(), **kw).view(torch.int32))


def test_every_recorded_smoothing_case(rivers, golden):
    """NaN positions identical and |gpu - D64| <= 4 e_ref + 1 ulp_fp32(max |h|): e_ref is the REFERENCE's own fp32 rounding error against the
    float64 formula (recorded with the case), so the yardstick is not the code under test.  4: the one operation that differs is exp (numpy's
    against the device's, each within an ulp), and the stencil amplifies such a difference as it amplifies the reference's own roundings.
    The bound must stay below 1e-3 of what the smoothing moves, so a kernel that does nothing cannot pass.  Printed with -s: the measured
    maximum and how many elements differ from the fp32 twin's bits (not bounded)."""
    n = 0
    for c, h, kw, want, _ in _cases(golden, "smooth"):
        name = c["name"]
        got = rivers.smooth_river_bumps(h, **kw)
        assert got.dtype == np.float32 and got.shape == h.shape, name
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        d64 = twin.smooth_d64(h, **kw)
        tol = 4 * c["e_ref"] + twin.ulp32(np.nanmax(np.abs(h)))
        err = float(np.nanmax(np.abs(got.astype(np.float64) - d64)))
        t32 = twin.smooth(h, **kw)
        off = int((got.view(np.uint32) != t32.view(np.uint32)).sum())
        print(f"{name:24s} max|gpu - D64| {err:.3e}  bound {tol:.3e}  e_ref {c['e_ref']:.3e}  off the fp32 twin's bits: {off} of {h.size}")
        assert err <= tol, (name, err, tol)
        if kw.get("iterations", 3) > 0:
            assert tol <= 1e-3 * float(np.nanmax(np.abs(want - h))), name
        else:
            assert np.array_equal(got.view(np.uint32), h.view(np.uint32)), name   # zero iterations is a copy
        n += 1
    assert n == 17


def _smooth_tol(h, **kw):
    """the recorded cases' bound for a seeded input: the fp32 twin (the reference's arithmetic, numpy's exp) stands for the reference"""
    d64 = twin.smooth_d64(h, **kw)
    e_ref = float(np.nanmax(np.abs(twin.smooth(h, **kw).astype(np.float64) - d64)))
    return d64, 4 * e_ref + twin.ulp32(np.nanmax(np.abs(h)))


def test_the_larger_canvas_against_the_twin(rivers):
    """1024 x 1536, once: the overlay picture (biome + integer flows, a NaN hole) and the smoothing (many blocks, NaN cells on the wrapped edges)."""
    H, W = 1024, 1536
    e = twin.land_and_sea(H, W, 61)
    e[100:140, 200:260] = np.nan
    rng = np.random.default_rng(62)
    flow = np.floor(rng.random((H, W), dtype=np.float32) ** 4 * 40).astype(np.float32)      # integers, about a fifth above 7
    flow[120, 210:230] = np.nan                                                              # a NaN flow draws nothing
    biome = np.kron(rng.integers(-2, 35, size=(H // 32, W // 32)), np.ones((32, 32), np.int64))
    pal = twin.palette(rivers.BIOME_PALETTE_U8)
    kw = dict(resolution=30, relief=0.8, flow_threshold=7)
    got = rivers.relief_overlay_map(torch.from_numpy(e).cuda(), biome=torch.from_numpy(biome).cuda(), flow=torch.from_numpy(flow).cuda(), **kw)
    msg = twin.compare(got.cpu().numpy(), twin.relief(e, pal=pal, biome=biome, flow=flow, **kw))
    assert msg is None, msg
    h = e.copy()
    h[0, 0] = h[H - 1, 700] = h[500, W - 1] = np.nan
    d64, tol = _smooth_tol(h)
    out = rivers.smooth_bumps(torch.from_numpy(h).cuda()).cpu().numpy()
    assert np.array_equal(np.isnan(out), np.isnan(h))
    assert np.nanmax(np.abs(out.astype(np.float64) - d64)) <= tol <= 1e-3 * np.nanmax(np.abs(d64 - h))


def test_the_smoothing_stencil_wraps_around_the_image(rivers):
    """np.roll: row 0's upper neighbour is row H - 1.  100 m added to the last row changes row 0 of the result, by what the twin says."""
    h = twin.land_and_sea(64, 80, 71)
    up = h.copy()
    up[-1] += np.float32(100.0)
    res = []
    for a in (h, up):
        d64, tol = _smooth_tol(a, iterations=1)
        got = rivers.smooth_river_bumps(a, iterations=1)
        assert np.abs(got.astype(np.float64) - d64).max() <= tol
        res.append((got, d64, tol))
    (a, a64, ta), (b, b64, tb) = res
    moved = np.abs(b64[0] - a64[0])
    assert moved.max() > 1.0                                                  # the twin: metres, not roundings
    assert np.abs((b[0].astype(np.float64) - a[0]) - (b64[0] - a64[0])).max() <= ta + tb
    assert np.array_equal(a[2:-3], b[2:-3])                                   # one iteration reaches one row


def test_biome_conversions(rivers, golden):
    """any integer dtype; a floating image truncates toward zero, NaN counts as 0; the drop-in ignores a biome of another shape"""
    c, e, kw, want, ov = next(x for x in _cases(golden, "relief") if x[0]["name"] == "biome_small")
    b = ov["biome"]
    ref = rivers.get_relief_map(e, None, b, None)
    for conv in (lambda a: a.astype(np.int64), lambda a: a.astype(np.int8), lambda a: torch.from_numpy(a.astype(np.int16)).cuda(),
                 lambda a: np.clip(a, 0, 255).astype(np.uint8), lambda a: torch.from_numpy(np.clip(a, 0, 255).astype(np.uint8)).cuda(),
                 lambda a: a.astype(np.float64) + np.where(a >= 0, 0.75, -0.75), lambda a: torch.from_numpy(a.astype(np.float32)).cuda() * 1.0):
        assert np.array_equal(rivers.get_relief_map(e, None, conv(b), None), ref, equal_nan=True)
    f = b.astype(np.float32)
    zero = b == 0
    f[zero] = np.nan
    assert zero.any() and np.array_equal(rivers.get_relief_map(e, None, f, None), ref, equal_nan=True)
    plain = rivers.get_relief_map(e, None, None, None)
    assert not np.array_equal(plain, ref, equal_nan=True)
    assert np.array_equal(rivers.get_relief_map(e, None, b[:, :-1], None), plain, equal_nan=True)
    rgb = np.random.default_rng(5).random(e.shape + (3,))                    # float64 colours are rounded to fp32 first
    out = rivers.get_relief_map(e, None, None, None, rgb=rgb)
    assert out.dtype == np.float32 and np.array_equal(out, rivers.get_relief_map(e, None, None, None, rgb=rgb.astype(np.float32)), equal_nan=True)


def _overlay_inputs(H, W, seed):
    e = twin.land_and_sea(H, W, seed)
    e[3:9, W // 2:W // 2 + 20] = np.nan
    rng = np.random.default_rng(seed + 1)
    flow = np.floor(rng.random((H, W), dtype=np.float32) ** 4 * 40).astype(np.float32)
    biome = rng.integers(-2, 35, size=(H, W)).astype(np.int32)
    rgb = rng.random((H, W, 3), dtype=np.float32)
    return e, dict(rgb=rgb, biome=biome, flow=flow)


def test_two_runs_and_host_vs_device_input_are_bit_identical(rivers):
    e, ov = _overlay_inputs(300, 420, 81)
    a = rivers.get_relief_map(e, None, ov["biome"], ov["flow"], rgb=ov["rgb"])
    b = rivers.get_relief_map(e, None, ov["biome"], ov["flow"], rgb=ov["rgb"])
    c = rivers.get_relief_map(torch.from_numpy(e).cuda(), None, torch.from_numpy(ov["biome"]).cuda(), torch.from_numpy(ov["flow"]).cuda(),
                              rgb=torch.from_numpy(ov["rgb"]).cuda())
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)
    s1, s2 = rivers.smooth_river_bumps(e), rivers.smooth_river_bumps(e)
    s3 = rivers.smooth_river_bumps(torch.from_numpy(e).cuda())
    assert np.array_equal(s1, s2, equal_nan=True) and np.array_equal(s1, s3, equal_nan=True)


def test_enqueue_only_on_a_caller_stream_gives_the_synchronous_result(rivers):
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    e, ov = _overlay_inputs(512, 640, 91)
    de = torch.from_numpy(e).cuda()
    dov = {k: torch.from_numpy(v).cuda() for k, v in ov.items()}
    ref = rivers.relief_overlay_map(de, **dov)
    ref_s = rivers.smooth_bumps(de, iterations=4)
    s = torch.cuda.Stream()
    with eng.on_stream(s, asynchronous=True):
        x = de * 1.0                                   # produced on the caller's stream, consumed there without a host sync
        f = dov["flow"] + 0.0
        got = rivers.relief_overlay_map(x, rgb=dov["rgb"], biome=dov["biome"], flow=f, engine=eng).clone()
        got_s = rivers.smooth_bumps(x, iterations=4, engine=eng).clone()
    torch.cuda.current_stream().synchronize()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)) and torch.equal(got_s.view(torch.int32), ref_s.view(torch.int32))


@pytest.mark.parametrize("smooth", [False, True])
def test_river_relief_map_is_the_chain_of_its_pieces(td, rivers, smooth):
    e = twin.land_and_sea(160, 224, 11)
    de = torch.from_numpy(e).cuda()
    biome = torch.from_numpy(np.random.default_rng(3).integers(0, 31, size=e.shape)).cuda()
    kw = dict(resolution=30, relief=0.7)
    got = rivers.river_relief_map(de, smooth=smooth, flow_threshold=5, biome=biome, **kw)
    routed = td.fill_depressions(de)
    if smooth:
        routed = rivers.smooth_bumps(routed)
    receiver, _, sink = td.flow_directions(routed)
    acc = td.flow_accumulation_map(routed, receiver, sink)
    want = rivers.relief_overlay_map(de, biome=biome, flow=acc, flow_threshold=5, **kw)
    assert (acc > 5).sum() > 100 and got.is_cuda and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got, rivers.relief_overlay_map(de, biome=biome, **kw))          # the rivers are drawn
    unfilled = rivers.river_relief_map(de, fill=False, smooth=smooth, flow_threshold=5, biome=biome, **kw)
    assert not torch.equal(unfilled, got)                                                  # pits cut the unfilled rivers short


def test_the_c_abi_refuses_bad_arguments(rivers):
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.relief import _device_tables
    eng = get_engine("cuda")
    st = C.c_void_p(eng.stream)
    e = torch.zeros(8, 8, device="cuda")
    out3, out1 = torch.empty(8, 8, 3, device="cuda"), torch.empty(8, 8, device="cuda")
    flow, biome, pal = torch.zeros(8, 8, device="cuda"), torch.zeros(8, 8, dtype=torch.int32, device="cuda"), rivers._device_palette(0)
    lut, wl, rl, ws, rs = _device_tables(0, 6.0, 1.2)
    he, hflow, hbiome, hpal, hout3, hout1 = e.cpu(), flow.cpu(), biome.cpu(), pal.cpu(), out3.cpu(), out1.cpu()   # host buffers, kept alive
    torch.cuda.synchronize()
    dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    lib = rivers.lib()

    def relief(H=8, W=8, src=e, r=rl, rgb=None, b=None, p=None, f=None, out=out3, lut_=lut):
        return lib.td_rivers_relief(st, dp(src), H, W, dp(lut_), dp(wl), r, dp(ws), rs, 315.0, 90.0, 1.0, 0, 0.0, 0.0, 0, 0.0, dp(rgb), dp(b), dp(p),
                                    dp(f), 7.0, dp(out), 1)

    def smooth(H=8, W=8, src=e, it=3, out=out1):
        return lib.td_rivers_smooth(st, dp(src), H, W, 50.0, 0.3, it, dp(out), 1)

    assert relief(f=flow, b=biome, p=pal) == 0 and smooth() == 0
    bad = [lambda: relief(H=1), lambda: relief(W=1), lambda: relief(r=65), lambda: relief(r=-1), lambda: relief(src=None), lambda: relief(out=None),
           lambda: relief(lut_=None), lambda: relief(src=he), lambda: relief(f=hflow), lambda: relief(rgb=hout3),
           lambda: relief(b=hbiome, p=pal), lambda: relief(b=biome, p=None), lambda: relief(b=biome, p=hpal), lambda: relief(out=hout3),
           lambda: smooth(H=1), lambda: smooth(W=1), lambda: smooth(it=65), lambda: smooth(it=-1), lambda: smooth(src=None), lambda: smooth(out=None),
           lambda: smooth(src=he), lambda: smooth(out=hout1), lambda: smooth(out=e), lambda: smooth(H=4, out=e[2:])]   # the last: a partial overlap
    for i, call in enumerate(bad):
        rc = call()
        assert rc < 0 and rivers._LIB.error_text(), i
    from terrain_diffusion_amd._lib import TdError
    with pytest.raises(TdError, match="iterations"):
        rivers.check(smooth(it=65))
    assert relief(f=flow, b=biome, p=pal) == 0 and smooth() == 0               # a refusal leaves the library usable
