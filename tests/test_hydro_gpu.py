"""Hydrology on the GPU (libtd_hydro.so, hydro_csrc/hydro_kernels.hip): every case recorded from the reference's own postprocessing.py
(tests/golden/hydro.npz) through the drop-ins, 1024^2 to 4096^2 canvases against the NumPy twin (tests/_hydro_twin.py), tile indexing by
translation, determinism, host vs device input, the enqueue-only stream mode, refusals, and a fill -> indicator of WorldPipeline output."""
import json

import numpy as np
import pytest
import torch

import _hydro_twin as twin
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available()
    return t


def _ulps(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0


def test_every_recorded_case_through_the_drop_ins(td, golden):
    g = golden("hydro")
    cases = json.loads(str(g["cases"]))
    assert len(cases) == 39
    for c in cases:
        name, z, kw = c["name"], g[c["input"]], c["kwargs"]
        if c["fn"] == "fill":
            got = td.fill_depressions_priority_flood(z, **kw)
            assert got.dtype == np.float32 and np.array_equal(got, g["out_" + name], equal_nan=True), name
            inp = z.copy()
            back = td.fill_depressions_priority_flood(inp, in_place=True, **kw)
            assert back is inp and np.array_equal(inp, got, equal_nan=True), name
        elif c["fn"] == "d8":
            rr, cc, sink, kmax = td.d8_flow(z, **kw)
            assert rr.dtype == cc.dtype == kmax.dtype == np.int64 and sink.dtype == np.bool_, name
            assert np.array_equal(rr * z.shape[1] + cc, g["receiver_" + name]), name
            assert np.array_equal(kmax, g["kmax_" + name]) and np.array_equal(sink, g["sink_" + name]), name
        elif c["fn"] == "acc":
            rr, cc, sink, _ = td.d8_flow(z)
            got = td.flow_accumulation(z, rr, cc, sink)
            assert got.dtype == np.float32 and np.array_equal(got, g["out_" + name]), name
        else:
            got = td.plot_flow_indicator(z, **kw)
            want = g["out_" + name]
            assert got.dtype == np.float32 and got.shape == want.shape, name
            assert _ulps(got, want) <= 1, (name, _ulps(got, want))


@pytest.mark.parametrize("n,seed", [(1024, 71), (2048, 72), (4096, 73)])
def test_large_canvases_against_the_twin(td, n, seed):
    z = twin.rugged(n, n, seed)
    zd = torch.from_numpy(z).cuda()
    # d8, bit for bit
    receiver, kmax, sink = td.flow_directions(zd)
    r, k, s = twin.d8(z)
    assert np.array_equal(receiver.cpu().numpy(), r) and np.array_equal(kmax.cpu().numpy(), k) and np.array_equal(sink.cpu().numpy(), s)
    # accumulation: exact by the recurrence
    acc = td.flow_accumulation_map(zd, receiver, sink).cpu().numpy()
    assert twin.accumulation_ok(z, r, s, acc) and acc.max() > 1000
    # fill: the twin's relaxation up to 1024^2, the fixed-point equations above
    filled, passes = td.fill_depressions(zd, return_passes=True)
    filled = filled.cpu().numpy()
    assert passes >= 2
    assert not np.isinf(filled[z > 0]).any()
    if n <= 1024:
        want, _ = twin.fill(z)
        assert np.array_equal(filled, want, equal_nan=True)
    assert twin.fill_fixed_point_violations(z, filled) == 0
    # the filled canvas drains: its d8 and accumulation as well
    rf, kf, sf = td.flow_directions(torch.from_numpy(filled).cuda())
    assert np.array_equal(rf.cpu().numpy(), twin.d8(filled)[0])
    accf = td.flow_accumulation_map(torch.from_numpy(filled).cuda(), rf, sf).cpu().numpy()
    assert twin.accumulation_ok(filled, rf.cpu().numpy(), sf.cpu().numpy(), accf)


def test_fill_variants_against_the_twin(td):
    z = twin.rugged(640, 900, 81)
    nodata = np.float32(321.25)
    z[300:310, 100:140] = nodata
    zd = torch.from_numpy(z).cuda()
    for kw in (dict(connectivity=4), dict(epsilon=0.0), dict(epsilon=0.01), dict(nodata=float(nodata))):
        got = td.fill_depressions(zd, **kw).cpu().numpy()
        want, _ = twin.fill(z, **kw)
        assert np.array_equal(got, want, equal_nan=True), kw


def test_d8_of_a_crop_is_the_crop_of_d8_one_pixel_inside(td):
    z = twin.rugged(1500, 1700, 91)
    zd = torch.from_numpy(z).cuda()
    W = z.shape[1]
    rec, km, sk = (t.cpu().numpy() for t in td.flow_directions(zd))
    y0, y1, x0, x1 = 131, 1377, 65, 1601
    rc, kc, sc = (t.cpu().numpy() for t in td.flow_directions(zd[y0:y1, x0:x1].contiguous()))
    wc = x1 - x0
    inner = (slice(y0 + 1, y1 - 1), slice(x0 + 1, x1 - 1))
    full = rec[inner]
    as_crop = (full // W - y0) * wc + (full % W - x0)
    assert np.array_equal(as_crop, rc[1:-1, 1:-1]) and np.array_equal(km[inner], kc[1:-1, 1:-1]) and np.array_equal(sk[inner], sc[1:-1, 1:-1])


def test_two_runs_and_host_vs_device_input_are_bit_identical(td):
    z = twin.rugged(700, 900, 101)
    zd = torch.from_numpy(z).cuda()
    a = [td.fill_depressions_priority_flood(z) for _ in range(2)] + [td.fill_depressions_priority_flood(zd)]
    assert all(np.array_equal(a[0], x, equal_nan=True) for x in a[1:])
    b = [td.plot_flow_indicator(z, 2) for _ in range(2)] + [td.plot_flow_indicator(zd, 2)]
    assert all(np.array_equal(b[0], x) for x in b[1:])
    d = [td.d8_flow(z), td.d8_flow(zd)]
    assert all(np.array_equal(p, q) for p, q in zip(*d))


def test_enqueue_only_on_a_caller_stream_gives_the_synchronous_result(td):
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    z = torch.from_numpy(twin.rugged(1024, 1024, 111)).cuda()
    ref_f = td.fill_depressions(z)
    ref_r, ref_k, ref_s = td.flow_directions(ref_f)
    ref_a = td.flow_accumulation_map(ref_f, ref_r, ref_s)
    ref_i = td.flow_indicator(ref_f, 3)
    s = torch.cuda.Stream()
    with eng.on_stream(s, asynchronous=True):
        x = z * 1.0                                        # produced on the caller's stream, consumed there without a host sync
        f = td.fill_depressions(x, engine=eng)
        r, k, sk = td.flow_directions(f, engine=eng)
        a = td.flow_accumulation_map(f, r, sk, engine=eng)
        i = td.flow_indicator(f, 3, engine=eng)
        got = [t.clone() for t in (f, r, k, sk, a, i)]
    torch.cuda.current_stream().synchronize()
    for p, q in zip(got, (ref_f, ref_r, ref_k, ref_s, ref_a, ref_i)):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)) if p.dtype == torch.float32 else torch.equal(p, q)   # NaN holes: bitwise


def test_bad_arguments_and_an_uphill_receiver_are_refused(td):
    import ctypes as C
    from terrain_diffusion_amd._lib import TdError
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.hydrology import check, lib
    z = twin.rugged(64, 80, 121)
    rr, cc, sink, _ = td.d8_flow(z)
    # an uphill edge: the lowest land cell that is not a sink sends its water to the highest land cell
    land = np.argwhere((z > 0) & ~sink)
    lo = land[np.argmin(z[tuple(land.T)])]
    hi = np.unravel_index(np.nanargmax(z), z.shape)
    rr2, cc2 = rr.copy(), cc.copy()
    rr2[tuple(lo)], cc2[tuple(lo)] = hi
    with pytest.raises(ValueError, match="not strictly downhill"):
        td.flow_accumulation(z, rr2, cc2, sink)
    rr2[tuple(lo)], cc2[tuple(lo)] = lo                   # a level edge (to itself)
    with pytest.raises(ValueError, match="not strictly downhill"):
        td.flow_accumulation(z, rr2, cc2, sink)
    rr2[0, 0] = 64
    with pytest.raises(IndexError):
        td.flow_accumulation(z, rr2, cc, sink)
    with pytest.raises(ValueError):
        td.flow_accumulation(z, rr[:, :-1], cc[:, :-1], sink[:, :-1])
    with pytest.raises(NotImplementedError):
        td.fill_depressions_priority_flood(z, max_raise=50.0)
    eng = get_engine("cuda")
    st = C.c_void_p(eng.stream)
    e = torch.from_numpy(z).cuda()
    dp = lambda t: C.c_void_p(t.data_ptr())
    i32 = torch.empty(64, 80, dtype=torch.int32, device="cuda")
    u8 = torch.empty(64, 80, dtype=torch.uint8, device="cuda")
    f32 = torch.empty(64, 80, device="cuda")
    for H, W, src in ((0, 80, e), (64, 0, e), ((1 << 20) + 1, 1, e), (64, 80, e.cpu())):
        with pytest.raises(TdError):
            check(lib().td_hydro_d8(st, dp(src), H, W, 1e-3, dp(i32), dp(u8), dp(u8), 1))
        with pytest.raises(TdError):
            check(lib().td_hydro_fill(st, dp(src), H, W, 1e-3, 8, 0, 0.0, dp(f32), None))
    with pytest.raises(TdError):   # accumulation beyond 2^24 cells
        check(lib().td_hydro_accumulate(st, dp(e), 4097, 4096, dp(i32), dp(u8), dp(f32), dp(i32), 1))
    with pytest.raises(TdError):
        check(lib().td_hydro_indicator(st, dp(f32), 64, 80, 65, dp(f32), 1))
    with pytest.raises(TdError):
        check(lib().td_hydro_fill(st, dp(e), 64, 80, -1e-3, 8, 0, 0.0, dp(f32), None))
    with pytest.raises(TdError):
        check(lib().td_hydro_fill(st, dp(e), 64, 80, 1e-3, 8, 0, 0.0, dp(e), None))


@pytest.fixture(scope="module")
def models(td):
    from oracle.unet import COARSE_CONFIG, DECODER_CONFIG, synth_state_dict, tiny_config
    bcfg = tiny_config(64, 1)
    ms = [td.EDMUnet2D(**c, dtype="fp32").load_state_dict(synth_state_dict(c, seed=s)) for c, s in ((COARSE_CONFIG, 1), (bcfg, 2), (DECODER_CONFIG, 3))]
    yield ms
    for m in ms:
        m.close()


def test_fill_then_indicator_of_world_pipeline_output(td, models):
    w = td.WorldPipeline.from_models(*models, seed=4242, decoder_tile_size=64, decoder_tile_stride=48, latents_batch_size=16).bind()
    try:
        elev = w.get(-21, 13, 75, 141, with_climate=False)["elev"]
        assert elev.dtype == torch.float32
        filled = td.fill_depressions(elev)
        ind = td.flow_indicator(filled, 2)
        host = elev.cpu().numpy()
        want_f, _ = twin.fill(host)
        assert np.array_equal(filled.cpu().numpy(), want_f, equal_nan=True)
        r, _, s = twin.d8(want_f)
        want_i = twin.indicator(twin.accumulate(want_f, r, s), 2)
        got = ind.cpu().numpy()
        assert got.shape == (48, 64) and _ulps(got, want_i) <= 1
        assert np.array_equal(td.plot_flow_indicator(td.fill_depressions_priority_flood(elev), 2), got)
    finally:
        w.close()
