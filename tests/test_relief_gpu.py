"""Shaded-relief rendering on the GPU (td_relief_map, relief_csrc/relief_kernels.hip): every case recorded from the reference's own get_relief_map
(tests/golden/relief.npz), larger seeded canvases against the NumPy twin (tests/_relief_twin.py), tile / halo indexing by translation,
determinism, host vs device input, the enqueue-only stream mode, and a render of WorldPipeline output."""
import json

import numpy as np
import pytest
import torch

import _relief_twin as twin
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available()
    return t


def _kw(c):
    return {k: (tuple(v) if isinstance(v, list) else v) for k, v in c["kwargs"].items()}


def test_every_recorded_case_through_get_relief_map(td, golden):
    g = golden("relief")
    cases = json.loads(str(g["cases"]))
    assert len(cases) == 11
    for c in cases:
        got = td.get_relief_map(g[c["input"]], None, None, None, **_kw(c))
        want = g["out_" + c["name"]]
        assert got.dtype == np.float32 and got.shape == want.shape, c["name"]
        msg = twin.compare(got, want)
        assert msg is None, (c["name"], msg)


@pytest.mark.parametrize("shape,seed,kw", [((1024, 1536), 21, {}),
                                           ((2048, 2048), 22, dict(resolution=30, relief=0.8, sigma_large=4.5, sigma_small=1.0, azimuths=(120.0,))),
                                           ((2048, 2048), 23, dict(vmin=-50.0, vmax=3000.0))])
def test_large_canvases_against_the_twin(td, shape, seed, kw):
    e = twin.land_and_sea(*shape, seed)
    e[100:140, 200:260] = np.nan
    got = td.relief_map(torch.from_numpy(e).cuda(), **kw).cpu().numpy()
    msg = twin.compare(got, twin.relief(e, **kw))
    assert msg is None, msg


def test_translation_is_bit_identical_away_from_the_crop_edges(td):
    """A render of a crop equals the crop of the render 25 px inside the crop's edges (blur radius 24 + the gradient's 1): catches tile and
    halo indexing errors.  Explicit vmin / vmax so that the colour range does not depend on the extent."""
    e = torch.from_numpy(twin.land_and_sea(2048, 2048, 31)).cuda()
    kw = dict(vmin=0.0, vmax=4000.0)
    full = td.relief_map(e, **kw)
    y0, y1, x0, x1 = 333, 1501, 77, 1990
    part = td.relief_map(e[y0:y1, x0:x1].contiguous(), **kw)
    assert torch.equal(full[y0 + 25:y1 - 25, x0 + 25:x1 - 25], part[25:-25, 25:-25])


def test_two_runs_and_host_vs_device_input_are_bit_identical(td):
    e = twin.land_and_sea(700, 900, 41)
    e[3:9, 500:520] = np.nan
    a = td.get_relief_map(e, None, None, None)
    b = td.get_relief_map(e, None, None, None)
    c = td.get_relief_map(torch.from_numpy(e).cuda(), None, None, None)
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)


def test_enqueue_only_on_a_caller_stream_gives_the_synchronous_result(td):
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    e = torch.from_numpy(twin.land_and_sea(1024, 1024, 51)).cuda()
    ref = td.relief_map(e)
    s = torch.cuda.Stream()
    with eng.on_stream(s, asynchronous=True):
        x = e * 1.0                                   # produced on the caller's stream, consumed there without a host sync
        out = td.relief_map(x, engine=eng)
        got = out.clone()                              # read on that stream after the call
    torch.cuda.current_stream().synchronize()
    assert torch.equal(got, ref)


def test_argument_errors_are_refused(td):
    from terrain_diffusion_amd._lib import TdError
    with pytest.raises(ValueError):
        td.relief_map(torch.zeros(1, 64, device="cuda"))
    with pytest.raises(ValueError):
        td.relief_map(torch.zeros(64, 64, device="cuda"), sigma_large=20.0)   # radius 80 > 64
    import ctypes as C
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.relief import _device_tables, check, lib
    eng = get_engine("cuda")
    e = torch.zeros(8, 8, device="cuda")
    out = torch.empty(8, 8, 3, device="cuda")
    lut, wl, rl, ws, rs = _device_tables(0, 6.0, 1.2)
    dp = lambda t: C.c_void_p(t.data_ptr())
    for H, W, r, src in ((1, 8, rl, e), (8, 1, rl, e), (8, 8, 65, e), (8, 8, -1, e), (8, 8, rl, e.cpu())):
        with pytest.raises(TdError):
            check(lib().td_relief_map(C.c_void_p(eng.stream), dp(src), H, W, dp(lut), dp(wl), r, dp(ws), rs, 315.0, 90.0, 1.0, 0, 0.0, 0.0, 0, 0.0,
                                      dp(out), 1))


@pytest.fixture(scope="module")
def models(td):
    from oracle.unet import COARSE_CONFIG, DECODER_CONFIG, synth_state_dict, tiny_config
    bcfg = tiny_config(64, 1)
    ms = [td.EDMUnet2D(**c, dtype="fp32").load_state_dict(synth_state_dict(c, seed=s)) for c, s in ((COARSE_CONFIG, 1), (bcfg, 2), (DECODER_CONFIG, 3))]
    yield ms
    for m in ms:
        m.close()


def test_relief_of_world_pipeline_output(td, models):
    """The explorer's call (inference/explorer/server.py): get_relief_map(world.get(...)["elev"], None, None, None, resolution=native_resolution)."""
    w = td.WorldPipeline.from_models(*models, seed=4242, decoder_tile_size=64, decoder_tile_stride=48, latents_batch_size=16).bind()
    try:
        elev = w.get(-21, 13, 75, 141, with_climate=False)["elev"]
        img = td.get_relief_map(elev, None, None, None, resolution=w.native_resolution)
        assert isinstance(img, np.ndarray) and img.shape == (96, 128, 3) and img.dtype == np.float32
        assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0
        msg = twin.compare(img, twin.relief(elev.cpu().numpy(), resolution=w.native_resolution))
        assert msg is None, msg
    finally:
        w.close()
