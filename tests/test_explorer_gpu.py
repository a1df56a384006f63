"""Explorer views on the GPU (include/td_explorer.h, explorer_csrc/explorer_kernels.hip): every case recorded from the reference's own routes and
sampler (tests/golden/explorer.npz) through the drop-ins, the NaN-ignoring ranges against NumPy, log1p against the twin, the land-tile search
at the sampler's default window, determinism, host vs device input, the enqueue-only stream mode, the host synchronisations per call counted,
the C-ABI's refusals, and the drop-ins on a real WorldPipeline against the twin (tests/_explorer_twin.py)."""
import ctypes as C
import json
import random
import warnings

import numpy as np
import pytest
import torch

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


class Recorded:
    """A world that answers from recorded blocks: .coarse[:, a:b, c:d] and .get(i1, j1, i2, j2) return the block recorded for exactly that
    box (on `device`), and every read is counted."""
    seed = 4242

    def __init__(self, coarse=None, gets=None, native_resolution=90.0, device="cpu"):
        up = lambda a: None if a is None else torch.from_numpy(a.copy()).to(device)      # uploaded once, here: a read copies nothing from the host
        self.blocks = {k: up(v) for k, v in (coarse or {}).items()}
        self.gets = {k: (up(e), up(c)) for k, (e, c) in (gets or {}).items()}
        self.native_resolution, self.coarse, self.reads = native_resolution, self, 0

    def __getitem__(self, idx):
        ch, si, sj = idx
        assert ch == slice(None)
        self.reads += 1
        return self.blocks[(si.start, si.stop, sj.start, sj.stop)].clone()

    def get(self, i1, j1, i2, j2, with_climate=True):
        self.reads += 1
        elev, clim = self.gets[(i1, j1, i2, j2)]
        return {"elev": elev.clone(), "climate": None if clim is None else clim.clone()}


def test_every_recorded_coarse_case_through_the_drop_ins(ex, golden):
    g = golden("explorer")
    for c in cpu.index(g)["coarse"]:
        box = c["box"]
        planes_want = twin.channels(g["coarse_" + c["name"]])
        for device in ("cpu", "cuda"):
            world = Recorded({tuple(box): g["coarse_" + c["name"]]}, device=device)

            def image(v):
                before = world.reads
                out = ex.coarse_image(world, v["channel"], *box, filters=cpu.filters_of(v))
                assert world.reads == before + 1, "the coarse region is read once"
                return out
            cpu.check_coarse_case(g, c, image, lambda: ex.coarse_stats(world, *box), lambda: ex.coarse_data(world, *box))
            planes, minmax = ex.coarse_channels(world.coarse[:, box[0]:box[1], box[2]:box[3]])
            assert np.array_equal(planes.cpu().numpy().view(np.uint32), planes_want.view(np.uint32)), c["name"]
            for ch in range(6):
                lo, hi = twin.nan_range(planes_want[ch])
                assert minmax[ch].cpu().tolist() == [lo, hi], (c["name"], ch)


def test_every_recorded_detail_case_through_the_drop_ins(ex, golden):
    g = golden("explorer")
    for c in cpu.index(g)["detail"]:
        n, a = c["name"], c["args"]
        clim = g["climate_" + n] if "climate_" + n in g.files else None
        world = Recorded(gets={tuple(c["box"]): (g["elev_" + n], clim)}, native_resolution=c["native_resolution"], device="cuda")
        for mode in c["modes"]:
            img = ex.detail_image(world, mode=mode, **a)
            want = g[f"png_{n}_{mode}"]
            assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == want.shape
            if mode == "relief" or (mode == "temperature" and clim is None):
                cpu.check_relief_image(img, want, (n, mode))
            else:
                assert np.array_equal(img, want), (n, mode, int((img != want).any(-1).sum()))
        if "raw_" + n in g.files:
            body, hdr = ex.detail_raw(world, **a)
            assert body == bytes(g["raw_" + n]) and hdr == json.loads(str(g["rawhdr_" + n])), n


def test_every_recorded_land_case_through_the_drop_ins(ex, golden, capsys):
    g = golden("explorer")
    blocks = {(-12, 12, -12, 12): g["land_coarse"]}
    for c in cpu.index(g)["info"]:
        blocks[(c["ci"], c["ci"] + 1, c["cj"], c["cj"] + 1)] = g["info_coarse_" + c["name"]]
    world = Recorded(blocks, device="cuda")
    for c in cpu.index(g)["land"]:
        n = c["name"]
        random.seed(int(g["seed"]))
        picks = ex.sample_land_tiles(world, c["window"], c["detail_size"], c["min_land_frac"], c["n_samples"])
        assert picks == [tuple(t) for t in g["picks_" + n].tolist()], n
        capsys.readouterr()
        full = ex.sample_land_tiles(world, c["window"], c["detail_size"], c["min_land_frac"], 10 ** 9)
        assert full == [tuple(t) for t in g["full_" + n].tolist()], n
        assert capsys.readouterr().out == f"Warning: Only found {len(full)} valid land tiles (requested {10 ** 9})\n"
    for c in cpu.index(g)["info"]:
        info = ex.get_coarse_climate_info(world, c["ci"], c["cj"])
        assert list(info) == ["temp", "temp_std", "precip", "precip_cv"] and list(info.values()) == g["info_" + c["name"]].tolist()


def _range_cases():
    rng = np.random.default_rng(3)
    out = []
    for shape in ((1, 1), (1, 63), (1, 64), (5, 13), (1, 4097), (1000, 1003)):
        a = (rng.standard_normal(shape) * 100).astype(F)
        out.append(("plain", a))
        b = a.copy()
        b.flat[0] = b.flat[-1] = np.nan
        out.append(("nan_ends", b))
        out.append(("all_nan", np.full(shape, np.nan, F)))
        c = a.copy()
        c.flat[rng.integers(c.size)] = np.inf
        c.flat[rng.integers(c.size)] = -np.inf
        out.append(("inf", c))
        z = np.where(rng.random(shape) < 0.5, F(0.0), F(-0.0)).astype(F)
        out.append(("zeros", z))
    return out


def test_nan_ignoring_ranges_against_numpy(ex):
    lut = np.zeros((256, 3), F)
    for name, a in _range_cases():
        lo, hi = twin.nan_range(a)
        sums = np.stack([a, np.ones_like(a)])
        _, mm = ex.coarse_channels(sums, n_signed_sq=0, eps=0.0)
        _, vmin, vmax = ex.colorize(torch.from_numpy(a).cuda(), lut)
        for got in (mm[0].cpu().tolist(), [float(vmin), float(vmax)]):
            if np.isnan(lo):
                assert np.isnan(got[0]) and np.isnan(got[1]), (name, a.shape)
            else:
                assert got == [lo, hi], (name, a.shape, got, lo, hi)     # -0.0 == +0.0: either zero is accepted


def test_log1p_is_within_one_ulp_of_the_twin(ex):
    """The displayed value of a one-pixel field is its own vmin: 200 values over the precipitation range and the edges."""
    rng = np.random.default_rng(4)
    xs = np.concatenate([[0.0, -3.0, 1e-30, 1e-7, 1.0, 3.4e38, np.inf], 10.0 ** rng.uniform(-6, 5, 193)]).astype(F)
    lut = torch.zeros(256, 3, device="cuda")
    for x in xs:
        _, vmin, vmax = ex.colorize(torch.full((1, 1), float(x), device="cuda"), lut, log1p=True)
        want = twin.display(np.array([[x]], F), True)[0, 0]
        got = F(float(vmin))
        assert float(vmax) == float(vmin)
        assert got == want or abs(float(got) - float(want)) <= float(np.spacing(want)), (x, got, want)


@pytest.mark.parametrize("half,frac", [(2, 0.5), (5, 0.7)])
def test_land_tiles_at_the_default_window_against_the_twin(ex, half, frac):
    rng = np.random.default_rng(10 + half)
    import _relief_twin
    e = _relief_twin.land_and_sea(600, 600, 61, sea=1.0 - frac)      # about `frac` land, so that the threshold cuts through the map
    e[rng.integers(0, 600, 50), rng.integers(0, 600, 50)] = np.nan
    want = twin.land_tiles(e, half, frac)
    idx, count = ex.land_tiles(torch.from_numpy(e).cuda(), half, frac)
    n = int(count)
    assert idx.dtype == torch.int32 and idx.numel() == (600 - 2 * half) ** 2
    assert 0 < len(want) < idx.numel() and n == len(want)
    assert np.array_equal(idx[:n].cpu().numpy(), want)
    if half == 5:
        assert not np.array_equal(want, twin.land_tiles(e, half, frac, exact=True))    # windows of exactly 70 cells exist and are left out
    idx0, count0 = ex.land_tiles(torch.from_numpy(e).cuda(), 0, 0.0)
    assert int(count0) == 0 and idx0.numel() == 0
    idx1, count1 = ex.land_tiles(torch.from_numpy(e[:10, :600]).cuda(), 5, 0.0)       # 2 half == H: no position
    assert int(count1) == 0


def _views(ex, world_coarse, elev, temp, filt):
    planes, mm = ex.coarse_channels(world_coarse)
    img, vmin, vmax = ex.colorize(planes[4], "viridis", log1p=True, filters=[(planes[0], filt, None), (planes[2], None, 15.0)])
    img2, _, _ = ex.colorize(elev, "terrain", vmin=-100.0, vmax=2500.5)
    raw = ex.raw_tile(elev, temp)
    idx, count = ex.land_tiles(planes[0], 2, 0.5)
    rgb = ex.relief_rgba8(torch.stack([planes[0], planes[2], planes[4]], dim=-1) / 50.0)
    return [planes, mm, img, vmin, vmax, img2, raw, count, idx, rgb]


def _inputs(golden):
    g = golden("explorer")
    return g["coarse_odd"], g["elev_nan"], g["climate_nan"][0]


def _same(a, b):
    n = int(a[7])
    assert int(b[7]) == n
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = (x[:n], y[:n]) if k == 8 else (x, y)
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True), k


def test_two_runs_and_host_vs_device_input_are_bit_identical(ex, golden):
    coarse, elev, temp = _inputs(golden)
    a = _views(ex, coarse, elev, temp, 0.0)
    b = _views(ex, coarse, elev, temp, 0.0)
    c = _views(ex, *(torch.from_numpy(v).cuda() for v in (coarse, elev, temp)), 0.0)
    _same(a, b)
    _same(a, c)
    assert a[2].shape == (41, 37, 4) and a[6].numel() == 6 * 96 * 96


def test_enqueue_only_on_a_caller_stream_gives_the_synchronous_result(ex, golden):
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    dev = [torch.from_numpy(v).cuda() for v in _inputs(golden)]
    ref = _views(ex, *dev, 0.0)
    s = torch.cuda.Stream()
    with eng.on_stream(s, asynchronous=True):
        x = [t * 1.0 for t in dev]                     # produced on the caller's stream, consumed there without a host sync
        got = [t.clone() for t in _views(ex, *x, 0.0)]   # read on that stream after the calls
    torch.cuda.current_stream().synchronize()
    _same(got, ref)


class _Syncs:
    """Counts what can synchronise the host inside a block: torch's own synchronising operations (sync debug mode "warn": .cpu(), .item(),
    bool(tensor)), explicit stream / device synchronisations, and the module's device-to-host copies."""

    def __init__(self, ex, monkeypatch):
        self.ex, self.mp, self.explicit = ex, monkeypatch, 0

    def __enter__(self):
        def counted(fn):
            def wrapper(*a, **k):
                self.explicit += 1
                return fn(*a, **k)
            return wrapper
        self.mp.setattr(torch.cuda.Stream, "synchronize", counted(torch.cuda.Stream.synchronize))
        self.mp.setattr(torch.cuda, "synchronize", counted(torch.cuda.synchronize))
        self.copies0 = self.ex.HOST_COPIES
        self.catch = warnings.catch_warnings(record=True)
        self.caught = self.catch.__enter__()
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        return self

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        self.catch.__exit__(*exc)
        self.mp.undo()
        self.copies = self.ex.HOST_COPIES - self.copies0
        self.messages = [str(w.message) for w in self.caught if "called a synchronizing" in str(w.message)]     # not the mode's own notice
        self.torch_syncs = len(self.messages)
        return False


def test_one_host_synchronisation_per_call(ex, golden, monkeypatch):
    g = golden("explorer")
    idx = cpu.index(g)
    d = {c["name"]: c for c in idx["detail"]}
    coarse_box = tuple(idx["coarse"][0]["box"])
    world = Recorded({coarse_box: g["coarse_odd"], (-12, 12, -12, 12): g["land_coarse"], (-5, 5, -5, 5): g["land_coarse"][:, 7:17, 7:17]},
                     {tuple(d["clim"]["box"]): (g["elev_clim"], g["climate_clim"]), tuple(d["raw"]["box"]): (g["elev_raw"], g["climate_raw"])},
                     device="cuda")
    a96, a64 = d["clim"]["args"], d["raw"]["args"]
    calls = {
        "coarse_image": (lambda: ex.coarse_image(world, 4, *coarse_box, filters={0: (0.0, None), 3: (None, 900.0)}), 1, 1),
        "coarse_stats": (lambda: ex.coarse_stats(world, *coarse_box), 1, 1),
        "coarse_data": (lambda: ex.coarse_data(world, *coarse_box), 1, 1),
        "detail_elevation": (lambda: ex.detail_image(world, mode="elevation", **a96), 1, 1),
        "detail_temperature": (lambda: ex.detail_image(world, mode="temperature", **a96), 1, 1),
        "detail_relief": (lambda: ex.detail_image(world, mode="relief", **a96), 1, 2),        # + relief_map's NaN check
        "detail_raw": (lambda: ex.detail_raw(world, **a64), 1, 1),
        "sample_land_tiles_24": (lambda: ex.sample_land_tiles(world, 12, 1024, 0.5, 5), 2, 2),
        "sample_land_tiles_10": (lambda: ex.sample_land_tiles(world, 5, 512, 0.5, 5), 2, 2),   # the same count for another window
    }
    for name, (fn, copies, syncs) in calls.items():
        fn()   # warm-up: colour tables and blur weights are uploaded once per GPU
        with _Syncs(ex, monkeypatch) as s:
            fn()
        assert (s.copies, s.torch_syncs, s.explicit) == (copies, syncs, 0), (name, s.copies, s.messages, s.explicit)


def test_c_abi_argument_errors(ex):
    from terrain_diffusion_amd._lib import TdError
    from terrain_diffusion_amd.engine import get_engine
    st = C.c_void_p(get_engine("cuda").stream)
    l = ex.lib()
    dp = lambda t: C.c_void_p(t.data_ptr())
    sums, out, mm = torch.ones(10, 8, 8, device="cuda"), torch.empty(9, 8, 8, device="cuda"), torch.empty(9, 2, device="cuda")
    field, lut, rgba, rng = torch.zeros(8, 8, device="cuda"), torch.zeros(256, 3, device="cuda"), torch.empty(8, 8, 4, dtype=torch.uint8, device="cuda"), torch.empty(2, device="cuda")
    idx, cnt = torch.empty(64, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    raw = torch.empty(6 * 64, dtype=torch.uint8, device="cuda")
    host = torch.zeros(8, 8)
    planes9, d9, i9 = (C.c_void_p * 9)(*[field.data_ptr()] * 9), (C.c_double * 9)(), (C.c_int * 9)()
    hostp = (C.c_void_p * 1)(host.data_ptr())
    bad = [
        lambda: l.td_explorer_channels(st, dp(sums), 0, 8, 8, 0, 1e-8, dp(out), dp(mm), 1),
        lambda: l.td_explorer_channels(st, dp(sums), 9, 8, 8, 0, 1e-8, dp(out), dp(mm), 1),
        lambda: l.td_explorer_channels(st, dp(sums), 6, 0, 8, 2, 1e-8, dp(out), dp(mm), 1),
        lambda: l.td_explorer_channels(st, dp(sums), 6, 8, 8, 7, 1e-8, dp(out), dp(mm), 1),
        lambda: l.td_explorer_channels(st, dp(host), 1, 4, 8, 0, 1e-8, dp(out), dp(mm), 1),
        lambda: l.td_explorer_channels(st, None, 6, 8, 8, 2, 1e-8, dp(out), dp(mm), 1),
        lambda: l.td_explorer_channels(st, dp(sums), 6, 1 << 14, 1 << 14, 2, 1e-8, dp(out), dp(mm), 1),
        lambda: l.td_explorer_colorize(st, dp(field), 8, 0, 0, 0, 0.0, 0.0, dp(lut), 0, None, None, None, None, None, dp(rgba), dp(rng), 1),
        lambda: l.td_explorer_colorize(st, dp(field), 8, 8, 0, 0, 0.0, 0.0, dp(lut), 9, planes9, d9, d9, i9, i9, dp(rgba), dp(rng), 1),
        lambda: l.td_explorer_colorize(st, dp(field), 8, 8, 0, 0, 0.0, 0.0, dp(lut), 1, hostp, d9, d9, i9, i9, dp(rgba), dp(rng), 1),
        lambda: l.td_explorer_colorize(st, dp(field), 8, 8, 0, 1, 2.0, 2.0, dp(lut), 0, None, None, None, None, None, dp(rgba), dp(rng), 1),
        lambda: l.td_explorer_colorize(st, dp(field), 8, 8, 0, 0, 0.0, 0.0, dp(host), 0, None, None, None, None, None, dp(rgba), dp(rng), 1),
        lambda: l.td_explorer_colorize(st, dp(field), 8, 8, 0, 0, 0.0, 0.0, dp(lut), 0, None, None, None, None, None, None, dp(rng), 1),
        lambda: l.td_explorer_quantize(st, dp(host), 8, 8, dp(rgba), 1),
        lambda: l.td_explorer_quantize(st, dp(field), -1, 8, dp(rgba), 1),
        lambda: l.td_explorer_raw(st, dp(field), dp(host), 8, 8, dp(raw), 1),
        lambda: l.td_explorer_raw(st, dp(field), None, 8, 8, None, 1),
        lambda: l.td_explorer_raw(st, dp(field), None, 8, 8, C.c_void_p(raw.data_ptr() + 1), 1),
        lambda: l.td_explorer_land_tiles(st, dp(field), 8, 8, -1, 0.5, dp(idx), dp(cnt), 1),
        lambda: l.td_explorer_land_tiles(st, dp(field), 8, 8, 5, 0.5, dp(idx), dp(cnt), 1),
        lambda: l.td_explorer_land_tiles(st, dp(field), 8, 8, 2, 0.5, None, dp(cnt), 1),
        lambda: l.td_explorer_land_tiles(st, dp(host), 8, 8, 2, 0.5, dp(idx), dp(cnt), 1),
        lambda: l.td_explorer_land_tiles(st, dp(field), 8, 8, 2, float("nan"), dp(idx), dp(cnt), 1),
    ]
    for k, fn in enumerate(bad):
        with pytest.raises(TdError):
            ex.check(fn())
        assert ex.lib().td_explorer_last_error().decode().startswith("td_explorer_"), k
    ex.check(l.td_explorer_land_tiles(st, dp(field), 8, 8, 0, 0.5, None, dp(cnt), 1))      # half 0: no index buffer needed
    assert int(cnt) == 0


@pytest.fixture(scope="module")
def models():
    import terrain_diffusion_amd as td
    from oracle.unet import COARSE_CONFIG, DECODER_CONFIG, synth_state_dict, tiny_config
    bcfg = tiny_config(64, 1)
    ms = [td.EDMUnet2D(**c, dtype="fp32").load_state_dict(synth_state_dict(c, seed=s)) for c, s in ((COARSE_CONFIG, 1), (bcfg, 2), (DECODER_CONFIG, 3))]
    yield ms
    for m in ms:
        m.close()


def test_the_drop_ins_on_a_world_pipeline_against_the_twin(ex, models, golden):
    import terrain_diffusion_amd as td
    g = golden("explorer")
    luts = cpu.luts(g)
    w = td.WorldPipeline.from_models(*models, seed=4242, decoder_tile_size=64, decoder_tile_stride=48, latents_batch_size=16).bind()
    try:
        box = (-6, 7, -5, 6)
        block = w.coarse[:, box[0]:box[1], box[2]:box[3]].cpu().numpy()
        assert block.shape == (7, 13, 11)
        for ch, filt in ((0, None), (2, {0: (0.0, None)}), (4, {2: (None, float(np.nanmedian(twin.channels(block)[2])))})):
            img, hdr = ex.coarse_image(w, ch, *box, filters=filt)
            want, want_hdr, margin = twin.coarse_image(block, ch, luts["viridis"], filt)
            if ch == 4:
                exempt = margin <= 4
                assert np.array_equal(img[~exempt], want[~exempt])
            else:
                assert np.array_equal(img, want) and hdr == want_hdr, ch
        assert cpu.json_equal(cpu.stats_as_json(ex.coarse_stats(w, *box)), cpu.stats_as_json(twin.coarse_stats(block)))
        assert cpu.json_equal(ex.coarse_data(w, *box), twin.coarse_data(block, list(box)))
        a = dict(ci=0, cj=0, detail_size=96, pan_i=27, pan_j=77)
        region = w.get(27 - 48, 77 - 48, 27 + 48, 77 + 48)
        elev, clim = region["elev"].cpu().numpy(), region["climate"].cpu().numpy()
        for mode in ("elevation", "temperature", "relief"):
            img = ex.detail_image(w, mode=mode, **a)
            want, kind, _ = twin.detail_image(elev, clim, mode, luts, w.native_resolution)
            assert kind == mode and img.shape == (96, 96, 4)
            if mode == "relief":
                cpu.check_relief_image(img, want, mode)
            else:
                assert np.array_equal(img, want), mode
        body, hdr = ex.detail_raw(w, **a)
        assert body == twin.raw_tile(elev, clim[0]) and hdr == {"X-Height": "96", "X-Width": "96", "X-Has-Temp": "1"}
        win = 8
        cblock = w.coarse[:, -win:win, -win:win].cpu().numpy()
        frac = float((twin.channels(cblock, eps=0.0)[0] > 0).mean())
        for ds, n in ((1024, 5), (512, 10 ** 6)):
            random.seed(7)
            got = ex.sample_land_tiles(w, win, ds, frac, n)
            random.seed(7)
            assert got == twin.sample_land_tiles(cblock, win, ds, frac, n), ds
        info = ex.get_coarse_climate_info(w, 2, -3)
        assert info == twin.climate_info(w.coarse[:, 2:3, -3:-2].cpu().numpy())
        png = ex.png_bytes(ex.detail_image(w, mode="elevation", **a))
        assert np.array_equal(twin.decode_png(png), twin.detail_image(elev, clim, "elevation", luts)[0])
    finally:
        w.close()
