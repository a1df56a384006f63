"""Minecraft terrain on the GPU (libtd_mc.so, mc_csrc/mc_kernels.hip): every case recorded from the reference's own minecraft_api.py and
api.py (tests/golden/mc.npz) through the drop-ins with the recorded noise replayed, the built-in noise and large requests against the NumPy
twin (tests/_mc_twin.py), translation, determinism, host vs device input, the enqueue-only stream mode, refusals, and requests on a
WorldPipeline."""
import json

import numpy as np
import pytest
import torch

import _mc_twin as twin
from test_mc_cpu import cases, check_case
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available()
    return t


class ReplayWorld:
    """Hands out the recorded windows in the recorded order, checking each request against the recorded one."""

    def __init__(self, c, wins):
        self.native_resolution, self.gets, self.wins, self.k = c["native_resolution"], c["gets"], wins, 0

    def get(self, i1, j1, i2, j2, with_climate=True):
        assert [i1, j1, i2, j2, with_climate] == self.gets[self.k], (self.k, [i1, j1, i2, j2, with_climate])
        e, cl = self.wins[self.k]
        self.k += 1
        return {"elev": torch.from_numpy(e.copy()).cuda(), "climate": None if cl is None else torch.from_numpy(cl.copy()).cuda()}


def replay_noise(planes, i0, j0):
    H, W = planes.shape[1:]
    want = twin.coords(i0, j0, H, W)

    def fn(name, coords):
        assert np.array_equal(coords, want) and coords.dtype == np.float32
        return planes[twin.NAMES.index(name)].ravel().copy()
    return fn


def ulps(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    d = twin.ulp_distance(a, b)
    return int(np.where(np.isnan(a) & np.isnan(b), 0, d).max()) if a.size else 0


def test_every_recorded_case_through_the_drop_ins(td, golden):
    seen, exempt = {"mc": 0, "api": 0}, 0
    for c, wins, g in cases(golden):
        n, s, box = c["name"], c["scale"], c["box"]
        i1, j1, i2, j2 = box
        H, W = i2 - i1, j2 - j1
        planes = g["noise_" + n]
        fn = replay_noise(planes, i1, j1)
        if c["fn"] == "api":
            got = td.get_terrain(ReplayWorld(c, wins), *box, s)
            en, cn = wins[0]
            r0, c0 = twin.crop_origin(i1, j1, s, 1) if s > 1 else (0, 0)
            want = twin.get_terrain(en, cn, *box, s) if s > 1 else {"elev": en, "climate": cn}
            assert np.array_equal(got["elev"].cpu().numpy(), want["elev"]), n                          # the twin, bit for bit
            from test_mc_cpu import upsample_close
            assert upsample_close(got["elev"].cpu().numpy(), g["elev_" + n], en, s, r0, c0)[0], n   # the reference, to 2 ulp
            assert (got["climate"] is None) == (cn is None), n
            if cn is not None:
                assert np.array_equal(got["climate"].cpu().numpy(), want["climate"]), n
                assert upsample_close(got["climate"].cpu().numpy(), g["climate_" + n], cn, s, r0, c0)[0], n
            seen["api"] += 1
            continue
        elev, biome = td.minecraft_terrain(ReplayWorld(c, wins), *box, scale=s, noise_scale=c["noise"], noise_fn=fn)
        assert elev.dtype == torch.float32 and biome.dtype == torch.int16 and tuple(biome.shape) == (H, W), n
        body, hdr = td.minecraft_payload(elev, biome)
        assert hdr == {"X-Height": str(H), "X-Width": str(W), "X-Dtype": "int16-le"}, n
        e, b = elev.cpu().numpy(), biome.cpu().numpy()
        if s == 1:
            exempt += check_case(c, wins, g, e, b, payload=body)
        else:
            up = td.get_upsampled(ReplayWorld(c, wins), *box, s, c["noise"], c["native_resolution"] / s, noise_fn=fn)
            assert torch.equal(up["elev"], elev) or (c["kind"] == "nan" and np.array_equal(up["elev"].cpu().numpy(), e, equal_nan=True)), n
            sm, pd = up["elev_smooth"].cpu().numpy(), up["elev_padded"].cpu().numpy()
            cl = None if up["climate"] is None else up["climate"].cpu().numpy()
            exempt += check_case(c, wins, g, e, b, sm, pd, cl, body)
            b2 = td.classify_biome(up["elev_smooth"], up["climate"], i1, j1, up["elev_padded"], c["native_resolution"] / s, noise_fn=fn)
            assert np.array_equal(b2.cpu().numpy(), b), n
            # the twin, bit for bit (the noise is the recorded one)
            want = twin.get_upsampled(*wins[0], *box, s, c["noise"], c["native_resolution"] / s, c["native_resolution"], planes)
            assert np.array_equal(pd, want["elev_padded"], equal_nan=True) and np.array_equal(e, want["elev"], equal_nan=True), n
        want_e, want_b = twin.minecraft_terrain(wins, *box, s, c["noise"], c["native_resolution"], planes)
        assert np.array_equal(b, want_b), n
        assert body == twin.payload(e, b), n
        seen["mc"] += 1
    print(f"margin-exempt pixels over all recorded cases: {exempt}")
    assert seen == {"mc": 24, "api": 6}


@pytest.mark.parametrize("i0,j0,H,W", [(0, 0, 64, 80), (-1000, 777, 300, 257), (123456, -98765, 512, 384)])
def test_built_in_noise_is_the_twins_bit_for_bit(td, i0, j0, H, W):
    got = td.noise_planes(i0, j0, H, W).cpu().numpy()
    want = twin.noise_planes(i0, j0, H, W)
    assert got.shape == (7, H, W) and np.array_equal(got, want)
    assert np.array_equal(got[0], got[3]) and np.array_equal(got[1], got[4]) and not np.array_equal(got[0], got[2])
    assert np.abs(got).max() < 1.5 and got.std(axis=(1, 2)).min() > 0.02


class FieldWorld:
    """A crop-consistent world: smooth fp32 fields of the absolute native pixel, sea and land, ridges steep enough for bare slopes, the
    climate spanning frozen to hot, arid to wet."""
    native_resolution = 90.0

    def __init__(self, seed=0):
        self.seed, self.calls = seed, 0

    def fields(self, i1, j1, i2, j2, with_climate):
        ii, jj = np.meshgrid(np.arange(i1, i2, dtype=np.float64), np.arange(j1, j2, dtype=np.float64), indexing="ij")
        ph = 0.37 * self.seed
        elev = 1400 * np.sin(ii / 53.0 + ph) * np.cos(jj / 71.0) + 900 * np.sin((ii + 2 * jj) / 23.0) + 600 * np.cos(jj / 9.0 - ii / 13.0) + 300
        temp = 12 + 18 * np.sin(ii / 97.0 - ph) + 6 * np.cos(jj / 41.0)
        ts = 700 + 600 * np.sin(jj / 61.0)
        precip = 900 + 850 * np.cos(ii / 37.0 + jj / 89.0)
        pcv = 60 + 50 * np.sin(ii / 29.0 + jj / 17.0)
        clim = np.stack([temp, ts, precip, pcv, 0.0065 + 0 * temp]).astype(F) if with_climate else None
        return elev.astype(F), clim

    def get(self, i1, j1, i2, j2, with_climate=True):
        self.calls += 1
        e, c = self.fields(i1, j1, i2, j2, with_climate)
        return {"elev": torch.from_numpy(e).cuda(), "climate": None if c is None else torch.from_numpy(c).cuda()}


def twin_request(world, i1, j1, i2, j2, s, noise_scale, chunk=512):
    """The twin's (elev, biome, margin, elev_padded, climate) of a request, row chunk by row chunk (each chunk a request of its own on the
    crop-consistent world: the same values, bounded memory)."""
    outs = {k: [] for k in ("elev", "biome", "margin", "padded", "climate")}
    for a in range(i1, i2, chunk):
        b = min(a + chunk, i2)
        H, W = b - a, j2 - j1
        planes = twin.noise_planes(a, j1, H, W)
        nr = world.native_resolution
        if s == 1:
            wins = [world.fields(a - 1, j1 - 1, b + 1, j2 + 1, False), world.fields(a, j1, b, j2, True)]
            e, bio = twin.minecraft_terrain(wins, a, j1, b, j2, 1, noise_scale, nr, planes)
            m = twin.margin(e, wins[1][1], twin.gradient(wins[0][0]), nr, planes)
            outs["padded"].append(None)
            outs["climate"].append(wins[1][1])
        else:
            win = world.fields(*twin.native_box(a, j1, b, j2, s, 2), True)
            up = twin.get_upsampled(*win, a, j1, b, j2, s, noise_scale, nr / s, nr, planes)
            e = up["elev"]
            grad = twin.gradient(up["elev_padded"])
            bio = twin.classify(up["elev_smooth"], up["climate"], grad, nr / s, planes)
            m = twin.margin(up["elev_smooth"], up["climate"], grad, nr / s, planes)
            outs["padded"].append(up["elev_padded"][1:-1])
            outs["climate"].append(up["climate"])
        outs["elev"].append(e); outs["biome"].append(bio); outs["margin"].append(m)
    return {k: (None if v[0] is None else np.concatenate(v, axis=-2)) for k, v in outs.items()}


@pytest.mark.parametrize("n,s,i1,j1", [(2048, 8, -3001, 517), (4096, 4, 1203, -2222), (1024, 1, -517, 300)])
def test_large_requests_against_the_twin(td, n, s, i1, j1):
    world = FieldWorld(seed=s)
    elev, biome = td.minecraft_terrain(world, i1, j1, i1 + n, j1 + n, scale=s, noise_scale=1.0)
    e, b = elev.cpu().numpy(), biome.cpu().numpy()
    want = twin_request(world, i1, j1, i1 + n, j1 + n, s, 1.0)
    if s > 1:
        up = td.get_upsampled(world, i1, j1, i1 + n, j1 + n, s, 0.0, world.native_resolution / s)
        assert np.array_equal(up["elev_padded"][1:-1].cpu().numpy(), want["padded"])     # upsample, bit for bit
        assert np.array_equal(up["climate"].cpu().numpy(), want["climate"])
        assert ulps(e, want["elev"]) <= 2                                              # detail amplitude: pow(1.5)
    else:
        assert np.array_equal(e, want["elev"])
    ok = want["margin"] >= 4
    assert np.array_equal(b[ok], want["biome"][ok]), int((b != want["biome"]).sum())
    print(f"{n}^2 at {s}x: {int((~ok).sum())} margin-exempt pixels, {int((b != want['biome']).sum())} differing; ids {np.unique(b).tolist()}")
    assert len(np.unique(b)) >= 10 and ok.mean() > 0.999
    body, _ = td.minecraft_payload(elev, biome)
    assert body == twin.payload(e, b)


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_a_sub_box_is_the_same_pixels_of_the_larger_request(td, s):
    # power-of-two scales only: with an inexact fl32(1 / s) torch's source index, hence the weight of an absolute pixel, depends on where the
    # native window starts -- the reference's values move with the request there too
    world = FieldWorld(seed=5)
    i1, j1, i2, j2 = -77, -45, 180, 201
    e, b = (t.cpu().numpy() for t in td.minecraft_terrain(world, i1, j1, i2, j2, scale=s))
    for (a, c, h, w) in ((-77, -45, 1, 9), (-61, -3, 9, 1), (-5, 17, 7, 5), (11, 13, 100, 121), (-76, -44, 255, 245)):
        es, bs = (t.cpu().numpy() for t in td.minecraft_terrain(world, a, c, a + h, c + w, scale=s))
        sl = (slice(a - i1, a - i1 + h), slice(c - j1, c - j1 + w))
        assert np.array_equal(es, e[sl]) and np.array_equal(bs, b[sl]), (s, a, c, h, w)
    if s > 1:
        t1 = td.get_terrain(world, i1, j1, i2, j2, s)
        t2 = td.get_terrain(world, -3, 5, 40, 47, s)
        assert torch.equal(t2["elev"], t1["elev"][-3 - i1:40 - i1, 5 - j1:47 - j1])
        assert torch.equal(t2["climate"], t1["climate"][:, -3 - i1:40 - i1, 5 - j1:47 - j1])


def test_determinism_and_host_vs_device_input(td):
    world = FieldWorld(seed=9)
    runs = [td.minecraft_terrain(world, 100, -300, 612, 212, scale=4) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    up = td.get_upsampled(world, 100, -300, 612, 212, 4, 0.0, 22.5)
    host = [up["elev_smooth"].cpu().numpy(), up["climate"].cpu().numpy(), up["elev_padded"].cpu().numpy()]
    bd = td.classify_biome(up["elev_smooth"], up["climate"], 100, -300, up["elev_padded"], 22.5)
    bh = td.classify_biome(*host[:2], 100, -300, host[2], 22.5)
    bf = td.classify_biome(*(torch.from_numpy(x).double() for x in host[:2]), 100, -300, torch.from_numpy(host[2]).double(), 22.5)
    assert torch.equal(bd, bh) and torch.equal(bd, bf) and torch.equal(bd, runs[0][1])
    p1, _ = td.minecraft_payload(runs[0][0], runs[0][1])
    p2, _ = td.minecraft_payload(runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy())
    assert p1 == p2


def test_enqueue_only_on_a_caller_stream_gives_the_synchronous_result(td):
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    world = FieldWorld(seed=3)
    ref_e, ref_b = td.minecraft_terrain(world, -512, 256, 512, 1280, scale=8, noise_scale=2.0)
    ref_p, _ = td.minecraft_payload(ref_e, ref_b)
    ref_n = td.noise_planes(5, 6, 300, 200)
    s = torch.cuda.Stream()
    with eng.on_stream(s, asynchronous=True):
        e, b = td.minecraft_terrain(world, -512, 256, 512, 1280, scale=8, noise_scale=2.0, engine=eng)
        n = td.noise_planes(5, 6, 300, 200, engine=eng)
        got = [e.clone(), b.clone(), n.clone()]
        p, _ = td.minecraft_payload(e, b, engine=eng)
    torch.cuda.current_stream().synchronize()
    assert torch.equal(got[0], ref_e) and torch.equal(got[1], ref_b) and torch.equal(got[2], ref_n) and p == ref_p


def test_refusals(td):
    import ctypes as C
    from terrain_diffusion_amd._lib import TdError
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.minecraft import check, lib
    world = FieldWorld()
    for bad in (dict(scale=0), dict(scale=-1), dict(scale=1.5)):
        with pytest.raises(ValueError):
            td.minecraft_terrain(world, 0, 0, 8, 8, **bad)
    with pytest.raises(ValueError):
        td.minecraft_terrain(world, 0, 0, 0, 8, scale=2)
    with pytest.raises(ValueError):
        td.get_terrain(world, 0, 0, 1 << 17, 1, 2)
    with pytest.raises(ValueError):
        td.classify_biome(torch.zeros(4, 5, device="cuda"), torch.zeros(5, 4, 4, device="cuda"), 0, 0, torch.zeros(6, 7, device="cuda"))

    class Liar(FieldWorld):
        def get(self, i1, j1, i2, j2, with_climate=True):
            out = super().get(i1, j1, i2, j2, with_climate)
            out["climate"] = out["climate"][:, :-1]
            return out
    with pytest.raises(ValueError):
        td.minecraft_terrain(Liar(), 0, 0, 16, 16, scale=4)
    with pytest.raises(ValueError):
        td.minecraft_terrain(world, 0, 0, 16, 16, scale=2, noise_fn=lambda n, c: np.zeros(3, F))
    eng = get_engine("cuda")
    st = C.c_void_p(eng.stream)
    src = torch.zeros(5, 10, 12, device="cuda")
    out = torch.empty(5, 8, 8, device="cuda")
    dp = lambda t: C.c_void_p(t.data_ptr())
    for args in ((5, 10, 12, 4, 33, 0, 8, 8), (5, 10, 12, 4, 0, 41, 8, 8), (5, 10, 12, 4, -1, 0, 8, 8), (5, 10, 12, 0, 0, 0, 8, 8),
                 (0, 10, 12, 4, 0, 0, 8, 8), (5, 10, 12, 4, 0, 0, 0, 8)):
        with pytest.raises(TdError):
            check(lib().td_mc_upsample(st, dp(src), *args, dp(out), 1))
    with pytest.raises(TdError):   # host buffer
        check(lib().td_mc_upsample(st, dp(src.cpu()), 5, 10, 12, 4, 0, 0, 8, 8, dp(out), 1))
    e = torch.zeros(8, 8, device="cuda")
    p = torch.zeros(10, 10, device="cuda")
    b = torch.empty(8, 8, dtype=torch.int16, device="cuda")
    with pytest.raises(TdError):   # row pitch below W
        check(lib().td_mc_finish(st, dp(e), 7, dp(p), None, 0, 8, 8, 0, 0, None, 1.0, 90.0, 90.0, 90.0, None, dp(b), 1))
    with pytest.raises(TdError):
        check(lib().td_mc_finish(st, dp(e), 8, dp(p), None, 0, 8, (1 << 16) + 1, 0, 0, None, 1.0, 90.0, 90.0, 90.0, None, dp(b), 1))
    with pytest.raises(TdError):
        check(lib().td_mc_payload(st, dp(e), None, 1 << 14, 1 << 14, dp(b), 1))
    with pytest.raises(TdError):
        check(lib().td_mc_noise(st, 0, 8, 0, 0, dp(e), 1))


@pytest.fixture(scope="module")
def models(td):
    from oracle.unet import COARSE_CONFIG, DECODER_CONFIG, synth_state_dict, tiny_config
    bcfg = tiny_config(64, 1)
    ms = [td.EDMUnet2D(**c, dtype="fp32").load_state_dict(synth_state_dict(c, seed=s)) for c, s in ((COARSE_CONFIG, 1), (bcfg, 2), (DECODER_CONFIG, 3))]
    yield ms
    for m in ms:
        m.close()


class Recording:
    """Passes world.get through and keeps a host copy of what it returned."""

    def __init__(self, world):
        self.world, self.native_resolution, self.wins = world, world.native_resolution, []

    def get(self, i1, j1, i2, j2, with_climate=True):
        out = self.world.get(i1, j1, i2, j2, with_climate=with_climate)
        c = out.get("climate")
        self.wins.append((out["elev"].cpu().numpy(), None if c is None else c.cpu().numpy()))
        return out


def test_minecraft_terrain_of_world_pipeline_output(td, models):
    w = td.WorldPipeline.from_models(*models, seed=4242, decoder_tile_size=64, decoder_tile_stride=48, latents_batch_size=16).bind()
    try:
        for s, box in ((1, (-21, 13, 43, 77)), (4, (-41, 29, 87, 157))):
            rec = Recording(w)
            elev, biome = td.minecraft_terrain(rec, *box, scale=s)
            H, W = box[2] - box[0], box[3] - box[1]
            planes = twin.noise_planes(box[0], box[1], H, W)
            want_e, want_b = twin.minecraft_terrain(rec.wins, *box, s, 1.0, w.native_resolution, planes)
            e, b = elev.cpu().numpy(), biome.cpu().numpy()
            assert e.shape == (H, W) and rec.wins[-1][1].shape[0] == 5
            assert (np.array_equal(e, want_e) if s == 1 else ulps(e, want_e) <= 2), s
            if s == 1:
                m = twin.margin(rec.wins[1][0], rec.wins[1][1], twin.gradient(rec.wins[0][0]), w.native_resolution, planes)
            else:
                up = twin.get_upsampled(*rec.wins[0], *box, s, 1.0, w.native_resolution / s, w.native_resolution, planes)
                m = twin.margin(up["elev_smooth"], up["climate"], twin.gradient(up["elev_padded"]), w.native_resolution / s, planes)
            assert np.array_equal(b[m >= 4], want_b[m >= 4]), s
    finally:
        w.close()
