"""The tiling and composition kernels on the MI355X, element by element, against their float64 twins (tests/_tile_twin.py).

Every committed case of every op goes through its C entry point (td_blend_windows, td_gather_regions, td_blend_normalize, td_resample2d, td_residual_plus,
td_elev_finish, td_climate_finish, td_ddim_cfg_step) on fp32 tensors the twin file makes, and is held to criterion A on every element, criterion B, the cap on the
bound's median and the non-finite rule.  One printed line per case.  Beside them: the weight window bit for bit, host and device tile pointers, the regions kernel bit
for bit against the blend kernel where 16 terms are live, the in-place DDIM step, every refusal as an error, and the noise windows on tiles that are no powers of two."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tile_twin as tw
from _engine_opts import engine_options_guard  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def eng(td):
    from terrain_diffusion_amd.engine import get_engine
    return get_engine("cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _blend(eng, cs, tiles, wi, wj, accumulate, prior, host_tiles=False):
    from terrain_diffusion_amd.sampling import blend_windows
    canvas = dev(prior) if accumulate else torch.full((cs["C"] + 1, cs["Hc"], cs["Wc"]), 777.0, device="cuda")      # without accumulate what the canvas held is ignored
    t = torch.from_numpy(np.ascontiguousarray(tiles))
    blend_windows(eng, canvas, t if host_tiles else t.cuda(), list(zip(wi, wj)), cs["rows"], cs["cols"], cs["size"], accumulate=bool(accumulate))
    torch.cuda.synchronize()
    return canvas.cpu().numpy()


def _regions(eng, cs):
    from terrain_diffusion_amd._lib import lib, check
    from terrain_diffusion_amd.engine import ptr
    wins = [dev(w) for w in cs["wins"]]
    ptrs = np.asarray([t.data_ptr() for t in wins], dtype=np.uint64)
    desc = np.ascontiguousarray(cs["desc"], dtype=np.int32)
    n, maxk = desc.shape[:2]
    out = torch.full((n, cs["C"] + 1, cs["h"], cs["w"]), 777.0, device="cuda")
    check(lib().td_gather_regions(eng._h, cs["C"], cs["size"], n, cs["h"], cs["w"], maxk, C.c_void_p(desc.ctypes.data), len(wins), C.c_void_p(ptrs.ctypes.data), ptr(out)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run(eng, op, name, cs, **kw):
    """the engine's answer to one case, in the signature tests/_tile_twin.py's all_cases calls"""
    from terrain_diffusion_amd import composition, sampling
    from terrain_diffusion_amd._lib import lib, check
    from terrain_diffusion_amd.engine import ptr
    if op == "blend":
        return _blend(eng, cs, kw["tiles"], kw["wi"], kw["wj"], kw["accumulate"], kw["prior"])
    if op == "regions":
        return _regions(eng, cs)
    if op == "normalise":
        return sampling.blend_normalize(eng, dev(cs["canvas"]), cs["scale"]).cpu().numpy()
    if op == "resample":
        return composition.resample(eng, dev(cs["x"]), cs["ty"], cs["tx"]).cpu().numpy()
    if op in ("residual_plus", "elev_finish"):
        packed, low = dev(cs["packed"]), dev(cs["low"])
        Hp, Wp = cs["low"].shape
        if op == "residual_plus":
            out = torch.full((Hp, Wp), 777.0, device="cuda")
            check(lib().td_residual_plus(eng._h, ptr(packed), ptr(low), Hp, Wp, float(cs["mean"]), float(cs["std"]), ptr(out)))
        else:
            oi, oj, h, w = kw["crop"]
            out = torch.full((h, w), 777.0, device="cuda")
            check(lib().td_elev_finish(eng._h, ptr(packed), ptr(low), Hp, Wp, oi, oj, h, w, float(cs["mean"]), float(cs["std"]), ptr(out)))
        torch.cuda.synchronize()
        return out.cpu().numpy()
    if op == "climate":
        feats, elev = dev(cs["feats"]), dev(cs["elev"])
        out = torch.full((5, cs["h"], cs["w"]), 777.0, device="cuda")
        check(lib().td_climate_finish(eng._h, ptr(feats), cs["Hs"], cs["Ws"], ptr(elev), cs["i1"], cs["j1"], cs["h"], cs["w"], float(cs["S"]), cs["ci1"], cs["cj1"], ptr(out)))
        torch.cuda.synchronize()
        return out.cpu().numpy()
    if op == "ddim":
        return _ddim(eng, cs, in_place=False)
    raise KeyError(op)


def _ddim(eng, cs, in_place):
    from terrain_diffusion_amd._lib import lib, check
    from terrain_diffusion_amd.engine import ptr
    x, un, co = dev(cs["x"]), dev(cs["uncond"]), dev(cs["cond"])
    out = x if in_place else torch.full_like(x, 777.0)
    check(lib().td_ddim_cfg_step(eng._h, ptr(x), ptr(un), ptr(co), x.numel(), float(cs["g"]), float(np.float32(cs["alpha_t"])), float(np.float32(cs["alpha_prev"])), ptr(out)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def results(eng):
    """every committed case once: {op: [(name, shape, figures, got)]}; the twin's references are computed here, once, and shared"""
    res = {}
    for op, name, shape, got, ref, E in tw.all_cases(lambda op, name, cs, **kw: run(eng, op, name, cs, **kw)):
        res.setdefault(op, []).append((name, shape, tw.judge(got, ref, E), got))
    return res


N_CASES = {"blend": 9, "regions": 3, "normalise": 5, "resample": 12, "residual_plus": 2, "elev_finish": 10, "climate": 10, "ddim": 8}


@pytest.mark.parametrize("op", tw.OPS)
def test_every_case_elementwise(results, op):
    assert len(results[op]) == N_CASES[op]                      # every committed case ran, nothing skipped
    bad = []
    print()
    for name, shape, st, got in results[op]:
        print(tw.line(op, name, "x".join(str(s) for s in shape), st))
        assert st["elements"] == int(np.prod(shape))
        bad += [f"{name}: {v}" for v in tw.verdict(op, st)]
        if name.startswith("zero-weight taps"):
            assert np.all(np.isfinite(got)), name                # inf / NaN under a zero weight never reaches the sum
    assert not bad, "\n".join(bad)


def test_cases_with_non_finite_values_are_the_ones_that_say_so(results):
    for op in tw.OPS:
        for name, shape, st, got in results[op]:
            assert (st["excluded"] > 0) == name.startswith("uncovered pixels"), (op, name, st["excluded"])


# ------------------------------------------------------------------------------------------------------------------ exact properties
def test_weight_window_is_the_twins_bit_for_bit(eng):
    from terrain_diffusion_amd.sampling import _linear_weight_window
    for size in (2, 5, 8, 16, 64):
        assert np.array_equal(_linear_weight_window(size)[0, 0].cpu().numpy(), tw.weight_window(size)), size


def test_host_and_device_tile_pointers_give_the_same_bits(eng):
    for name in ("regular size 16 stride 8, 40x40, C 5", "overhang on all four sides, size 8, 11x13, C 2"):
        cs = tw.blend_cases()[name]
        wi, wj = [g[0] for g in cs["grid"]], [g[1] for g in cs["grid"]]
        a = _blend(eng, cs, cs["tiles"], wi, wj, 0, None, host_tiles=False)
        b = _blend(eng, cs, cs["tiles"], wi, wj, 0, None, host_tiles=True)
        assert np.array_equal(a, b), name


def test_regions_kernel_is_bit_identical_to_the_blend_kernel_with_16_live_terms(eng):
    b = tw.blend_cases()["stride size/4: 16 live terms, size 16, 28x28, C 7"]
    r = tw.regions_cases()["the stride size/4 blend geometry as one region, 28x28, maxk 16"]
    wi, wj = [g[0] for g in b["grid"]], [g[1] for g in b["grid"]]
    blend = _blend(eng, b, b["tiles"], wi, wj, 0, None)
    reg = _regions(eng, r)[0]
    live = tw.blend_ref(b["tiles"], 7, 28, 28, 16, b["rows"], b["cols"], wi, wj)[0]
    assert int(np.count_nonzero(reg != blend)) == 0 and np.all(np.isfinite(blend))
    inner = np.zeros((28, 28), bool)
    inner[12:16, 12:16] = True                                    # rows and columns 12 .. 15 lie in all four windows of their axis
    assert np.all(live[7][inner] > 0) and blend.shape == (8, 28, 28)


def test_ddim_step_in_place_is_bit_identical(eng):
    """pano.denoise passes the latent as `out`: both kernel parameters are __restrict__, each thread reads its element before it writes it"""
    for name, cs in tw.ddim_cases().items():
        assert np.array_equal(_ddim(eng, cs, in_place=True), _ddim(eng, cs, in_place=False)), name


# ------------------------------------------------------------------------------------------------------------------ refusals: errors, not crashes
def test_refusals(td, eng):
    from terrain_diffusion_amd import composition, sampling
    from terrain_diffusion_amd._lib import TdError, lib, check
    from terrain_diffusion_amd.engine import ptr
    z = lambda *s: torch.zeros(s, device="cuda")
    with pytest.raises(TdError):                                  # C = 8
        sampling.blend_windows(eng, z(9, 8, 8), z(1, 8, 4, 4), [(0, 0)], [0], [0], 4)
    with pytest.raises(TdError):                                  # a fifth covering window
        sampling.blend_windows(eng, z(2, 12, 12), z(5, 1, 8, 8), [(i, 0) for i in range(5)], [0, 1, 2, 3, 4], [0], 8)
    with pytest.raises(TdError):
        sampling.blend_windows(eng, z(2, 12, 12), z(5, 1, 8, 8), [(0, i) for i in range(5)], [0], [0, 1, 2, 3, 4], 8)
    with pytest.raises(TdError):                                  # window index out of range
        sampling.blend_windows(eng, z(2, 12, 12), z(1, 1, 8, 8), [(2, 0)], [0, 4], [0, 4], 8)
    with pytest.raises(TdError):
        sampling.blend_windows(eng, z(2, 12, 12), z(1, 1, 8, 8), [(0, -1)], [0, 4], [0, 4], 8)
    bad = dict(C=1, size=4, h=4, w=4, wins=[np.zeros((1, 4, 4), np.float32)], desc=np.array([[[1, 0, 0]]], np.int32))
    with pytest.raises(TdError):                                  # slot >= n_windows
        _regions(eng, bad)
    x = z(1, 4, 5)
    iy, wy = tw.identity_taps(4)
    ix, wx = tw.identity_taps(5)
    for t in (5, -1):
        b = ix.copy()
        b[2, 0] = t
        with pytest.raises(TdError):                              # a column tap out of range
            composition.resample(eng, x, (iy, wy), (b, wx))
        b = iy.copy()
        b[1, 0] = t - 1 if t > 0 else t
        with pytest.raises(TdError):
            composition.resample(eng, x, (b, wy), (ix, wx))
    p, low, out = z(2, 19, 23), z(19, 23), z(10, 23)
    for oi, oj, h, w in ((10, 0, 10, 23), (0, 1, 10, 23), (-1, 0, 10, 23), (0, -1, 10, 22)):
        with pytest.raises(TdError):                              # a crop outside the window
            check(lib().td_elev_finish(eng._h, ptr(p), ptr(low), 19, 23, oi, oj, h, w, 0.0, 1.0, ptr(out)))
    v = z(16)
    for a, pr in ((0.0, 0.5), (1.5, 0.5), (0.5, 0.0), (0.5, 1.0000001), (float("nan"), 0.5), (-0.1, 0.5)):
        with pytest.raises(TdError):                              # alpha outside (0, 1]
            check(lib().td_ddim_cfg_step(eng._h, ptr(v), ptr(v), ptr(v), 16, 7.5, a, pr, ptr(z(16))))
    torch.cuda.synchronize()
    assert float(z(1).sum()) == 0.0                               # the device still answers


# ------------------------------------------------------------------------------------------------------------------ noise windows on tiles that are no powers of two
@pytest.mark.parametrize("tile_h,tile_w,channels", [(24, 40, 1), (24, 40, 5), (7, 5, 1), (7, 5, 5)])
def test_noise_windows_on_tiles_that_are_no_powers_of_two(td, tile_h, tile_w, channels):
    """every other noise-patch case of the suite uses 8, 16, 32 or 64, where the floor division of noise_gather_kernel and a bit mask cannot be told apart"""
    from oracle import rng
    seed = 4242 + tile_h
    for h, w in ((tile_h, tile_w), (tile_h, max(1, tile_w - 2)), (max(1, tile_h // 2), tile_w), (3, 2)):
        origins = [(0, 0), (-1, -1), (-tile_h, -tile_w), (-tile_h + 1, -tile_w - 1), (-3, 2), (5, -4), (tile_h - 1, tile_w - 1), (-tile_h - 5, 3 * tile_w + 1), (-3, 2),
                   (2 * tile_h, -2 * tile_w), (-2 * tile_h - 1, 2 * tile_w - 1), (1000 * tile_h + 3, -1000 * tile_w - 2)]
        got = td.gaussian_noise_patches(seed, origins, h, w, channels=channels, tile_h=tile_h, tile_w=tile_w, scale=80.0).cpu().numpy()
        ref = np.stack([rng.gaussian_noise_patch(seed, y, x, h, w, channels, tile_h, tile_w) for y, x in origins]).astype(np.float32) * np.float32(80.0)
        d = int(np.count_nonzero(got != ref))
        assert got.shape == ref.shape and d == 0, (h, w, d)
    print(f"\nnoise windows, tile {tile_h}x{tile_w}, {channels} channels, scale 80: 4 window sizes x {len(origins)} origins bit-exact")
