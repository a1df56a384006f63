"""GPU: one window batch of the grid sampler as one engine call (td_sample_grid_batch) and the conditioning rows on the GPU (td_cond_rows).
Everything here is bit-exact: the rows against the per-window host path (_process_cond_img on a (1,7,4,4) patch), the fused call against the
four separate calls it replaces (engine option grid_fused = 0), and the old exports against what the fused call used."""
import numpy as np
import pytest
import torch

from _engine_opts import engine_options_guard, pinned  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu

MEANS = torch.tensor([0.31, -0.27, 1.9, -0.6, 0.05, 2.4, -1.1])
STDS = torch.tensor([0.5, 1.5, 0.75, 1.25, 0.9, 1.1, 0.6])
HIST = torch.tensor([[0.11, -0.42, 0.93, 0.27, -0.08]])
NOISE_LEVEL = 0.3


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as td
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return td


@pytest.fixture(scope="module")
def eng(td):
    from terrain_diffusion_amd.engine import get_engine
    return get_engine("cuda")


def _rows_grid():
    """(1,7,6,7): 3 x 4 window positions; one NaN cell, window (2,3)'s climate 2x2 all NaN in channels 2..5, one +inf, one -inf"""
    from oracle import rng
    g = torch.from_numpy(rng.standard_normal(4242, (1, 7, 6, 7))).clone()
    g[0, 0, 1, 2] = float("nan")
    g[0, 2:6, 3:5, 4:6] = float("nan")
    g[0, 1, 4, 1] = float("inf")
    g[0, 6, 2, 5] = float("-inf")
    return g


def _host_rows(td, grid, pos):
    from terrain_diffusion_amd.sampling import _process_cond_img
    return torch.cat([_process_cond_img(grid[..., i:i + 4, j:j + 4].cpu(), HIST, MEANS, STDS, NOISE_LEVEL) for i, j in pos])


@pytest.mark.parametrize("where", ["host", "device"])
def test_cond_rows_bit_exact(td, eng, where):
    from terrain_diffusion_amd.sampling import cond_rows
    grid = _rows_grid()
    pos = [(i, j) for i in range(3) for j in range(4)]
    order = np.random.default_rng(5).permutation(12)
    pos = [pos[k] for k in order] + [pos[order[3]]]          # 13 positions, shuffled, one repeated
    assert (2, 3) in pos and len(pos) == 13
    ref = _host_rows(td, grid, pos)
    got = cond_rows(eng, grid.cuda() if where == "device" else grid, pos, HIST, MEANS, STDS, NOISE_LEVEL)
    assert got.is_cuda and got.shape == (13, 58) and ref.shape == (13, 58)
    assert torch.isfinite(ref).all()
    assert torch.equal(got.cpu(), ref), int((got.cpu() != ref).sum())


def test_cond_rows_one_window(td, eng):
    from terrain_diffusion_amd.sampling import cond_rows
    grid = _rows_grid()
    got = cond_rows(eng, grid, [(2, 3)], HIST, MEANS, STDS, NOISE_LEVEL)
    assert torch.equal(got.cpu(), _host_rows(td, grid, [(2, 3)]))


@pytest.fixture(scope="module")
def model(td):
    from oracle.unet import synth_state_dict, tiny_config
    cfg = tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype="bf16")
    m.load_state_dict(synth_state_dict(cfg, seed=77))
    yield m
    m.close()


def _both_arms(td, eng, model, cond, shape=(1, 5, 48, 48), options=None, **kw):
    """sample_base_diffusion with grid_fused = 1 and = 0 under `options`; every option goes back to what it was"""
    sch = td.EDMDPMSolverMultistepScheduler()
    stats = dict(cond_means=MEANS, cond_stds=STDS, noise_level=torch.tensor(NOISE_LEVEL), histogram_raw=HIST)
    outs = []
    with pinned(eng, **(options or {})):
        for fused in (1, 0):
            with pinned(eng, grid_fused=fused):
                outs.append(td.sample_base_diffusion(model, sch, shape, cond, steps=3, return_windows=kw.get("tile_size", 32) is not None,
                                                     **{"tile_size": 32, **stats, **kw}))
    return outs


def _assert_same(a, b):
    if isinstance(a, tuple):
        (ca, wa), (cb, wb) = a, b
        assert sorted(wa) == sorted(wb) and len(wa) > 0
        for t in wa:
            assert torch.equal(wa[t], wb[t]), t
        a, b = ca, cb
    assert a.shape == b.shape and torch.isfinite(a).all()
    assert torch.equal(a, b)


def _grid():
    from oracle import tiling
    return tiling.synthetic_cond_grid(2, 2)          # (1,7,5,5): 2 x 2 windows of 32 on a 48 x 48 canvas


def test_fused_defaults(td, eng, model):
    a, b = _both_arms(td, eng, model, _grid())
    assert len(a[1]) == 4
    _assert_same(a, b)


def test_fused_chunks_straddling_noise_tiles(td, eng, model):
    a, b = _both_arms(td, eng, model, _grid(), max_batch=3, noise_origin=(-40, 12296), return_canvas=True)
    assert a[0].shape == (6, 48, 48) and len(a[1]) == 4
    _assert_same(a, b)


def test_fused_tile_subset(td, eng, model):
    # the accumulator canvas: without window (0, 0) the top-left corner has weight 0, and the normalised canvas is 0 / 0 = NaN there in either arm
    a, b = _both_arms(td, eng, model, _grid().cuda(), tiles=[(0, 1), (1, 0), (1, 1)], return_canvas=True)
    assert sorted(a[1]) == [(0, 1), (1, 0), (1, 1)] and float(a[0][5, 0, 0]) == 0.0 and float(a[0][5, 40, 40]) > 0.0
    _assert_same(a, b)


def test_fused_two_lanes(td, eng, model):
    """the two-lane branch of td_sample_grid_batch (dual_stream = 1 and a batch of at least dual_stream_min_batch windows) against the four calls, which split
    the same way in td_sample_edm_img: both options are pinned here, whatever the engine ships with, and the batch is checked to reach the threshold"""
    with pinned(eng, dual_stream=1, dual_stream_min_batch=2):
        from terrain_diffusion_amd.geometry import tile_starts
        n_windows = len(tile_starts(48, 32, 16)) ** 2                  # one batch (max_batch = 64) of the 48 x 48 canvas' windows
        assert eng.get_option("dual_stream", -1) == 1 and eng.get_option("dual_stream_min_batch", -1) == 2 and n_windows == 4 >= 2
        assert n_windows >= max(2, eng.get_option("dual_stream_min_batch", -1))      # the engine's own condition for two lanes
        a, b = _both_arms(td, eng, model, _grid())
        assert eng.get_option("dual_stream", -1) == 1 and eng.get_option("dual_stream_min_batch", -1) == 2    # (still, after both arms)
    assert len(a[1]) == len(b[1]) == n_windows                     # lanes of 2 and 2 windows
    _assert_same(a, b)


def test_fused_single_window_row(td, eng, model):
    from oracle import rng
    row = torch.from_numpy(rng.standard_normal(99, (58,)))
    a, b = _both_arms(td, eng, model, row, shape=(1, 5, 32, 32), tile_size=None)
    assert a.shape == (1, 5, 32, 32)
    _assert_same(a, b)


def test_old_exports_match_what_the_fused_call_used(td, eng, model):
    """gaussian_noise_patches and blend_windows on the inputs of the chunked, straddling case: after 0 solver steps (sampler_stop_after = 0) the
    fused call's pre-blend windows ARE its initial noise, and its canvas is the blend of exactly those windows"""
    from terrain_diffusion_amd import noise as _noise
    from terrain_diffusion_amd.sampling import blend_windows
    sch = td.EDMDPMSolverMultistepScheduler()
    sch.set_timesteps(3)
    with pinned(eng, sampler_stop_after=0):
        canvas, wins = td.sample_base_diffusion(model, sch, (1, 5, 48, 48), _grid(), steps=3, tile_size=32, max_batch=3, noise_origin=(-40, 12296),
                                                return_canvas=True, return_windows=True, cond_means=MEANS, cond_stds=STDS,
                                                noise_level=torch.tensor(NOISE_LEVEL), histogram_raw=HIST)
    tiles = [(0, 0), (0, 1), (1, 0), (1, 1)]
    starts = [0, 16]
    x = _noise.gaussian_noise_patches(42 + 5819, [(-40 + starts[i], 12296 + starts[j]) for i, j in tiles], 32, 32, channels=5, tile_h=64, tile_w=64,
                                      scale=float(sch.sigmas[0]))
    for k, t in enumerate(tiles):
        assert torch.equal(wins[t], x[k]), t
    ref = torch.zeros((6, 48, 48), device=x.device)
    blend_windows(eng, ref, x[:3].contiguous(), tiles[:3], starts, starts, 32, accumulate=True)
    blend_windows(eng, ref, x[3:].contiguous(), tiles[3:], starts, starts, 32, accumulate=True)
    assert torch.equal(canvas, ref)
