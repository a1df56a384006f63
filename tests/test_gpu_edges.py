"""GPU: edge cases, error behaviour of the C-ABI surface, and size-independent properties at BASELINE sizes."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_rms
from _engine_opts import engine_options_guard, pinned  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    return t


@pytest.fixture(scope="module")
def tiny(td):
    from oracle.unet import synth_state_dict, tiny_config
    cfg = tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(synth_state_dict(cfg, seed=77))
    yield m, cfg
    m.close()


def test_api_misuse_fails_loudly(td, tiny):
    from oracle.unet import synth_state_dict, tiny_config
    from terrain_diffusion_amd._lib import lib
    m, cfg = tiny
    fresh = td.EDMUnet2D(**cfg, dtype="bf16")
    with pytest.raises(RuntimeError):                                   # forward before weights
        fresh(torch.zeros(1, 5, 16, 16), torch.tensor([1.0]), [torch.zeros(1, 58)])
    sd = synth_state_dict(cfg, seed=77)
    bad = dict(sd); bad.pop("out_gain")
    with pytest.raises(KeyError):                                       # missing parameter
        fresh.load_state_dict(bad)
    bad = dict(sd); bad["enc.512x512_conv.weight"] = torch.zeros(64, 6, 3, 2)
    with pytest.raises(ValueError):                                     # wrong shape
        fresh.load_state_dict(bad)
    assert lib().td_unet_set_param(fresh._h, b"no.such.param", None, 0) != 0 and b"unknown parameter" in lib().td_last_error()
    fresh.close()
    with pytest.raises(td.TdError):                                     # H, W must be divisible by 2^(levels-1)
        m(torch.zeros(1, 5, 12, 12).cuda(), torch.tensor([1.0]), [torch.zeros(1, 58).cuda()])
    with pytest.raises(ValueError):                                     # wrong number of conditional inputs
        m(torch.zeros(1, 5, 16, 16).cuda(), torch.tensor([1.0]), [])
    with pytest.raises(NotImplementedError):                            # unsupported constructor options say so
        td.EDMUnet2D(**{**cfg, "fourier_scale": 1})
    with pytest.raises(NotImplementedError):
        td.EDMDPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
    with pytest.raises(td.TdError):                                     # window larger than the noise tile
        td.gaussian_noise_patches(1, [(0, 0)], 65, 64, channels=1, tile_h=64, tile_w=64)
    assert td.gaussian_noise_patches(1, [], 8, 8).shape[0] == 0        # empty batch is a no-op
    assert td.standard_normal(5, (0,)).size == 0


def test_degenerate_sizes(td, tiny):
    """1-step and 2-step schedules, canvas == tile, canvas smaller than 2 tiles, untiled path, batch of 1 window."""
    from oracle import tiling
    from oracle.unet import OracleUnet, synth_state_dict
    m, cfg = tiny
    om = OracleUnet(cfg, synth_state_dict(cfg, seed=77))
    sch = td.EDMDPMSolverMultistepScheduler()
    kw = dict(cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0), histogram_raw=torch.zeros(1, 5))
    for H, W, steps in [(16, 16, 1), (16, 16, 2), (16, 24, 3), (16, 17, 2)]:
        cond = tiling.synthetic_cond_grid(len(tiling.tile_starts(H, 16, 8)), len(tiling.tile_starts(W, 16, 8)))
        y = td.sample_base_diffusion(m, sch, (1, 5, H, W), cond, steps=steps, tile_size=16, noise_seed=3, **kw)
        ref = tiling.sample_base_diffusion_tiled(om, (1, 5, H, W), cond, steps=steps, tile_size=16, noise_seed=3)
        assert y.shape == (1, 5, H, W) and rel_rms(y.cpu().numpy(), ref.numpy()) < 2e-2, (H, W, steps)
    # untiled path returns the raw sample like the reference's `return samples` (sample_diffusion_base.py:113)
    c58 = tiling.process_cond_img(tiling.synthetic_cond_grid(1, 1), torch.zeros(1, 5), torch.zeros(7), torch.ones(7), 0.0)[0]
    y = td.sample_base_diffusion(m, sch, (1, 5, 16, 16), c58, steps=2, tile_size=None, noise_seed=3, **kw)
    assert y.shape == (1, 5, 16, 16) and torch.isfinite(y).all()


def test_determinism_and_seed_sensitivity(td, tiny):
    """same (seed, coordinates) -> bit-identical output on repeat; different seed or origin -> different output; a window's
    result does not depend on where it sits in the batch."""
    m, _ = tiny
    sch = td.EDMDPMSolverMultistepScheduler()
    cond = torch.zeros(3, 58)
    a = td.sample_independent_tiles(m, sch, [(0, 0), (64, 64), (-128, 32)], cond, steps=4, tile_size=16, noise_seed=9)
    b = td.sample_independent_tiles(m, sch, [(0, 0), (64, 64), (-128, 32)], cond, steps=4, tile_size=16, noise_seed=9)
    assert torch.equal(a, b)
    c = td.sample_independent_tiles(m, sch, [(-128, 32), (0, 0), (64, 64)], cond, steps=4, tile_size=16, noise_seed=9)
    assert torch.equal(c[1], a[0]) and torch.equal(c[0], a[2])
    d = td.sample_independent_tiles(m, sch, [(0, 0)], cond[:1], steps=4, tile_size=16, noise_seed=10)
    assert not torch.equal(d[0], a[0])
    assert not torch.equal(a[0], a[1])


def test_noise_field_properties_full_size(td):
    """BASELINE-size noise (5x64x64 per window, 64 windows of an 8x8 grid at stride 32): every overlap agrees bit-for-bit,
    moments are those of N(0,1), and the field is translation-consistent (window at (y,x) == crop of a bigger window)."""
    origins = [(32 * i, 32 * j) for i in range(8) for j in range(8)]
    w = td.gaussian_noise_patches(42 + 5819, origins, 64, 64, channels=5, tile_h=64, tile_w=64)
    g = w.view(8, 8, 5, 64, 64)
    assert torch.equal(g[:, :-1, :, :, 32:], g[:, 1:, :, :, :32]) and torch.equal(g[:-1, :, :, 32:, :], g[1:, :, :, :32, :])
    assert abs(float(w.mean())) < 5e-3 and abs(float(w.std()) - 1.0) < 5e-3
    big = td.gaussian_noise_patches(42 + 5819, [(0, 0)], 64, 64, channels=5, tile_h=64, tile_w=64)
    assert torch.equal(big[0], g[0, 0])
    neg = td.gaussian_noise_patches(7, [(-64, -64), (-32, -32)], 64, 64, channels=2, tile_h=64, tile_w=64)
    assert torch.equal(neg[0][:, 32:, 32:], neg[1][:, :32, :32])


def test_blend_linearity_and_partition_of_unity_full_size(td):
    """overlap blend at BASELINE config-3 size (8x8 windows of 64 on a 288x288 canvas): linear in the tiles, reproduces a constant,
    and the interior weight sum equals the analytic constant (2 - 0.999*32/31.5)^2."""
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.sampling import blend_windows, blend_normalize, _tile_starts
    eng = get_engine("cuda")
    hs = ws = _tile_starts(288, 64, 32)
    idx = [(i, j) for i in range(8) for j in range(8)]
    g = torch.Generator(device="cuda").manual_seed(0)
    A = torch.randn(64, 5, 64, 64, device="cuda", generator=g)
    B = torch.randn(64, 5, 64, 64, device="cuda", generator=g)

    def blend(t):
        c = torch.zeros(6, 288, 288, device="cuda")
        blend_windows(eng, c, t.contiguous(), idx, hs, ws, 64)
        return c
    ca, cb, cab = blend(A), blend(B), blend(2 * A - 3 * B)
    assert torch.allclose(cab[:5], 2 * ca[:5] - 3 * cb[:5], rtol=1e-4, atol=1e-4)
    assert torch.equal(ca[5], cb[5])
    const = (2 - 0.999 * 32 / 31.5) ** 2
    assert torch.allclose(ca[5][32:256, 32:256], torch.full((224, 224), const, device="cuda"), atol=1e-5)
    ones = blend_normalize(eng, blend(torch.ones_like(A)), 1.0)
    assert torch.allclose(ones, torch.ones_like(ones), rtol=1e-6)
    # accumulate in two launches == one launch (weights) and close for values
    c2 = torch.zeros(6, 288, 288, device="cuda")
    blend_windows(eng, c2, A[:32].contiguous(), idx[:32], hs, ws, 64)
    blend_windows(eng, c2, A[32:].contiguous(), idx[32:], hs, ws, 64, accumulate=True)
    assert torch.allclose(c2, ca, rtol=1e-5, atol=1e-5)


def test_unet_linearity_in_out_gain_and_clip_range(td):
    """property of the network maths that does not need the oracle: the output scales linearly with out_gain, and stays finite for
    extreme inputs (activations are clipped at +-256 inside every block)."""
    from oracle.unet import synth_state_dict, tiny_config
    cfg = tiny_config(64, 1)
    sd = synth_state_dict(cfg, seed=5)
    x = torch.randn(1, 5, 16, 16).cuda()
    c = torch.randn(1, 58).cuda()
    outs = []
    for gain in (1.0, 2.5):
        sd["out_gain"] = torch.tensor(gain)
        m = td.EDMUnet2D(**cfg, dtype="fp32").load_state_dict(sd)
        outs.append(m(x, torch.tensor([0.8]), [c]))
        big = m(x * 1e4, torch.tensor([1.5]), [c * 50])
        assert torch.isfinite(big).all()
        m.close()
    assert rel_rms((outs[1] / 2.5).cpu().numpy(), outs[0].cpu().numpy()) < 1e-6


def test_forward_bitwise_repeatable_under_load(td):
    """race detector for the LDS-DMA ring / patch restage protocol: the full-size base U-Net (throughput kernels at every level for
    batch 16) must give bit-identical outputs on 30 back-to-back runs, for both a batch and its permutation."""
    from oracle.unet import BASE_CONFIG, synth_state_dict
    m = td.EDMUnet2D(**BASE_CONFIG, dtype="bf16").load_state_dict(synth_state_dict(BASE_CONFIG, seed=3))
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(16, 5, 64, 64, device="cuda", generator=g)
    c = torch.randn(16, 58, device="cuda", generator=g)
    t = torch.linspace(-1.0, 1.5, 16)
    ref = m(x, t, [c])
    assert torch.isfinite(ref).all()
    for _ in range(30):
        assert torch.equal(m(x, t, [c]), ref)
    perm = torch.arange(15, -1, -1, device="cuda")
    out = m(x[perm].contiguous(), t[perm.cpu()].contiguous(), [c[perm].contiguous()])
    assert torch.equal(out[perm], ref)
    m.close()


def test_producer_side_activation_is_bit_identical(td):
    """plan option producer_act (decoder-block inputs activated once in the producer's epilogue instead of during every patch
    staging of the consumer) must not change a single bit, in bf16 and in fp32 mode."""
    from oracle.unet import synth_state_dict, tiny_config
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    cfg = tiny_config(128, 2)
    sd = synth_state_dict(cfg, seed=11)
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(12, 5, 64, 64, device="cuda", generator=g)
    c = torch.randn(12, 58, device="cuda", generator=g)
    t = torch.linspace(-0.5, 1.5, 12)
    for dtype in ("bf16", "fp32"):
        m = td.EDMUnet2D(**cfg, dtype=dtype).load_state_dict(sd)
        with pinned(eng, producer_act=1):
            a = m(x, t, [c])
        with pinned(eng, producer_act=0):
            b = m(x, t, [c])
        assert torch.equal(a, b), dtype
        m.close()


def test_forward_and_checkpoint_argument_validation(td):
    """noise_labels must have 1 or n entries (the engine reads n of them), x must have in_channels channels, and a checkpoint that lacks a
    parameter is refused even with strict=False (which, as in torch, only tolerates unexpected keys)."""
    from oracle.unet import synth_state_dict, tiny_config
    cfg = tiny_config(64, 1)
    sd = synth_state_dict(cfg, seed=3)
    m = td.EDMUnet2D(**cfg, dtype="fp32")
    short = dict(sd)
    short.pop(next(k for k in sd if k.endswith("conv_res0.weight")))
    with pytest.raises(KeyError):
        m.load_state_dict(short)
    with pytest.raises(ValueError):
        m.load_state_dict(short, strict=False)
    m.load_state_dict({**sd, "some_extra_buffer": torch.zeros(3)}, strict=False)
    x = torch.randn(3, cfg["in_channels"], 64, 64, device="cuda")
    c = torch.randn(3, 58, device="cuda")
    assert m(x, torch.tensor([0.3]), [c]).shape == (3, cfg["out_channels"] if cfg.get("out_channels") else cfg["in_channels"], 64, 64)
    with pytest.raises(ValueError):
        m(x, torch.tensor([0.3, 0.4]), [c])
    with pytest.raises(ValueError):
        m(x[:, :3], torch.tensor([0.3]), [c])
    m.close()


def test_caller_supplied_stream_orders_engine_work_without_host_sync(td):
    """td_engine_set_stream + option "async" (VERDICT round 2 item 8): a producer kernel, the engine's sampler and a consumer kernel
    are enqueued on ONE caller stream without any host synchronisation in between; the result equals the default synchronous path bit for bit.
    A delay kernel in front keeps the stream busy while everything is enqueued, so a missing dependency would read unfinished data."""
    import torch
    from oracle.unet import synth_state_dict, tiny_config
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.sampling import sample_tiles_edm
    eng = get_engine("cuda")
    cfg = tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(synth_state_dict(cfg, seed=77))
    sch = td.EDMDPMSolverMultistepScheduler()
    g = torch.Generator(device="cuda").manual_seed(3)
    base = torch.randn(4, 5, 16, 16, device="cuda", generator=g)
    cond = torch.randn(4, m.cond_row_len if hasattr(m, "cond_row_len") else 58, device="cuda", generator=g)
    sch.set_timesteps(6)
    ref_in = (base * 3.0 + 1.0).contiguous()
    ref = sample_tiles_edm(m, sch, ref_in.clone(), cond, 6) * 0.5
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with pytest.raises(ValueError):
        eng.set_stream(torch.cuda.default_stream())
    big = torch.randn(4096, 4096, device="cuda")
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), eng.on_stream(s):
        for _ in range(20):
            big = big @ big * 1e-3                      # ~ms of queued work ahead of the producer
        x = (base * 3.0 + 1.0).contiguous()             # producer on s
        y = sample_tiles_edm(m, sch, x, cond, 6)        # engine: enqueued on s, returns without waiting
        out = y * 0.5                                   # consumer on s
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert eng.stream != s.cuda_stream                  # the context restored the engine's own stream
    m.close()


def test_unknown_engine_option_is_refused(td):
    """Round-4 review: td_engine_set_option stored any key ("batch_invarient" was accepted and never read -- silently losing the sharded bit-identity)."""
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd._lib import lib
    eng = get_engine("cuda")
    with pytest.raises(RuntimeError, match="unknown engine option"):
        eng.set_option("batch_invarient", 1)            # (the one bare call of the suite: the refusal is what is tested, and nothing is stored)
    assert b"batch_invarient" in lib().td_last_error()
    with pinned(eng, batch_invariant=0):                # the real key is still accepted
        assert eng.get_option("batch_invariant", -1) == 0


def test_on_stream_is_reentrant_and_ordered_behind_the_previous_stream(td):
    """Round-4 advisor: (1) entering on_stream(side) did not order `side` behind torch's previously current stream -- inputs produced there just
    before entry were read unordered (ptr() no longer synchronises once the engine shares torch's current stream); (2) an inner on_stream block
    (the sharded samplers enter one) dropped the caller's stream and enqueue-only mode for the rest of the caller's block."""
    from oracle.unet import synth_state_dict, tiny_config
    from terrain_diffusion_amd.engine import get_engine, engine_on_current_stream
    from terrain_diffusion_amd.sampling import sample_tiles_edm
    eng = get_engine("cuda")
    cfg = tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(synth_state_dict(cfg, seed=77))
    sch = td.EDMDPMSolverMultistepScheduler()
    sch.set_timesteps(6)
    g = torch.Generator(device="cuda").manual_seed(5)
    base = torch.randn(4, 5, 16, 16, device="cuda", generator=g)
    cond = torch.randn(4, 58, device="cuda", generator=g)
    ref = sample_tiles_edm(m, sch, (base * 2.0).contiguous(), cond, 6)
    torch.cuda.synchronize()
    outer, inner = torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.randn(4096, 4096, device="cuda")
    for _ in range(20):
        big = big @ big * 1e-3                          # ~ms of work queued on the DEFAULT stream ...
    x = (base * 2.0).contiguous()                       # ... in front of the producer of the engine's input, still on the default stream
    with eng.on_stream(outer):                          # must wait for the default stream (no host synchronisation in between)
        y = sample_tiles_edm(m, sch, x.clone(), cond, 6)   # (the sampler works in place)
        with eng.on_stream(inner, asynchronous=False):
            assert engine_on_current_stream("cuda") and eng.stream == inner.cuda_stream
            y2 = sample_tiles_edm(m, sch, x.clone(), cond, 6)
        # back in the outer block: the caller's stream and enqueue-only mode are restored
        assert eng.stream == outer.cuda_stream and engine_on_current_stream("cuda") and eng._async
        y3 = sample_tiles_edm(m, sch, x.clone(), cond, 6)
    torch.cuda.synchronize()
    assert eng.stream not in (outer.cuda_stream, inner.cuda_stream) and not eng._async
    assert torch.equal(y, ref) and torch.equal(y2, ref) and torch.equal(y3, ref)
    m.close()


def test_pano_denoise_ddim_cfg_step_vs_oracle(td):
    """BASELINE configs[0] (annotated_infinite_panorama.py:125-134): the classifier-free-guidance mix + DDIM update on the engine
    (td_ddim_cfg_step, driven by pano.denoise with a stand-in denoiser -- SD-v1.5's UNet2DCondition is third-party) against oracle/ddim.py's
    restatement of the published algorithm, 4 steps on 2 tiles' worth of 64x64 latents as configs[0] words it.  The DDIM arithmetic itself is
    unpinned (diffusers absent; oracle/ddim.py header); this pins the HIP kernel to the restatement: <= 2 ulp-level fp32 differences."""
    import torch
    from oracle import ddim, rng
    from terrain_diffusion_amd import pano
    sch = pano.DDIMSchedule().set_timesteps(4)
    # (torch.cumprod and np.cumprod round the 1000-term fp32 product differently in the last place)
    assert sch.timesteps.tolist() == list(ddim.timesteps(4)) and np.allclose(sch.alphas_cumprod.numpy(), ddim.alphas_cumprod(), rtol=2e-6, atol=0)
    lat = rng.standard_normal(81, (1, 4, 64, 128)).astype(np.float32)       # two 64x64 latent tiles side by side

    def stub_np(inp, t):   # a deterministic "U-Net": mixes the input with a timestep-dependent field, different for the two CFG halves
        f = np.float32(np.sin(0.01 * t))
        return np.concatenate([inp[:1] * np.float32(0.3) + f, inp[1:] * np.float32(0.35) - f * np.float32(0.5)]).astype(np.float32)
    ref = ddim.denoise(lat, ddim.timesteps(4), 4, stub_np, guidance_scale=7.5, acp=sch.alphas_cumprod.numpy())
    got = pano.denoise(torch.from_numpy(lat), sch.timesteps, lambda inp, t: torch.from_numpy(stub_np(inp.cpu().numpy(), int(t))), sch, guidance_scale=7.5)
    err = rel_rms(got.cpu().numpy(), ref)
    print(f"pano.denoise (4 DDIM steps, CFG 7.5) vs oracle/ddim.py: rel-RMS {err:.2e}")
    assert err < 2e-6


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_solver_step_fused_into_output_conv_is_bit_identical(td, dtype):
    """north_star: 'the per-tile EDM scheduler step ... fused into the epilogue'.  With engine option fuse_solver (default on) the DPM-Solver++ update
    and the next step's input preconditioning run in the epilogue of the U-Net's output conv (EPI_DPM_STEP) instead of a separate pass over F;
    the arithmetic and its order are the separate kernel's, so 12 steps of the tiled sampler agree BIT FOR BIT with fuse_solver = 0 (which the
    autoguided sampler still uses: its update needs both models' outputs)."""
    import torch
    from oracle import tiling
    from oracle.unet import synth_state_dict, tiny_config
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    cfg = tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype=dtype).load_state_dict(synth_state_dict(cfg, seed=77))
    sch = td.EDMDPMSolverMultistepScheduler()
    cond = tiling.synthetic_cond_grid(4, 2)
    kw = dict(cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0), histogram_raw=torch.zeros(1, 5), steps=12, tile_size=16, noise_seed=3)
    outs = {}
    for f in (1, 0):
        with pinned(eng, fuse_solver=f):
            outs[f] = td.sample_base_diffusion(m, sch, (1, 5, 40, 24), cond, **kw).clone()
    assert torch.isfinite(outs[1]).all() and torch.equal(outs[1], outs[0])
    m.close()


def test_third_order_solver_on_engine(td):
    """solver_order = 3 (dpmsolver.py:563-615) through the engine: the tiled sampler in fp32 mode against the oracle's tiled sampler (whose scheduler
    restatement is pinned to traces of the reference scheduler, tests/golden/schedule3.npz), 6 steps (order trace 1,2,3,3,2,1: lower_order_second)
    and 16 steps; the fused output-conv epilogue and the separate solver kernel agree bit for bit."""
    import torch
    from oracle import tiling
    from oracle.unet import OracleUnet, synth_state_dict, tiny_config
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    cfg = tiny_config(64, 1)
    sd = synth_state_dict(cfg, seed=77)
    m = td.EDMUnet2D(**cfg, dtype="fp32").load_state_dict(sd)
    om = OracleUnet(cfg, sd)
    sch = td.EDMDPMSolverMultistepScheduler(solver_order=3)
    cond = tiling.synthetic_cond_grid(3, 3)
    kw = dict(cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0), histogram_raw=torch.zeros(1, 5), tile_size=16, noise_seed=11)
    for steps in (6, 16):
        got = td.sample_base_diffusion(m, sch, (1, 5, 32, 32), cond, steps=steps, **kw).clone()
        ref = tiling.sample_base_diffusion_tiled(om, (1, 5, 32, 32), cond, steps=steps, tile_size=16, noise_seed=11, solver_order=3)
        err = rel_rms(got.cpu().numpy(), ref.numpy())
        print(f"third-order DPM-Solver++, {steps} steps, fp32 engine vs oracle: {err:.2e}")
        assert err < 1e-5
        assert eng.get_option("solver_order", 2) == 2             # the sampler put back what it found: the scheduler's order is the call's, not the engine's
        with pinned(eng, fuse_solver=0):
            unfused = td.sample_base_diffusion(m, sch, (1, 5, 32, 32), cond, steps=steps, **kw)
        assert torch.equal(got, unfused)
    second = td.sample_base_diffusion(m, td.EDMDPMSolverMultistepScheduler(solver_order=2), (1, 5, 32, 32), cond, steps=16, **kw)
    assert not torch.equal(second, got)                       # the order really changed the trajectory
    m.close()
