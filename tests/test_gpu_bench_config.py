"""The BENCHMARK configuration under parity.

The driver line is BASELINE configs[2]: the full-size 30m base U-Net, 64 overlapping 64x64 windows batched per solver step, bf16.  At that
batch the plan picks the 8-wave "big" conv tile variants, which no batch-1 test ever reaches.  These tests
  (a) run the base model at batch 64 and compare four samples of the batch with the oracle,
  (b) force every legal conv tile shape / flavour (big, small, narrow, bn 96 / 128) through the base model and
      assert they agree BIT FOR BIT with each other, layer by layer (same K order, same MFMA -- DESIGN.md's claim),
  (c) run configs[2] end to end (8x8 grid, 20 steps) and compare four windows before the blend with the oracle plus the blended
      canvas with an independent blend of the engine's own windows.
Tolerances: bf16 <= 2e-2 rel-RMS against the fp32 oracle (the reference's own bf16-vs-fp32 is 1.0e-2 per forward, 1.5e-2 after 20 steps).
"""
import numpy as np
import pytest
import torch

from conftest import rel_rms
from _engine_opts import engine_options_guard, pinned  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def base(td):
    from oracle.unet import BASE_CONFIG, OracleUnet, synth_state_dict
    cfg = dict(BASE_CONFIG)
    sd = synth_state_dict(cfg, seed=1234)
    m = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(sd)
    yield m, OracleUnet(cfg, sd)
    m.close()


def _batch_inputs(n, seed=5):
    from oracle import rng
    x = torch.from_numpy(rng.standard_normal(seed, (n, 5, 64, 64)))
    c = torch.from_numpy(rng.standard_normal(seed + 1, (n, 58)))
    return x, c


def test_base_forward_batch64_vs_oracle(td, base):
    """(a) one forward at the bench batch size; samples 0, 21, 42, 63 against the oracle; the profile dump proves the big tile variants ran."""
    from terrain_diffusion_amd.engine import get_engine
    m, om = base
    eng = get_engine("cuda")
    x, c = _batch_inputs(64)
    t = torch.full((64,), 1.1)
    with pinned(eng, profile=1):
        eng.profile_read(reset=True)
        try:
            y = m(x.cuda(), t, [c.cuda()])
            labels = [l for l, _, _ in eng.profile_ops()]
        finally:
            eng.profile_read(reset=True)
    assert any(" f2b " in l for l in labels), "the 8-wave big tile variant did not run at batch 64"
    # both cout tilings and both wave counts of the LDS-DMA flavour are exercised at this batch size (which layer gets which is the plan's choice)
    assert any("bn128" in l and " f2" in l for l in labels) and any("bn96" in l and " f2b " in l for l in labels) and any(" f2s " in l for l in labels), labels[:5]
    pick = [0, 21, 42, 63]
    with torch.no_grad():
        ref = om(x[pick], t[pick], [c[pick]])
    errs = [rel_rms(y[i].cpu().numpy(), ref[k].numpy()) for k, i in enumerate(pick)]
    print("batch-64 base forward, bf16 vs oracle, samples 0/21/42/63:", ["%.3e" % e for e in errs])
    assert max(errs) < 2e-2, errs


# in network order, so that the first mismatch names the layer that diverged
LAYERS = ["enc.512x512_conv", "enc.512x512_block0.conv_res0", "enc.512x512_block0.conv_res1", "enc.512x512_block2.conv_res1", "enc.256x256_down.conv_res1",
          "enc.256x256_block0.conv_skip", "enc.256x256_block1.conv_res0", "enc.256x256_block2.conv_res1", "enc.128x128_block0.conv_res1",
          "enc.128x128_block2.conv_res1", "enc.64x64_block0.conv_res0", "enc.64x64_block2.conv_res1", "dec.64x64_in0.conv_res1", "dec.64x64_block0.conv_res1",
          "dec.128x128_up.conv_res1", "dec.128x128_block1.conv_res0", "dec.256x256_up.conv_res1", "dec.256x256_block2.conv_res1", "dec.512x512_up.conv_res0",
          "dec.512x512_block3.conv_res1"]


def _forward_with(eng, m, x, t, c, n, **opts):
    # the arms of these tests compare tile shapes of the LDS-DMA conv (conv_glds): the small-batch flavour (round 4, conv_sb.hip -- its own tile
    # hooks are sb_mt / sb_nt, tests/test_gpu_small_batch.py) would otherwise take the small grids of a batch <= 8 whatever the glds_* hooks say
    # (and the wide tile of round 6, conv_glds_wide.hip -- another K order, compared with a tolerance in test_wide_tile_*  -- would take the 64x64 /
    # 32x32 levels of a 64-window batch)
    opts = dict(opts, sb=opts.get("sb", 0), glds_wide=opts.get("glds_wide", 0))
    with pinned(eng, **opts):
        with pinned(eng, profile=1):
            eng.profile_read(reset=True)
            y = m(x, t, [c])
            labels = [l for l, _, _ in eng.profile_ops()]
            eng.profile_read(reset=True)
        acts = {l: m.read_activation(n, 64, 64, l, max_elems=n * 384 * 64 * 64) for l in LAYERS}
        return y, acts, labels


@pytest.mark.parametrize("n", [64, 8])
def test_conv_tile_variants_bit_identical(td, base, n):
    """(b) every legal tile shape of the LDS-DMA conv (8 waves x 256 px / 4 waves x 128 px, 16-wide and the narrow 8x8 x 4 / x 2 image
    tiles, couts in 96s / 128s) accumulates every output in the same K order with the same MFMA:
    the outputs of the whole network and of eight layers spread over the four resolution levels must be bit-identical.  That includes the
    pixel-norm statistic: sums of squares are kept per 32-cout MFMA block, so the consumer adds the same partials in the same order whatever
    tile shape produced them (round 2: they used to be kept per cout tile, which made bn 96 and bn 128 differ in the last bits).  Split-K
    (the one thing that changes the summation order of a conv) is switched off in every arm."""
    from terrain_diffusion_amd.engine import get_engine
    m, _ = base
    eng = get_engine("cuda")
    x, c = _batch_inputs(n, seed=9)
    x, c = x.cuda(), c.cuda()
    t = torch.full((n,), 0.7)
    arms = {"auto": dict(glds_splitk=0), "big": dict(glds_splitk=0, glds_variant=0), "small": dict(glds_splitk=0, glds_variant=1),
            "big/bn96": dict(glds_splitk=0, glds_variant=0, glds_bn=96), "small/bn128": dict(glds_splitk=0, glds_variant=1, glds_bn=128),
            # round 3: 1x1 K-segments (the decoder's fused skip convs) are streamed by LDS-DMA; the register-staged path is the other arm
            "reg1x1": dict(glds_splitk=0, glds_dma1x1=0), "reg1x1/big": dict(glds_splitk=0, glds_dma1x1=0, glds_variant=0),
            "reg1x1/small/bn128": dict(glds_splitk=0, glds_dma1x1=0, glds_variant=1, glds_bn=128)}
    res = {k: _forward_with(eng, m, x, t, c, n, **o) for k, o in arms.items()}
    seen = {k: {tag for l in res[k][2] for tag in (" f2b ", " f2s ", "bn96", "bn128") if tag in l} for k in res}
    assert " f2b " in seen["big"] and " f2s " in seen["small"], seen
    assert all(" f2s " not in l for l in res["big"][2] if "8x8" in l and " f2" in l), "narrow big variant <8,8,4,...> must run in the 'big' arm"
    y0, a0, _ = res["auto"]
    assert torch.isfinite(y0).all() and float(y0.abs().mean()) > 1e-3
    for k, (y, acts, labels) in res.items():
        for l in LAYERS:
            how = [q for q in labels if q.startswith(l + " ")] + [q for q in res["auto"][2] if q.startswith(l + " ")]
            assert torch.equal(acts[l], a0[l]), (k, l, float((acts[l] - a0[l]).abs().max()), how)
        assert torch.equal(y, y0), (k, float((y - y0).abs().max()))


@pytest.mark.parametrize("out_channels", [1, 2, 3])
def test_fewcout_output_conv_against_the_mfma_tile(td, out_channels):
    """Round 6: the decoder model's 64 -> 1 output conv (and the same network with 2 / 3 output channels: the flavour's two other instantiations) on the VALU flavour (conv_fewcout.hip: one pixel per thread, fp32 multiply-adds, no 64-cout MFMA tile
    for one cout) against the same network with the flavour off (engine option fewcout = 0: conv_glds's tile).  Same products, fp32 sums in another order:
    the fp32 network output agrees to 1e-5 rel-RMS.  Whole tiles (256 x 256) and a ragged map (144 x 176: tiles hang over the right / bottom edge)."""
    from oracle.unet import DECODER_CONFIG, synth_state_dict
    from terrain_diffusion_amd.engine import get_engine
    from oracle import rng
    eng = get_engine("cuda")
    cfg = dict(DECODER_CONFIG, out_channels=out_channels)
    m = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(synth_state_dict(cfg, seed=98))
    try:
        for n, h, w in ((2, 256, 256), (3, 144, 176)) if out_channels == 1 else ((2, 144, 176),):
            x = torch.from_numpy(rng.standard_normal(6, (n, DECODER_CONFIG["in_channels"], h, w))).cuda()
            t = torch.full((n,), 0.9)
            outs, tags = {}, {}
            for v in (0, 1):
                with pinned(eng, fewcout=v, profile=1):
                    eng.profile_read(reset=True)
                    outs[v] = m(x, t, []).clone()
                    tags[v] = [l for l, _, _ in eng.profile_ops() if l.startswith("out_conv")]
                    eng.profile_read(reset=True)
            assert len(tags[1]) == 1 and " f6 " in tags[1][0] and " f6 " not in tags[0][0], tags
            e = rel_rms(outs[1].cpu().numpy(), outs[0].cpu().numpy())
            print(f"few-cout output conv {n} x {h} x {w}: vs the MFMA tile rel-RMS {e:.2e}   {tags[1][0]}")
            assert torch.isfinite(outs[1]).all() and float(outs[1].abs().mean()) > 1e-4 and e < 1e-5, e
    finally:
        m.close()


def test_wide_tile_persistent_loop_same_bits(td):
    """Round 6: the wide tile's persistent tile loop (engine option glds_wide_persist = 1; conv_glds_wide.hip, PERS instantiation: 2 x CUs workgroups walk the
    launch's tiles, staging split by wave) keeps the K order of the one-tile-per-workgroup form: the decoder model's forward at 256 x 256 (its 64-channel
    256 x 256 level is 1024 tiles per launch at batch 4 = two rounds of 512 workgroups; encoder blocks with pixel-norm factors, modulation rows, residual
    runs, second outputs and sum-of-squares planes) must come out bit for bit the same with the loop on and off."""
    from oracle.unet import DECODER_CONFIG, synth_state_dict
    from terrain_diffusion_amd.engine import get_engine
    from oracle import rng
    eng = get_engine("cuda")
    m = td.EDMUnet2D(**DECODER_CONFIG, dtype="bf16").load_state_dict(synth_state_dict(DECODER_CONFIG, seed=97))
    x = torch.from_numpy(rng.standard_normal(5, (4, DECODER_CONFIG["in_channels"], 256, 256))).cuda()
    t = torch.full((4,), 0.9)
    outs, tags = {}, {}
    for v in (0, 1):
        with pinned(eng, glds_wide_persist=v, profile=1):
            eng.profile_read(reset=True)
            outs[v] = m(x, t, []).clone()
            tags[v] = [l for l, _, _ in eng.profile_ops()]
            eng.profile_read(reset=True)
    n_p = sum(" f2wp " in l for l in tags[1])
    print("launches on the persistent loop:", n_p, "of", sum(" f2w" in l for l in tags[1]), "wide launches")
    assert n_p >= 4 and all(" f2wp " not in l for l in tags[0]), (n_p, tags[1])
    assert torch.isfinite(outs[0]).all() and float(outs[0].abs().mean()) > 1e-4
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())
    m.close()


@pytest.mark.parametrize("n,hw", [(64, 64), (5, 72)])
def test_wide_tile_against_the_other_tiles_and_the_oracle(td, base, n, hw):
    """Round 6: the wide tile of the LDS-DMA conv (conv_glds_wide.hip: 256 px x 96 / 64 couts, 4 waves, 32-channel K-groups, double-buffered patch).  Its K
    order differs from the other tiles' (channel half outside the taps), so it is compared with a tolerance, not bit for bit: the planner's choice
    (64x64 / 32x32 levels of a 64-window batch) and the tile forced wherever it is legal (option glds_wide = 2: also the launches with a 1x1 tail, the
    16x16 level, ragged 72 -> 36 -> 18 maps whose 16x16 tiles hang over the edge) against the network without it -- eight layers spread over the levels
    and the output -- and sample 0 against the oracle at the bf16 bound."""
    from terrain_diffusion_amd.engine import get_engine
    from oracle import rng
    m, om = base
    eng = get_engine("cuda")
    x = torch.from_numpy(rng.standard_normal(41, (n, 5, hw, hw))).cuda()
    c = torch.from_numpy(rng.standard_normal(42, (n, 58))).cuda()
    t = torch.full((n,), 0.7)
    res = {}
    for k, o in {"off": dict(glds_wide=0, sb=1), "auto": dict(glds_wide=1, sb=1), "force": dict(glds_wide=2, sb=1)}.items():
        if hw == 64:
            res[k] = _forward_with(eng, m, x, t, c, n, **o)
        else:
            with pinned(eng, **o, profile=1):
                eng.profile_read(reset=True)
                y = m(x, t, [c])
                labels = [l for l, _, _ in eng.profile_ops()]
                eng.profile_read(reset=True)
                res[k] = (y, {}, labels)
    n_w = {k: sum(" f2w " in l for l in res[k][2]) for k in res}
    print("launches on the wide tile:", n_w)
    assert n_w["off"] == 0 and n_w["force"] > n_w["auto"] and (n_w["auto"] >= 10 if (n, hw) == (64, 64) else True), n_w
    y0, a0, _ = res["off"]
    for k in ("auto", "force"):
        y, acts, _ = res[k]
        for l in acts:
            e = rel_rms(acts[l].float().cpu().numpy(), a0[l].float().cpu().numpy())
            # two bf16 networks whose convs round differently in the last place: the difference grows with depth (1e-3 after the first blocks, 8e-3 at
            # the 16x16 level) and stays inside the bf16 bound against the fp32 oracle, which is what is asserted below for every arm
            assert e < 2e-2, (k, l, e)
        e = rel_rms(y.cpu().numpy(), y0.cpu().numpy())
        print(f"wide tile {k}: network output vs the other tiles, rel-RMS {e:.2e}")
        assert e < 2e-2, (k, e)
    with torch.no_grad():
        ref = om(x[:1].cpu(), t[:1], [c[:1].cpu()])
    for k in res:
        e = rel_rms(res[k][0][:1].cpu().numpy(), ref.numpy())
        print(f"wide tile {k}: sample 0 vs oracle {e:.3e}")
        assert e < 2e-2, (k, e)


@pytest.mark.parametrize("n,hw,splitk", [(20, 72, 0), (7, 40, 0), (64, 64, 1), (3, 64, 1), (1, 64, 1)])
def test_conv_1x1_dma_ragged_tiles_bit_identical_and_vs_oracle(td, base, n, hw, splitk):
    """the LDS-DMA 1x1 path on maps that do not divide into tiles (72 -> 36 -> 18 -> 9, 40 -> 20 -> 10 -> 5: ragged 16-wide tiles; their out-of-image
    MFMA columns are fed from a clamped address), and with split-K on at small batches (slices that start inside a 1x1 segment, narrow 8-wide tiles,
    pure 1x1 convs): bit-identical to the register path, and sample 0 against the oracle (bf16 bound)."""
    from terrain_diffusion_amd.engine import get_engine
    from oracle import rng
    m, om = base
    eng = get_engine("cuda")
    x = torch.from_numpy(rng.standard_normal(31, (n, 5, hw, hw))).cuda()
    c = torch.from_numpy(rng.standard_normal(32, (n, 58))).cuda()
    t = torch.full((n,), 0.9)
    ys = {}
    for o in (0, 1):
        with pinned(eng, glds_splitk=splitk, glds_dma1x1=o, sb=0, profile=1):   # conv_glds' own split-K + 1x1 paths
            eng.profile_read(reset=True)
            ys[o] = m(x, t, [c]).clone()
            labels = [l for l, _, _ in eng.profile_ops()]
            eng.profile_read(reset=True)
        assert any(" f2" in l and "conv_res1" in l and l.startswith("dec.") for l in labels), labels[:5]
    assert torch.equal(ys[0], ys[1]), float((ys[0] - ys[1]).abs().max())
    with torch.no_grad():
        ref = om(x[:1].cpu(), t[:1], [c[:1].cpu()])
    err = rel_rms(ys[1][0].cpu().numpy(), ref[0].numpy())
    assert err < 2e-2, err


def _oracle_windows(om, noise, cond, steps, sigma_data=0.5):
    """oracle EDM loop (sample_diffusion_base.py:147-162 restated in oracle/tiling.py) on a batch of windows: returns the pre-blend x."""
    from oracle import schedule
    sigmas, _ = schedule.karras_sigmas(steps, 0.002, 80.0, 7.0)
    orders = schedule.solver_orders(steps)
    x = noise * sigmas[0]
    m_prev = None
    with torch.no_grad():
        for i in range(steps):
            xin = schedule.precondition_inputs(x, sigmas[i], sigma_data)
            cn = schedule.trigflow_t(sigmas[i].view(-1).expand(x.shape[0]), sigma_data)
            F_ = om(xin, cn, [cond])
            x, m_prev = schedule.dpm_step(sigmas, i, orders[i], x, F_, m_prev, sigma_data)
    return x


def test_config2_grid8_end_to_end(td, base):
    """(c) BASELINE configs[2]: 8x8 windows of 64x64 (stride 32) on a 288x288 canvas, 20 DPM-Solver++ steps, bf16, all 64 windows in one batch
    -- the bench.py default.  Four windows (corners and interior) are compared with the oracle BEFORE the blend (windows are independent),
    and the blended canvas with an independent torch blend of the engine's own windows (sample_diffusion_base.py:164-168)."""
    from oracle import rng, tiling
    m, om = base
    sch = td.EDMDPMSolverMultistepScheduler(sigma_min=0.002, sigma_max=80.0, sigma_data=0.5)
    cond = tiling.synthetic_cond_grid(8, 8)
    seed = 42 + 5819
    y, win = td.sample_base_diffusion(m, sch, (1, 5, 288, 288), cond, cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0),
                                      histogram_raw=torch.zeros(1, 5), steps=20, tile_size=64, noise_seed=seed, return_windows=True)
    assert len(win) == 64 and torch.isfinite(y).all()
    starts = tiling.tile_starts(288, 64, 32)
    pick = [(0, 0), (3, 4), (7, 7), (2, 6)]
    noise = torch.stack([torch.from_numpy(rng.gaussian_noise_patch(seed, starts[i], starts[j], 64, 64, channels=5, tile_h=64, tile_w=64)) for i, j in pick])
    c58 = torch.cat([tiling.process_cond_img(cond[..., i:i + 4, j:j + 4], torch.zeros(1, 5), torch.zeros(7), torch.ones(7), 0.0) for i, j in pick])
    ref = _oracle_windows(om, noise, c58, 20)
    errs = [rel_rms(win[t].cpu().numpy(), ref[k].numpy()) for k, t in enumerate(pick)]
    print("configs[2] windows (0,0) (3,4) (7,7) (2,6), bf16 x 20 steps vs oracle:", ["%.3e" % e for e in errs])
    assert max(errs) < 2e-2, errs
    # blend: weighted sum in the reference's loop order over the engine's own windows, then / weights / sigma_data
    w = tiling.linear_weight_window(64)
    acc = torch.zeros(5, 288, 288)
    wsum = torch.zeros(288, 288)
    for i, i0 in enumerate(starts):
        for j, j0 in enumerate(starts):
            acc[:, i0:i0 + 64, j0:j0 + 64] += win[(i, j)].cpu() * w
            wsum[i0:i0 + 64, j0:j0 + 64] += w
    blend_ref = acc / wsum / 0.5
    e_blend = rel_rms(y[0].cpu().numpy(), blend_ref.numpy())
    print(f"configs[2] blended canvas vs independent blend of the same windows: {e_blend:.3e}")
    assert e_blend < 1e-6
    # and against the reference-pinned golden path end to end at this size: the oracle's blend of ITS four windows agrees where only they contribute
    assert rel_rms(y[0, :, :32, :32].cpu().numpy(), (ref[0][:, :32, :32] / 0.5).numpy()) < 2e-2


def test_config3_grid32_full_size_one_gpu(td, base):
    """BASELINE configs[3] at FULL size on one GPU: 32x32 windows of 64x64 (stride 32) on the 1056x1056 latent canvas,
    all 20 DPM-Solver++ steps, bf16, batch-invariant mode (what the sharded run uses), 16 batches of 64 windows.
      * four windows -- corner, top edge, interior, last row / last column -- against the oracle BEFORE the blend, as test_config2 does;
      * the one-rank canvas against the canvas assembled from TWO simulated ranks (ShardPlan's 2-D block mesh, the seam windows handed over in
        memory, every rank blending its own region): bit for bit.
    The multi-rank dry run of bench.py only ran 2 of the 20 steps and checked properties; this is the full-size comparison it lacked."""
    from oracle import rng, tiling
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.parallel import ShardPlan, engine_fns, blend_region
    m, om = base
    eng = get_engine("cuda")
    with pinned(eng, batch_invariant=1):
        sch = td.EDMDPMSolverMultistepScheduler(sigma_min=0.002, sigma_max=80.0, sigma_data=0.5)
        H = W = 1056
        starts = tiling.tile_starts(H, 64, 32)
        assert len(starts) == 32
        cond = tiling.synthetic_cond_grid(32, 32)
        seed = 42 + 5819
        kw = dict(cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0), histogram_raw=torch.zeros(1, 5))
        y, win = td.sample_base_diffusion(m, sch, (1, 5, H, W), cond, steps=20, tile_size=64, noise_seed=seed, max_batch=64, return_windows=True, **kw)
        assert len(win) == 1024 and tuple(y.shape) == (1, 5, H, W) and torch.isfinite(y).all()
        pick = [(0, 0), (0, 17), (16, 13), (31, 31)]
        noise = torch.stack([torch.from_numpy(rng.gaussian_noise_patch(seed, starts[i], starts[j], 64, 64, channels=5, tile_h=64, tile_w=64)) for i, j in pick])
        c58 = torch.cat([tiling.process_cond_img(cond[..., i:i + 4, j:j + 4], torch.zeros(1, 5), torch.zeros(7), torch.ones(7), 0.0) for i, j in pick])
        ref = _oracle_windows(om, noise, c58, 20)
        errs = [rel_rms(win[t].cpu().numpy(), ref[k].numpy()) for k, t in enumerate(pick)]
        print("configs[3] windows (0,0) (0,17) (16,13) (31,31), bf16 x 20 steps, batch-invariant, vs oracle:", ["%.3e" % e for e in errs])
        assert max(errs) < 2e-2, errs
        # the canvas corner only the first window reaches, end to end against the oracle
        assert rel_rms(y[0, :, :32, :32].cpu().numpy(), (ref[0][:, :32, :32] / 0.5).numpy()) < 2e-2
        del win
        # two simulated ranks: same plan / seam lists / regional blend as the RCCL path (parallel.py), exchange done in memory
        plan = ShardPlan(H, W, 64, 2)
        fns = engine_fns(m, sch, plan, cond, steps=20, channels=5, noise_seed=seed, noise_origin=(0, 0), max_batch=64, **kw)
        tiles = [fns[0](plan.windows[r]) for r in range(2)]
        full = torch.empty((5, H, W), device="cuda")
        seam = 0
        for r in range(2):
            have = {}
            for w_ in plan.needed[r]:
                o = plan.owner[w_]
                have[w_] = tiles[o][plan.windows[o].index(w_)]
                seam += o != r
            y0, y1, x0, x1 = plan.regions[r]
            full[:, y0:y1, x0:x1] = blend_region(plan, r, have, fns[1], fns[2], 5, 1.0 / 0.5)
        assert seam == 32, seam                      # one column (or row) of 32 windows reaches into the neighbour's region
        assert torch.equal(full[None], y), "two-rank canvas differs from the one-rank canvas"


@pytest.mark.parametrize("dual", [0, 1])
def test_config3_default_plan_bit_identical_across_rank_counts(td, base, dual):
    """BASELINE configs[3] WITHOUT batch_invariant.  At world 1 / 2 / 4 / 8 a rank owns 1024 / 512 / 256 / 128 windows and the
    sampler cuts them into batches of max_batch = 64: every launch on every rank count has the same batch size, hence the same plan (tile shapes,
    split-K, conv flavour) and the same K order -- a window's result must not depend on which 63 other windows ride in its batch or on its position in
    it.  Full size, 20 steps, bf16, DEFAULT plan (and with the two sampler lanes bench.py's grid32 turns on): the one-rank canvas against the canvases
    assembled from 2 and 4 simulated ranks, bit for bit.  Loop sharded: sample_diffusion_base.py:147-168."""
    from oracle import tiling
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.parallel import ShardPlan, engine_fns, blend_region
    m, om = base
    eng = get_engine("cuda")
    with pinned(eng, batch_invariant=0, dual_stream=dual):
        sch = td.EDMDPMSolverMultistepScheduler(sigma_min=0.002, sigma_max=80.0, sigma_data=0.5)
        H = W = 1056
        cond = tiling.synthetic_cond_grid(32, 32)
        seed = 42 + 5819
        kw = dict(cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0), histogram_raw=torch.zeros(1, 5))
        y = td.sample_base_diffusion(m, sch, (1, 5, H, W), cond, steps=20, tile_size=64, noise_seed=seed, max_batch=64, **kw)
        assert tuple(y.shape) == (1, 5, H, W) and torch.isfinite(y).all()
        for world in (2, 4):
            plan = ShardPlan(H, W, 64, world)
            assert all(len(ws) % 64 == 0 for ws in plan.windows), [len(ws) for ws in plan.windows]
            fns = engine_fns(m, sch, plan, cond, steps=20, channels=5, noise_seed=seed, noise_origin=(0, 0), max_batch=64, **kw)
            tiles = [fns[0](plan.windows[r]) for r in range(world)]
            full = torch.empty((5, H, W), device="cuda")
            for r in range(world):
                have = {w_: tiles[plan.owner[w_]][plan.windows[plan.owner[w_]].index(w_)] for w_ in plan.needed[r]}
                y0, y1, x0, x1 = plan.regions[r]
                full[:, y0:y1, x0:x1] = blend_region(plan, r, have, fns[1], fns[2], 5, 1.0 / 0.5)
            nbad = int((full[None] != y).sum())
            print(f"configs[3] default plan (dual_stream={dual}): {world}-rank canvas vs one-rank canvas: {nbad} differing values")
            assert nbad == 0, f"{world}-rank canvas differs from the one-rank canvas in {nbad} values (default plan, dual_stream={dual})"
            del tiles, full


def test_fp16_tile_variants_bit_identical_and_close_to_bf16(td):
    """fp16 storage runs through the same conv flavours (v_mfma_f32_32x32x16_f16): the tile-shape identity holds there too, and the result sits
    closer to the fp32 oracle than bf16's (10 vs 7 mantissa bits)."""
    from oracle.unet import BASE_CONFIG, OracleUnet, synth_state_dict
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    sd = synth_state_dict(BASE_CONFIG, seed=1234)
    m = td.EDMUnet2D(**BASE_CONFIG, dtype="fp16").load_state_dict(sd)
    x, c = _batch_inputs(8, seed=9)
    t = torch.full((8,), 0.7)
    outs = {}
    for k, o in {"big": dict(glds_splitk=0, glds_variant=0), "small": dict(glds_splitk=0, glds_variant=1)}.items():
        outs[k] = _forward_with(eng, m, x.cuda(), t, c.cuda(), 8, **o)[0]
    assert torch.equal(outs["big"], outs["small"])
    with torch.no_grad():
        ref = OracleUnet(BASE_CONFIG, sd)(x[:2], t[:2], [c[:2]])
    err = rel_rms(outs["big"][:2].cpu().numpy(), ref.numpy())
    print(f"fp16 base forward vs oracle: {err:.3e}")
    assert err < 4e-3
    m.close()


def test_solver_order_one_is_honoured(td):
    """a scheduler with solver_order=1 must give first-order results on the engine path (it silently ran 2M before)."""
    from oracle import tiling
    from oracle.unet import synth_state_dict, tiny_config
    cfg = tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype="fp32").load_state_dict(synth_state_dict(cfg, seed=77))
    kw = dict(cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0), histogram_raw=torch.zeros(1, 5), steps=6, tile_size=16)
    cond = tiling.synthetic_cond_grid(3, 3)
    outs = {}
    for order in (1, 2):
        sch = td.EDMDPMSolverMultistepScheduler(solver_order=order)
        outs[order] = td.sample_base_diffusion(m, sch, (1, 5, 32, 32), cond, **kw)
    assert not torch.equal(outs[1], outs[2])
    # host-driven loop with the scheduler mirror's own step() (first order) as the reference
    sch = td.EDMDPMSolverMultistepScheduler(solver_order=1)
    sch.set_timesteps(6)
    from terrain_diffusion_amd import noise as _noise
    x = _noise.gaussian_noise_patches(42 + 5819, [(0, 0)], 16, 16, channels=5, tile_h=64, tile_w=64, scale=float(sch.sigmas[0]), device="cuda")
    from terrain_diffusion_amd.sampling import _process_cond_img
    c = _process_cond_img(cond[..., 0:4, 0:4], torch.zeros(1, 5), torch.zeros(7), torch.ones(7), 0.0).cuda()
    xs = x.clone()
    for i, tt in enumerate(sch.timesteps):
        sig = sch.sigmas[i]
        F = m(sch.precondition_inputs(xs, sig), sch.trigflow_precondition_noise(sig).view(1), [c])
        xs = sch.step(F, tt, xs).prev_sample
    from terrain_diffusion_amd.sampling import sample_tiles_edm
    xe = sample_tiles_edm(m, td.EDMDPMSolverMultistepScheduler(solver_order=1), x.clone(), c, 6)
    assert rel_rms(xe.cpu().numpy(), xs.cpu().numpy()) < 1e-5
    m.close()


def test_graph_survives_cvec_reallocation(td):
    """the cached EDM graph holds pointers into the modulation-vector buffer; a later call on the same (N,H,W) plan
    that needs more rows re-allocates it.  The next sampler call must re-capture instead of replaying over freed memory."""
    from oracle.unet import synth_state_dict, tiny_config
    cfg = tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(synth_state_dict(cfg, seed=5))
    sch = td.EDMDPMSolverMultistepScheduler()
    from terrain_diffusion_amd.sampling import sample_tiles_edm
    g = torch.Generator(device="cuda").manual_seed(3)
    n = 8
    x0 = torch.randn(n, 5, 16, 16, device="cuda", generator=g) * 80
    c = torch.randn(n, 58, device="cuda", generator=g)
    a = sample_tiles_edm(m, sch, x0.clone(), c, 4)            # captures the graph: 4 steps x 8 tiles = 32 rows
    t = torch.linspace(0.1, 1.5, n)                           # distinct t per sample: n*n = 64 rows -> reallocation
    _ = m(torch.randn(n, 5, 16, 16, device="cuda", generator=g), t, [c])
    junk = [torch.randn(1 << 20, device="cuda") for _ in range(8)]  # recycle freed device memory
    b = sample_tiles_edm(m, sch, x0.clone(), c, 4)
    del junk
    assert torch.equal(a, b)
    m.close()


def test_batch_too_large_for_32bit_addressing_is_refused(td):
    from oracle.unet import synth_state_dict, tiny_config
    cfg = tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(synth_state_dict(cfg, seed=5))
    with pytest.raises(td.TdError, match="32-bit"):
        m(torch.zeros(200, 5, 512, 512, device="cuda"), torch.zeros(200), [torch.zeros(200, 58, device="cuda")])
    m.close()


def test_nccl_seam_exchange_two_gpus(td):
    """the real RCCL branch of the seam exchange (parallel.exchange_windows: batch_isend_irecv on device tensors); needs >= 2 GPUs."""
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible: the RCCL path is covered by the driver's multi-GPU bench run")
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29731",
                          os.path.join(root, "tests", "_nccl_exchange_worker.py")], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "NCCL_EXCHANGE_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-5), ("bf16", 2e-2), ("fp16", 4e-3)])
def test_decoder_window_at_real_size(td, dtype, tol):
    """BASELINE configs[4] / VERDICT item 6: ONE decoder window at its production size -- 512x512 pixels, stride 384, 64x64 latents upsampled x8
    (world_pipeline.py:1209-1242) -- against the oracle's _decoder_inference restatement (pinned to the reference at tile 64).  The 64-channel
    512x512 layers are the activation-bound regime no other test touches."""
    from oracle import stages
    from oracle.unet import DECODER_CONFIG, OracleUnet, synth_state_dict
    from terrain_diffusion_amd.infinite_tensor import InfiniteTensor, TensorWindow
    from terrain_diffusion_amd.pipeline import build_decoder_stage
    from oracle import rng
    sd = synth_state_dict(DECODER_CONFIG, seed=2468)
    md = td.EDMUnet2D(**DECODER_CONFIG, dtype=dtype).load_state_dict(sd)
    g = torch.Generator().manual_seed(11)
    wl = torch.rand(64, 64, generator=g) + 0.5
    lat_win = torch.cat([torch.from_numpy(rng.standard_normal(33, (5, 64, 64))) * wl, wl[None]])
    src = InfiniteTensor((6, None, None), lambda ctx: lat_win, TensorWindow(size=(6, 64, 64), stride=(6, 48, 48)), tensor_id="lat_src512")
    ds = build_decoder_stage(md, src, seed=1234, tile_size=512, tile_stride=384)
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    with pinned(eng, profile=1):
        eng.profile_read(reset=True)
        try:
            out = ds.f([(0, 1, -2)], [lat_win])[0]
            labels = [l for l, _, _ in eng.profile_ops()]
        finally:
            eng.profile_read(reset=True)
    if dtype != "fp32":
        # round 6: the 64-cout levels of the decoder run on the wide tile of the LDS-DMA conv, 1x1 tails (the dec blocks' fused skip conv) included --
        # the LDS-DMA-streamed tail of conv_glds_wide.hip is what this window exercises against the oracle
        wide = [l for l in labels if " f2w " in l]
        assert any("dec.512x512_block" in l and "conv_res1" in l for l in wide) and any("enc.512x512_block" in l for l in wide), labels[:8]
    ref = stages.decoder_inference(OracleUnet(DECODER_CONFIG, sd), (0, 1, -2), lat_win, seed=1234, tile_size=512, tile_stride=384)
    assert out.shape == ref.shape == (2, 512, 512)
    assert torch.equal(out[1], ref[1])                                          # blend window: bit-exact
    err = rel_rms((out[0] / out[1]).numpy(), (ref[0] / ref[1]).numpy())
    print(f"decoder 512x512 window {dtype}: rel-RMS vs oracle {err:.3e}")
    assert err < tol
    md.close()


def test_config4_cascade_full_size_fp16_capped_store_vs_oracle_chain(td):
    """BASELINE configs[4] in ONE test: the coarse -> two-phase latent -> decoder cascade with the FULL-SIZE base model
    (30m, 192 channels), the decoder at its production window (512x512 pixels, stride 384), **fp16**, every window in HBM behind a store capped
    below the working set (streaming eviction + recomputation), against the same InfiniteTensor graph whose window functions are the CPU oracle's
    (oracle/stages.py, pinned window by window to the reference's _coarse_inference / _latent_inference / _decoder_inference).
    The region [128,384) x [128,768) of the decoder tensor is covered by exactly the decoder windows (0,0) and (0,1); they pull 15 latent windows
    (two blended trig-flow phases each) and 2 coarse windows through the graph.  Tolerance: fp16 <= 4e-3 per forward (N2), 1.5e-2 through the chain."""
    from oracle import stages
    from oracle.unet import BASE_CONFIG, COARSE_CONFIG, DECODER_CONFIG, OracleUnet, synth_state_dict
    from terrain_diffusion_amd.pipeline import build_coarse_stage, build_latent_stage, build_decoder_stage
    from terrain_diffusion_amd.infinite_tensor import InfiniteTensor, TensorWindow, DeviceTileStore
    seed = 4242
    means6 = [0.3, -0.2, 0.1, 0.0, 0.4, -0.1]; stds6 = [1.5, 0.8, 1.2, 0.9, 1.1, 0.7]; snr = [0.5, 0.4, 0.6, 0.3, 0.8]
    hist = torch.tensor([[0.1, 0.3, 0.2, 0.25, 0.15]])
    cm, cs_ = [0.2, 0.1, 0.0, -0.1, 0.3, 0.0, 0.66], [1.2, 1.1, 0.9, 1.0, 1.3, 0.8, 0.47]
    sdc, sdb, sdd = synth_state_dict(COARSE_CONFIG, seed=1), synth_state_dict(BASE_CONFIG, seed=1234), synth_state_dict(DECODER_CONFIG, seed=2468)
    mc = td.EDMUnet2D(**COARSE_CONFIG, dtype="fp16").load_state_dict(sdc)
    mb = td.EDMUnet2D(**BASE_CONFIG, dtype="fp16").load_state_dict(sdb)
    md = td.EDMUnet2D(**DECODER_CONFIG, dtype="fp16").load_state_dict(sdd)
    # capped store: one decoder window (2 x 512 x 512 fp32 = 2 MiB) + a few latent windows -- far below the ~6 MiB the region touches
    store = DeviceTileStore(cache_size_bytes=3 * 2 ** 20)
    kwr = dict(device_resident=True, tile_store=store)
    coarse = build_coarse_stage(mc, td.EDMDPMSolverMultistepScheduler(), seed=seed, cond_map_fn=stages.synthetic_coarse_map, coarse_means=means6,
                                coarse_stds=stds6, cond_snr=snr, **kwr)
    lat = build_latent_stage(mb, seed=seed, coarse=coarse, histogram_raw=hist, cond_means=cm, cond_stds=cs_, **kwr)
    dec = build_decoder_stage(md, lat, seed=seed, tile_size=512, tile_stride=384, **kwr)
    box = (slice(None), slice(128, 384), slice(128, 768))
    got = dec[box].cpu()
    assert store.evictions > 0, "the store was meant to evict while the region streams"
    # ---- the same graph on the oracle (fp32 CPU)
    oc, ob, od = OracleUnet(COARSE_CONFIG, sdc), OracleUnet(BASE_CONFIG, sdb), OracleUnet(DECODER_CONFIG, sdd)
    ocoarse = InfiniteTensor((7, None, None), lambda ctx: stages.coarse_inference(oc, ctx, seed=seed, cond_map_fn=stages.synthetic_coarse_map, means=means6,
                             stds=stds6, cond_snr=snr), TensorWindow(size=(7, 64, 64), stride=(7, 48, 48)), tensor_id="o4_coarse")
    lwin, cwin = TensorWindow(size=(6, 64, 64), stride=(6, 32, 32)), TensorWindow(size=(7, 4, 4), stride=(7, 1, 1), offset=(0, -1, -1))
    kw = dict(seed=seed, histogram_raw=hist, cond_means=cm, cond_stds=cs_)
    t0, t1 = torch.atan(torch.tensor(80.0) / 0.5), torch.arctan(torch.tensor(0.35) / 0.5)
    ol0 = InfiniteTensor((6, None, None), lambda ctx, c: stages.latent_inference(ob, [ctx], None, [c], t0, seed_offset=5819, **kw)[0], lwin,
                         args=(ocoarse,), args_windows=(cwin,), tensor_id="o4_lat0")
    ol1 = InfiniteTensor((6, None, None), lambda ctx, s_, c: stages.latent_inference(ob, [ctx], [s_], [c], t1, seed_offset=5820, **kw)[0], lwin,
                         args=(ol0, ocoarse), args_windows=(lwin, cwin), tensor_id="o4_lat1")
    odec = InfiniteTensor((2, None, None), lambda ctx, l: stages.decoder_inference(od, ctx, torch.as_tensor(l), seed=seed, tile_size=512, tile_stride=384),
                          TensorWindow(size=(2, 512, 512), stride=(2, 384, 384)), args=(ol1,), args_windows=(TensorWindow(size=(6, 64, 64), stride=(6, 48, 48)),),
                          tensor_id="o4_dec")
    ref = torch.as_tensor(odec[box])
    assert got.shape == ref.shape == (2, 256, 640)
    assert torch.allclose(got[1], ref[1], rtol=1e-6, atol=1e-7)                                              # blend weights of the two windows
    # the latent region the two decoder windows consumed, and the decoded residual
    e_lat = rel_rms((torch.as_tensor(lat[:5, 16:48, 16:96]).cpu() / torch.as_tensor(lat[5:6, 16:48, 16:96]).cpu()).numpy(),
                    (torch.as_tensor(ol1[:5, 16:48, 16:96]) / torch.as_tensor(ol1[5:6, 16:48, 16:96])).numpy())
    err = rel_rms((got[0] / got[1]).numpy(), (ref[0] / ref[1]).numpy())
    print(f"configs[4] cascade, full-size base + 512x512 decoder, fp16, capped store: latents {e_lat:.3e}, decoder output {err:.3e} rel-RMS vs the oracle chain; {store.evictions} evictions")
    assert e_lat < 1e-2 and err < 1.5e-2
    for m_ in (mc, mb, md):
        m_.close()


def test_bench_multi_rank_branch_dry_run_on_one_gpu():
    """bench.py --gpus 2 end to end on ONE GPU (TD_BENCH_ONE_GPU=1: both ranks on cuda:0, seams through gloo / host memory -- RCCL refuses two
    ranks on one device): self-launch through torch.distributed.run, 2-D block mesh, seam exchange, per-rank blend, max-over-ranks timing and the
    N > 1 JSON line (strong scaling, seam object).  A plumbing check of the branch the 8-GPU driver run takes, not a measurement."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TD_BENCH_ONE_GPU="1")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--edm-steps", "2"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["decoded_mp_per_step"] == pytest.approx(71.368704)
    assert d["seam"]["bytes_total_per_step"] == 32 * 5 * 64 * 64 * 4 and d["seam"]["windows_rank0"] == 512 and "dry run" in d["seam"]["backend"]
    assert d["value"] > 0 and d["roofline"]["frac"] > 0


def test_bench_plain_run_times_the_steps_only_and_full_adds_the_legs(tmp_path):
    """bench.py without --full: the timed steps and the line (no kernel profile, latency leg or CPU baseline); --dump-outputs writes the last timed
    step's tiles.  With --full the extra legs are back in the line, and the same arguments give the same outputs (seeded inputs)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--workload", "tiles", "--tiles-per-step", "2", "--edm-steps", "2", "--steps", "3", "--warmup", "1"]
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *common, *extra, "--dump-outputs", str(tmp_path / mode)],
                           capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[mode] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    p, f = lines["plain"], lines["full"]
    for d in (p, f):
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["unit"] == "MP/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
        assert abs(d["value"] - d["config"]["decoded_mp_per_step"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    assert "latency_single_tile_ms" not in p and "cpu_baseline" not in p and "all_conv_kernels_ms_per_step" not in p["roofline"]
    assert p["roofline"]["frac"] > 0
    assert f["latency_single_tile_ms"] > 0 and f["roofline"]["all_conv_kernels_ms_per_step"] > 0 and "cpu_baseline" not in f
    a, b = np.load(tmp_path / "plain" / "tiles.npy"), np.load(tmp_path / "full" / "tiles.npy")
    assert a.dtype == np.float32 and a.shape == (2, 5, 64, 64) and np.isfinite(a).all()
    assert rel_rms(b, a) < 1e-3
