"""GPU parity tests: the HIP path (through the C-ABI) vs the oracle and the committed golden vectors.

Tolerances (stated per SURVEY.md §8d):
  * integer work (tile seeds, PCG stream -> accept/reject order): bit-exact; normals: <= 1 ulp fp32 (f64 log on the
    device is not correctly rounded), with >= 99.99 % of values bit-identical.
  * fp32 mode (exact-fp32 MFMA, weights folded with the reference's fp32 arithmetic): <= 5e-6 rel-RMS per forward,
    <= 1e-5 after 20 solver steps (measured 7.1e-7 / 3.8e-7 on the full-size base model; the reference's own
    fp32-vs-fp64 is 4.7e-7 / 3.0e-7).
  * bf16 mode (bf16 storage, fp32 accumulate): <= 2e-2 rel-RMS per forward and after 20 steps (measured 6.2e-3 / 4.0e-3;
    the reference's own bf16-vs-fp32 is 1.0e-2 / 1.5e-2).
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
def orc():
    from oracle import rng, schedule, tiling, unet
    return dict(rng=rng, schedule=schedule, tiling=tiling, unet=unet)


def _model(td, orc, cfg, seed, dtype):
    m = td.EDMUnet2D(**cfg, dtype=dtype)
    m.load_state_dict(orc["unet"].synth_state_dict(cfg, seed=seed))
    return m


# ------------------------------------------------------------------------------------------- noise
def test_tile_seed_exact(td, golden):
    g = golden("rng")
    for (seed, _, _), (ty, tx), ref in zip(g["tile_seed_in"], g["tile_seed_in_signed"], g["tile_seed_out"]):
        assert td._tile_seed(int(seed), int(ty), int(tx)) == int(ref)


def _ulp_diff(a, b):
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def test_standard_normal_stream(td, golden, orc):
    g = golden("rng")
    got = td.standard_normal(123, (4097,))
    ref = g["normal_seed123_n4097"]
    # BIT-exact against the reference stream (round 3: 8 000 000 device normals of four seeds were compared with the host stream and not one
    # differed, profiles/r03_noise_bit_exactness.txt -- the 1-ulp / 99.99 % allowance of rounds 1-2 was never needed)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), int(_ulp_diff(got, ref).max())
    # odd length, single value, longer than one round
    for seed, n in ((7, 1), (9, 2047), (11, 70001)):
        a, b = td.standard_normal(seed, (n,)), orc["rng"].standard_normal(seed, (n,)).astype(np.float32)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (seed, n)


def test_noise_patches(td, golden, orc):
    g = golden("rng")
    cases = [("patch_latent_m32_32", (42, -32, 32, 64, 64, 5, 64, 64)), ("patch_latent_aligned", (42 + 5819, 128, -64, 64, 64, 5, 64, 64)),
             ("patch_coarse_48_m96", (43, 48, -96, 64, 64, 6, 64, 64)), ("patch_small", (7, -3, 61, 7, 9, 2, 16, 32)), ("patch_1x1", (7, -1, -1, 1, 1, 1, 8, 8))]
    for key, (seed, y0, x0, h, w, c, th, tw) in cases:
        got = td.gaussian_noise_patch(seed, y0, x0, h, w, channels=c, tile_h=th, tile_w=tw)
        # north_star: "bit-reproducible per (seed, tile-coord)" -- and bit-EQUAL to the reference's patches (negative coordinates, 4-tile straddles)
        assert got.shape == g[key].shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(g[key]).view(np.uint32)), (key, int(_ulp_diff(got, g[key]).max()))
    # batched windows share noise tiles; overlap consistency
    origins = [(32 * i, 32 * j) for i in range(3) for j in range(3)]
    b = td.gaussian_noise_patches(99, origins, 64, 64, channels=5, tile_h=64, tile_w=64, scale=2.0).cpu().numpy()
    ref = np.stack([orc["rng"].gaussian_noise_patch(99, y, x, 64, 64, 5, 64, 64) for y, x in origins]).astype(np.float32) * np.float32(2.0)
    assert np.array_equal(b, ref)   # scaling by 2 is exact in fp32
    assert np.array_equal(b[0][:, 32:, 32:], b[4][:, :32, :32])


def test_schedule(td, golden):
    g = golden("schedule")
    for n in (4, 12, 20, 32):
        # the sigma ladder is host arithmetic with the reference's own fp32 torch ops: bit-exact (the round-1 C export, 2e-6 off, is gone)
        sch = td.EDMDPMSolverMultistepScheduler()
        sch.set_timesteps(n)
        assert np.array_equal(sch.sigmas.numpy(), g[f"sigmas_{n}"])
        # timesteps = 0.25*ln(sigma) are only a lookup key; torch.log differs by 1 ulp between host CPUs (SLEEF code path)
        assert np.allclose(sch.timesteps.numpy(), g[f"timesteps_{n}"], rtol=3e-7, atol=1e-7)


def test_weight_window_exact(td, golden):
    g = golden("geometry")
    for s in (4, 16, 64, 512):
        assert np.array_equal(td._linear_weight_window(s)[0, 0].cpu().numpy(), g[f"lww_{s}"])


# ------------------------------------------------------------------------------------------- U-Net forward
@pytest.mark.parametrize("dtype,tol", [("fp32", 5e-6), ("bf16", 2e-2)])
def test_unet_tiny(td, orc, golden, dtype, tol):
    g = golden("unet")
    cfg = orc["unet"].tiny_config(64, 1)
    m = _model(td, orc, cfg, 77, dtype)
    x = torch.from_numpy(orc["rng"].standard_normal(7, (2, 5, 16, 16)))
    t = torch.tensor([1.2, 0.3])
    cond = torch.from_numpy(orc["rng"].standard_normal(8, (2, 58)))
    y = m(x.cuda(), noise_labels=t, conditional_inputs=[cond.cuda()])
    assert y.is_cuda and y.shape == (2, 5, 16, 16)
    assert rel_rms(y.cpu().numpy(), g["tiny_out"]) < tol
    # host-pointer path of the C-ABI gives the same answer
    y2 = m(x, noise_labels=t, conditional_inputs=[cond])
    assert not y2.is_cuda and torch.equal(y2, y.cpu())
    m.close()


@pytest.mark.parametrize("dtype,tol", [("fp32", 5e-6), ("bf16", 2e-2)])
def test_unet_tiny2_encoder_attention(td, orc, golden, dtype, tol):
    g = golden("unet")
    cfg = orc["unet"].tiny_config(64, 2, attn_resolutions=[128])
    m = _model(td, orc, cfg, 78, dtype)
    x = torch.from_numpy(orc["rng"].standard_normal(9, (1, 5, 32, 32)))
    y = m(x.cuda(), noise_labels=torch.tensor([0.9]), conditional_inputs=[torch.from_numpy(orc["rng"].standard_normal(10, (1, 58))).cuda()])
    assert rel_rms(y.cpu().numpy(), g["tiny2_out"]) < tol
    m.close()


def test_unet_tiny_batch_invariance(td, orc):
    """each sample of a batch equals the batch-1 result bit-for-bit (fixed reduction order, no atomics)."""
    cfg = orc["unet"].tiny_config(64, 1)
    m = _model(td, orc, cfg, 77, "fp32")
    x = torch.from_numpy(orc["rng"].standard_normal(21, (3, 5, 16, 16))).cuda()
    cond = torch.from_numpy(orc["rng"].standard_normal(22, (3, 58))).cuda()
    t = torch.tensor([0.7, 0.7, 0.7])
    yb = m(x, t, [cond])
    for i in range(3):
        yi = m(x[i:i + 1].contiguous(), t[i:i + 1], [cond[i:i + 1].contiguous()])
        assert rel_rms(yi.cpu().numpy(), yb[i:i + 1].cpu().numpy()) < 1e-6
    m.close()


@pytest.fixture(scope="module")
def base_models(td, orc):
    cfg = dict(orc["unet"].BASE_CONFIG)
    sd = orc["unet"].synth_state_dict(cfg, seed=1234)
    return {d: td.EDMUnet2D(**cfg, dtype=d).load_state_dict(sd) for d in ("fp32", "bf16", "fp16")}


# fp16 storage (WorldPipeline dtype='fp16', BASELINE configs[4]): 10 mantissa bits instead of bf16's 7 -> tolerance 4e-3 (8x tighter than bf16)
@pytest.mark.parametrize("dtype,tol", [("fp32", 5e-6), ("bf16", 2e-2), ("fp16", 4e-3)])
def test_unet_base_forward(td, orc, golden, base_models, dtype, tol):
    g = golden("unet")
    x = torch.from_numpy(orc["rng"].standard_normal(7, (1, 5, 64, 64))).cuda()
    cb = torch.from_numpy(orc["rng"].standard_normal(8, (1, 58))).cuda()
    y = base_models[dtype](x, torch.tensor([1.1]), [cb])
    err = rel_rms(y.cpu().numpy(), g["base_out"])
    print(f"base forward {dtype}: rel-RMS vs reference {err:.3e}")
    assert err < tol


# ------------------------------------------------------------------------------------------- samplers
def _sample(td, m, H, W, steps, tile, seed, **kw):
    from oracle import tiling
    sch = td.EDMDPMSolverMultistepScheduler(sigma_min=0.002, sigma_max=80.0, sigma_data=0.5)
    cond = tiling.synthetic_cond_grid(len(tiling.tile_starts(H, tile, tile // 2)), len(tiling.tile_starts(W, tile, tile // 2)))
    return td.sample_base_diffusion(m, sch, (1, 5, H, W), cond, cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0),
                                    histogram_raw=torch.zeros(1, 5), steps=steps, tile_size=tile, noise_seed=seed, **kw)


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-5), ("bf16", 2e-2), ("fp16", 4e-3)])
def test_tiled_sampler_tiny(td, orc, golden, dtype, tol):
    g = golden("sampling")
    cfg = orc["unet"].tiny_config(64, 1)
    m = _model(td, orc, cfg, 77, dtype)
    for key, (H, W, steps, seed) in {"tiny_grid3_steps6": (32, 32, 6, 42 + 5819), "tiny_grid3_steps16": (32, 32, 16, 42 + 5819),
                                     "tiny_ragged_40x24_steps5": (40, 24, 5, 99)}.items():
        y = _sample(td, m, H, W, steps, 16, seed)
        e_ref = rel_rms(y.cpu().numpy(), g[key])
        assert e_ref < tol, (key, e_ref)
        # batching: max_batch=2 chunks vs one batch.  The default plan picks tile shape / split-K per batch size, so the K summation
        # order may differ (fp32: ~1e-6, bf16: a few 1e-3); engine option batch_invariant pins it -> bit-identical
        y2 = _sample(td, m, H, W, steps, 16, seed, max_batch=2)
        e_b = rel_rms(y2.cpu().numpy(), y.cpu().numpy())
        assert e_b < {"fp32": 1e-5, "bf16": 1e-2, "fp16": 2e-3}[dtype], (key, "chunked vs single batch", e_b)
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    with pinned(eng, batch_invariant=1):
        ya = _sample(td, m, 32, 32, 6, 16, 42 + 5819)
        yb = _sample(td, m, 32, 32, 6, 16, 42 + 5819, max_batch=2)
        assert torch.equal(ya, yb), ("batch_invariant mode", float((ya - yb).abs().max()))
        e_inv = rel_rms(ya.cpu().numpy(), g["tiny_grid3_steps6"])
        assert e_inv < tol, ("batch_invariant mode vs reference", e_inv)
    m.close()


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-5), ("bf16", 3e-2)])
def test_autoguidance_vs_reference(td, orc, golden, dtype, tol):
    """sample_base_diffusion(guide_model=..., guidance_scale=...) on the engine (td_sample_edm_guided: both U-Nets per step, the guidance mix
    fused into the solver-step kernel) against the reference's own guided sampler output.  Guidance extrapolates (scale 2: F_g + 2 (F_m - F_g))
    and so amplifies bf16 rounding of both models: 3e-2."""
    from oracle import tiling
    g = golden("guided")
    cfg_m, cfg_g = orc["unet"].tiny_config(128, 1), orc["unet"].tiny_config(64, 1)
    m, gm = _model(td, orc, cfg_m, 81, dtype), _model(td, orc, cfg_g, 82, dtype)
    sch = td.EDMDPMSolverMultistepScheduler(sigma_min=0.002, sigma_max=80.0, sigma_data=0.5)
    for key, (H, W, steps, scale) in {"guided_grid3_steps6_s2": (32, 32, 6, 2.0), "guided_ragged_24x40_steps5_s1p5": (24, 40, 5, 1.5)}.items():
        cond = tiling.synthetic_cond_grid(len(tiling.tile_starts(H, 16, 8)), len(tiling.tile_starts(W, 16, 8)))
        y = td.sample_base_diffusion(m, sch, (1, 5, H, W), cond, cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0),
                                     histogram_raw=torch.zeros(1, 5), steps=steps, tile_size=16, guide_model=gm, guidance_scale=scale)
        err = rel_rms(y.cpu().numpy(), g[key])
        print(f"autoguidance {key} {dtype}: rel-RMS vs reference {err:.3e}")
        assert err < tol, (key, err)
        y1 = td.sample_base_diffusion(m, sch, (1, 5, H, W), cond, cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0),
                                      histogram_raw=torch.zeros(1, 5), steps=steps, tile_size=16, guide_model=gm, guidance_scale=1.0)
        assert rel_rms(y1.cpu().numpy(), g[key]) > 10 * tol   # scale 1.0 == no guidance: must differ from the guided golden
    m.close(); gm.close()


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-5), ("bf16", 2e-2)])
def test_consistency_sampler_tiny(td, orc, golden, dtype, tol):
    from oracle import tiling
    g = golden("sampling")
    cfg = orc["unet"].tiny_config(64, 1)
    m = _model(td, orc, cfg, 77, dtype)
    sch = td.EDMDPMSolverMultistepScheduler()
    y = td.sample_base_consistency(m, sch, (1, 5, 32, 32), tiling.synthetic_cond_grid(3, 3), cond_means=torch.zeros(7), cond_stds=torch.ones(7),
                                   noise_level=torch.tensor(0.0), histogram_raw=torch.zeros(1, 5), intermediate_t=float(np.arctan(0.35 / 0.5)), tile_size=16)
    assert rel_rms(y.cpu().numpy(), g["tiny_consistency_2phase"]) < tol
    m.close()


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-5), ("bf16", 2e-2), ("fp16", 4e-3)])
def test_base_tile_20_steps(td, golden, base_models, dtype, tol):
    """BASELINE config 2 (single 64x64 latent tile, 20 EDM steps) vs the reference's own output."""
    g = golden("sampling")
    y = _sample(td, base_models[dtype], 64, 64, 20, 64, 42 + 5819)
    err = rel_rms(y.cpu().numpy(), g["base_tile_steps20"])
    print(f"base tile x20 steps {dtype}: rel-RMS vs reference {err:.3e}")
    assert err < tol


def test_blend_properties(td, orc):
    """blend of constant tiles returns the constant (any grid, incl. ragged); canvas weight channel == sum of windows."""
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.sampling import blend_windows, blend_normalize
    eng = get_engine("cuda")
    for H, W, size in ((96, 160, 64), (40, 24, 16), (64, 64, 64)):
        hs, ws = orc["tiling"].tile_starts(H, size, size // 2), orc["tiling"].tile_starts(W, size, size // 2)
        idx = [(i, j) for i in range(len(hs)) for j in range(len(ws))]
        tiles = torch.full((len(idx), 5, size, size), 3.25, device="cuda")
        canvas = torch.zeros((6, H, W), device="cuda")
        blend_windows(eng, canvas, tiles, idx, hs, ws, size)
        out = blend_normalize(eng, canvas, 1.0)
        assert torch.allclose(out, torch.full_like(out, 3.25), rtol=1e-6)
        wref = torch.zeros(H, W)
        ww = orc["tiling"].linear_weight_window(size)
        for i in hs:
            for j in ws:
                wref[i:i + size, j:j + size] += ww
        assert torch.equal(canvas[5].cpu(), wref)


def test_engine_side_fold_mode(td, orc, golden):
    """fold="engine" (fp64 normalisation inside the engine) differs from the reference only by the rounding of torch's fp32
    vector_norm over multi-million-element weights (coherent ~3e-6 per large conv): stays within 1e-4 of the reference."""
    g = golden("unet")
    cfg = orc["unet"].tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype="fp32")
    m.load_state_dict(orc["unet"].synth_state_dict(cfg, seed=77), fold="engine")
    x = torch.from_numpy(orc["rng"].standard_normal(7, (2, 5, 16, 16))).cuda()
    y = m(x, torch.tensor([1.2, 0.3]), [torch.from_numpy(orc["rng"].standard_normal(8, (2, 58))).cuda()])
    assert rel_rms(y.cpu().numpy(), g["tiny_out"]) < 1e-4
    m.close()


def test_per_layer_activations_tiny(td, orc, golden):
    """every block output of the tiny model vs the reference's forward hooks (fp32 mode, 5e-6 each)."""
    g = golden("unet")
    cfg = orc["unet"].tiny_config(64, 1)
    m = _model(td, orc, cfg, 77, "fp32")
    x = torch.from_numpy(orc["rng"].standard_normal(7, (2, 5, 16, 16))).cuda()
    m(x, torch.tensor([1.2, 0.3]), [torch.from_numpy(orc["rng"].standard_normal(8, (2, 58))).cuda()])
    emb = m.read_activation(2, 16, 16, "@emb").reshape(2, -1)
    assert rel_rms(emb.numpy(), g["tiny_emb"]) < 5e-6
    plan = orc["unet"].build_plan(cfg)
    n = 0
    for b in plan["enc"] + plan["dec"]:
        lab = b["name"] if b["kind"] == "conv" else b["name"] + (".attn_proj" if b["attn"] else ".conv_res1")
        a = m.read_activation(2, 16, 16, lab)
        assert rel_rms(a.numpy(), g["tiny_tap:" + b["name"]]) < 5e-6, b["name"]
        n += 1
    assert n == 21
    m.close()


def test_unet_glds_flavour_forced(td, orc, golden):
    """the LDS-DMA throughput kernel (normally chosen only for large pixel counts) forced onto every layer of the tiny models:
    same bf16 tolerance vs the reference, and close to the register-staged flavour (same maths, different summation order)."""
    from terrain_diffusion_amd.engine import get_engine
    g = golden("unet")
    eng = get_engine("cuda")
    outs = {}
    for flavour, min_wgs in (("tap", 1 << 30), ("glds", 0)):
        with pinned(eng, glds_min_wgs=min_wgs):
            cfg = orc["unet"].tiny_config(64, 1)
            m = _model(td, orc, cfg, 77, "bf16")
            x = torch.from_numpy(orc["rng"].standard_normal(7, (2, 5, 16, 16))).cuda()
            y = m(x, torch.tensor([1.2, 0.3]), [torch.from_numpy(orc["rng"].standard_normal(8, (2, 58))).cuda()])
            assert rel_rms(y.cpu().numpy(), g["tiny_out"]) < 2e-2, flavour
            outs[flavour] = y.cpu().numpy()
            m.close()
            cfg2 = orc["unet"].tiny_config(64, 2, attn_resolutions=[128])
            m2 = _model(td, orc, cfg2, 78, "bf16")
            x2 = torch.from_numpy(orc["rng"].standard_normal(9, (3, 5, 32, 32))).cuda()   # batch 3: ragged image groups (4 images per narrow tile)
            c2 = torch.from_numpy(orc["rng"].standard_normal(10, (1, 58))).expand(3, -1).contiguous().cuda()
            y2 = m2(x2, torch.tensor([0.9, 0.9, 0.9]), [c2])
            outs[flavour + "2"] = y2.cpu().numpy()
            m2.close()
    assert rel_rms(outs["glds"], outs["tap"]) < 1e-2
    assert rel_rms(outs["glds2"], outs["tap2"]) < 1e-2
    o2 = orc["unet"].OracleUnet(orc["unet"].tiny_config(64, 2, attn_resolutions=[128]), orc["unet"].synth_state_dict(orc["unet"].tiny_config(64, 2, attn_resolutions=[128]), seed=78))
    x2 = torch.from_numpy(orc["rng"].standard_normal(9, (3, 5, 32, 32)))
    ref = o2(x2, torch.tensor([0.9, 0.9, 0.9]), [torch.from_numpy(orc["rng"].standard_normal(10, (1, 58))).expand(3, -1)]).numpy()
    assert rel_rms(outs["glds2"], ref) < 2e-2


def test_synthetic_weights_match_oracle_recipe(td, orc):
    """the product's GPU-generated synthetic weights equal the oracle's CPU recipe (<= 1 ulp on normals)."""
    from terrain_diffusion_amd.synthetic import synthetic_state_dict, synthetic_cond_grid
    cfg = orc["unet"].tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype="bf16")
    a = synthetic_state_dict(m, seed=77)
    b = orc["unet"].synth_state_dict(cfg, seed=77)
    assert set(a) == set(b)
    for k in a:
        assert torch.allclose(a[k].float(), b[k].float(), rtol=2e-7, atol=0), k
    assert torch.allclose(synthetic_cond_grid(2, 3), orc["tiling"].synthetic_cond_grid(2, 3), rtol=2e-7, atol=0)
    m.close()


def test_independent_tiles_batch(td, orc, golden, base_models):
    """a batch of independent single tiles == the single-tile sampler run one at a time (bf16; tile 0 vs the reference golden)."""
    from oracle import tiling
    g = golden("sampling")
    sch = td.EDMDPMSolverMultistepScheduler()
    c0 = tiling.process_cond_img(tiling.synthetic_cond_grid(1, 1), torch.zeros(1, 5), torch.zeros(7), torch.ones(7), 0.0)
    c1 = tiling.process_cond_img(tiling.synthetic_cond_grid(1, 1, seed=5), torch.zeros(1, 5), torch.zeros(7), torch.ones(7), 0.0)
    out = td.sample_independent_tiles(base_models["bf16"], sch, [(0, 0), (4096, -640)], torch.cat([c0, c1]), steps=20)
    assert out.shape == (2, 5, 64, 64)
    assert rel_rms(out[0:1].cpu().numpy(), g["base_tile_steps20"]) < 2e-2
    solo = td.sample_independent_tiles(base_models["bf16"], sch, [(4096, -640)], c1, steps=20)
    assert rel_rms(solo.cpu().numpy(), out[1:2].cpu().numpy()) < 2e-2   # different kernel flavours/tiles at batch 1 vs 2: same maths


def test_sharded_sampling_simulated_ranks(td, orc):
    """2 and 4 'ranks' simulated on one GPU (same plan / seam lists / regional blend as the RCCL path, exchange done in memory):
    with the engine in batch-invariant mode the assembled canvas is BIT-identical to the unsharded sampler."""
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.parallel import ShardPlan, engine_fns, blend_region
    from oracle import tiling
    eng = get_engine("cuda")
    with pinned(eng, batch_invariant=1):
        cfg = orc["unet"].tiny_config(64, 1)
        m = _model(td, orc, cfg, 77, "bf16")
        sch = td.EDMDPMSolverMultistepScheduler()
        H, W, S, steps = 40, 56, 16, 5
        cond = tiling.synthetic_cond_grid(len(tiling.tile_starts(H, S, S // 2)), len(tiling.tile_starts(W, S, S // 2)))
        kw = dict(cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0), histogram_raw=torch.zeros(1, 5))
        ref = td.sample_base_diffusion(m, sch, (1, 5, H, W), cond, steps=steps, tile_size=S, noise_seed=7, **kw)
        # the sharded runs also use the two-lane sampler (engine option dual_stream: half-batches on two HIP streams, what bench.py switches on
        # for the strong-scaling workload): in batch-invariant mode the lane split must not change a bit either
        with pinned(eng, dual_stream=1, dual_stream_min_batch=2):
            for world in (2, 4):
                plan = ShardPlan(H, W, S, world)
                fns = engine_fns(m, sch, plan, cond, steps=steps, channels=5, noise_seed=7, noise_origin=(0, 0), max_batch=64, **kw)
                tiles = [fns[0](plan.windows[r]) for r in range(world)]
                full = torch.empty((5, H, W), device="cuda")
                for r in range(world):
                    have = {}
                    for w_ in plan.needed[r]:
                        o = plan.owner[w_]
                        have[w_] = tiles[o][plan.windows[o].index(w_)]
                    y0, y1, x0, x1 = plan.regions[r]
                    full[:, y0:y1, x0:x1] = blend_region(plan, r, have, fns[1], fns[2], 5, 1.0 / 0.5)
                assert torch.equal(full[None], ref), world
        m.close()


def test_infinite_latent_stage_vs_oracle(td, orc):
    """Lazy 2-phase InfiniteDiffusion latent stage (InfiniteTensor graph on the engine, negative coordinates) vs an explicit CPU
    restatement with the oracle U-Net: every window that touches the request, both phases, blend between phases."""
    from terrain_diffusion_amd.pipeline import build_latent_stage
    from oracle import tiling, rng
    cfg = orc["unet"].tiny_config(64, 1)
    sd_ = orc["unet"].synth_state_dict(cfg, seed=77)
    m = td.EDMUnet2D(**cfg, dtype="fp32").load_state_dict(sd_)
    om = orc["unet"].OracleUnet(cfg, sd_)
    T, S, C, sdat, seed = 16, 8, 5, 0.5, 11
    t1 = float(np.arctan(0.35 / 0.5))

    def cond_fn(ctxs):
        return torch.stack([torch.from_numpy(rng.standard_normal(5000 + 97 * c[1] + c[2], (58,))) for c in ctxs])

    lat = build_latent_stage(m, seed=seed, cond_fn=cond_fn, intermediate_ts=(t1,), tile=T, batch_size=7)
    y0, y1, x0, x1 = -4, 12, 6, 20
    got = lat[:, y0:y1, x0:x1]
    got = got[:-1] / got[-1:]
    # explicit restatement
    w = tiling.linear_weight_window(T)
    t0 = float(torch.atan(torch.tensor(80.0) / sdat))

    def touching(lo, hi):
        return [k for k in range(-10, 10) if k * S < hi and k * S + T > lo]

    memo = {}

    def window(phase, i, j):
        if (phase, i, j) in memo:
            return memo[(phase, i, j)]
        z = torch.from_numpy(rng.gaussian_noise_patch(seed + 5819 + phase, i * S, j * S, T, T, C, T, T))[None] * sdat
        if phase == 0:
            sample = torch.zeros(1, C, T, T)
            t = torch.tensor(t0)
        else:
            acc = torch.zeros(C + 1, T, T)
            for ii in touching(i * S, i * S + T):
                for jj in touching(j * S, j * S + T):
                    a, e, b, f_ = max(i * S, ii * S), min(i * S + T, ii * S + T), max(j * S, jj * S), min(j * S + T, jj * S + T)
                    acc[:, a - i * S:e - i * S, b - j * S:f_ - j * S] += window(phase - 1, ii, jj)[:, a - ii * S:e - ii * S, b - jj * S:f_ - jj * S]
            sample = (acc[:-1] / acc[-1:])[None] * sdat
            t = torch.tensor(t1)
        x_t = torch.cos(t) * sample + torch.sin(t) * z
        pred = -om(x_t / sdat, t.view(1), [cond_fn([(0, i, j)])])
        out = (torch.cos(t) * x_t - torch.sin(t) * sdat * pred)[0] / sdat
        memo[(phase, i, j)] = torch.cat([out * w[None], w[None]])
        return memo[(phase, i, j)]

    acc = torch.zeros(C + 1, y1 - y0, x1 - x0)
    for i in touching(y0, y1):
        for j in touching(x0, x1):
            a, e, b, f_ = max(y0, i * S), min(y1, i * S + T), max(x0, j * S), min(x1, j * S + T)
            acc[:, a - y0:e - y0, b - x0:f_ - x0] += window(1, i, j)[:, a - i * S:e - i * S, b - j * S:f_ - j * S]
    exp = acc[:-1] / acc[-1:]
    assert rel_rms(got.numpy(), exp.numpy()) < 1e-5
    m.close()


# ------------------------------------------------------------------------------------------- coarse / decoder roles
@pytest.mark.parametrize("dtype,tol", [("fp32", 5e-6), ("bf16", 2e-2)])
def test_coarse_and_decoder_forward(td, orc, golden, dtype, tol):
    from oracle.unet import COARSE_CONFIG, DECODER_CONFIG
    g = golden("stages")
    mc = td.EDMUnet2D(**COARSE_CONFIG, dtype=dtype).load_state_dict(orc["unet"].synth_state_dict(COARSE_CONFIG, seed=4321))
    x = torch.from_numpy(orc["rng"].standard_normal(41, (2, 11, 64, 64))).cuda()
    conds = [torch.from_numpy(orc["rng"].standard_normal(50 + i, (2,))) for i in range(5)]
    y = mc(x, torch.tensor([1.3, 0.4]), conds)
    assert y.shape == (2, 6, 64, 64) and rel_rms(y.cpu().numpy(), g["coarse_out"]) < tol
    if dtype == "fp32":
        assert rel_rms(mc.read_activation(2, 64, 64, "@emb").reshape(2, -1).numpy(), g["coarse_emb"]) < 5e-6
    mc.close()
    md = td.EDMUnet2D(**DECODER_CONFIG, dtype=dtype).load_state_dict(orc["unet"].synth_state_dict(DECODER_CONFIG, seed=2468))
    xd = torch.from_numpy(orc["rng"].standard_normal(43, (1, 5, 64, 64))).cuda()
    yd = md(xd, torch.tensor([1.5]), [])
    assert yd.shape == (1, 1, 64, 64) and rel_rms(yd.cpu().numpy(), g["decoder_out"]) < tol
    md.close()


def test_coarse_stage_loop_and_decoder_step_vs_oracle(td, orc):
    """The per-tile arithmetic of _coarse_inference (world_pipeline.py:928-951: 6 sample + 5 conditioning-image channels, 20-step
    DPM-Solver++ loop) and of _decoder_inference (world_pipeline.py:1221-1241: 1 sample + 4 upsampled-latent channels, one
    trig-flow step) through td_sample_edm_img / td_sample_consistency_img vs the oracle U-Net + oracle solver (fp32, 1e-5)."""
    from oracle.unet import COARSE_CONFIG, DECODER_CONFIG
    from oracle import schedule
    from terrain_diffusion_amd.sampling import sample_tiles_edm, consistency_step
    rng_, U = orc["rng"], orc["unet"]
    # ---- coarse
    sdc = U.synth_state_dict(COARSE_CONFIG, seed=4321)
    mc = td.EDMUnet2D(**COARSE_CONFIG, dtype="fp32").load_state_dict(sdc)
    oc = U.OracleUnet(COARSE_CONFIG, sdc)
    n, S, steps = 2, 16, 20
    sch = td.EDMDPMSolverMultistepScheduler()
    sch.set_timesteps(steps)
    cond_img = torch.from_numpy(rng_.standard_normal(61, (n, 5, S, S)))
    conds = [torch.full((n,), float(np.log(np.tan(np.arctan(0.5 + 0.1 * i)) / 8.0))) for i in range(5)]
    x0 = torch.from_numpy(rng_.standard_normal(62, (n, 6, S, S))) * sch.sigmas[0]
    x = x0.clone().cuda()
    sample_tiles_edm(mc, sch, x, mc.cond_rows(conds, n, "cuda"), steps, cond_img=cond_img.cuda().contiguous())
    sig, orders = schedule.karras_sigmas(steps)[0], schedule.solver_orders(steps)
    xr, m_prev = x0.clone(), None
    with torch.no_grad():
        for i in range(steps):
            xin = torch.cat([schedule.precondition_inputs(xr, sig[i]), cond_img], dim=1)
            F_ = oc(xin, schedule.trigflow_t(sig[i].view(-1).expand(n)), conds)
            xr, m_prev = schedule.dpm_step(sig, i, orders[i], xr, F_, m_prev)
    assert rel_rms(x.cpu().numpy(), xr.numpy()) < 1e-5
    mc.close()
    # ---- decoder
    sdd = U.synth_state_dict(DECODER_CONFIG, seed=2468)
    md = td.EDMUnet2D(**DECODER_CONFIG, dtype="fp32").load_state_dict(sdd)
    od = U.OracleUnet(DECODER_CONFIG, sdd)
    T = 64
    lat = torch.from_numpy(rng_.standard_normal(71, (1, 4, T // 8, T // 8)))
    up = torch.nn.functional.interpolate(lat, size=(T, T), mode="nearest")                       # world_pipeline.py:1224-1226
    z = torch.from_numpy(rng_.gaussian_noise_patch(42 + 5819, 3 * 48, -2 * 48, T, T, 1, T, T))[None]
    t = float(torch.atan(torch.tensor(80.0) / 0.5))
    out = consistency_step(md, t, 0.5, None, z.cuda().contiguous(), cond=None, cond_img=up.cuda().contiguous())
    with torch.no_grad():
        tt = torch.tensor(t)
        x_t = torch.cos(tt) * torch.zeros(1, 1, T, T) + torch.sin(tt) * (z * 0.5)
        pred = -od(torch.cat([x_t / 0.5, up], dim=1), tt.view(1), [])
        ref = torch.cos(tt) * x_t - torch.sin(tt) * 0.5 * pred
    assert rel_rms(out.cpu().numpy(), ref.numpy()) < 1e-5
    md.close()


def test_coarse_and_decoder_stage_builders_vs_reference_golden(td, orc, golden):
    """build_coarse_stage / build_decoder_stage (engine, fp32 mode) reproduce the windows that the reference's own _coarse_inference /
    _decoder_inference produced (tests/golden/stage_glue.npz), window by window and as the blended InfiniteTensor region."""
    from oracle.unet import COARSE_CONFIG, DECODER_CONFIG
    from oracle import stages
    from terrain_diffusion_amd.pipeline import build_coarse_stage, build_decoder_stage, pool_coarse_conditioning
    from terrain_diffusion_amd.infinite_tensor import InfiniteTensor, TensorWindow
    U = orc["unet"]
    g = golden("stage_glue")
    assert np.array_equal(pool_coarse_conditioning(torch.from_numpy(g["pool_in"]), 4, "max", "min").numpy(), g["pool4_max_min"])
    mc = td.EDMUnet2D(**COARSE_CONFIG, dtype="fp32").load_state_dict(U.synth_state_dict(COARSE_CONFIG, seed=4321))
    sch = td.EDMDPMSolverMultistepScheduler()
    for name, ctx, pool in [("coarse_ctx_0_1_m2_pool1", (0, 1, -2), 1), ("coarse_ctx_0_m1_0_pool2", (0, -1, 0), 2)]:
        cs = build_coarse_stage(mc, sch, seed=1234, cond_map_fn=stages.synthetic_coarse_map, coarse_means=g["coarse_means"], coarse_stds=g["coarse_stds"],
                                cond_snr=g["cond_snr"], coarse_pooling=pool, elev_coarse_pool_mode="max", p5_coarse_pool_mode="min")
        win = cs.f([ctx])[0]
        assert win.shape == (7, 64 // pool, 64 // pool) and np.array_equal(win[-1].numpy(), g[name][-1])
        assert rel_rms(win.numpy(), g[name]) < 1e-5, name
    # blended region == sum of the overlapping windows (stride 48 on tile 64): rows 48..63 x cols 16..95 are covered by windows
    # i, j in {0, 1} only (window k spans [48k, 48k + 64))
    cs = build_coarse_stage(mc, sch, seed=1234, cond_map_fn=stages.synthetic_coarse_map, coarse_means=g["coarse_means"], coarse_stds=g["coarse_stds"],
                            cond_snr=g["cond_snr"], batch_size=4)
    region = torch.as_tensor(cs[:, 48:64, 16:96])
    wins = {(i, j): cs.f([(0, i, j)])[0] for i in (0, 1) for j in (0, 1)}
    ref = torch.zeros(7, 16, 80)
    for (i, j), wv in wins.items():
        ys = slice(48 - 48 * i, 64 - 48 * i)
        xs0, xs1 = max(16, 48 * j), min(96, 48 * j + 64)
        ref[:, :, xs0 - 16:xs1 - 16] += wv[:, ys, xs0 - 48 * j:xs1 - 48 * j]
    assert torch.allclose(region, ref, rtol=1e-5, atol=1e-5)
    mc.close()
    # ---- decoder (tile 64, stride 48, latent compression 8): feed the golden latent window through an InfiniteTensor source
    md = td.EDMUnet2D(**DECODER_CONFIG, dtype="fp32").load_state_dict(U.synth_state_dict(DECODER_CONFIG, seed=2468))
    lat_win = torch.from_numpy(g["decoder_latents_in"])
    src = InfiniteTensor((6, None, None), lambda ctx: lat_win, TensorWindow(size=(6, 8, 8), stride=(6, 8, 8)), tensor_id="lat_src")
    ds = build_decoder_stage(md, src, seed=1234, tile_size=64, tile_stride=48)
    out = ds.f([(0, 2, -1)], [lat_win])[0]
    assert out.shape == (2, 64, 64) and rel_rms(out.numpy(), g["decoder_ctx_0_2_m1"]) < 1e-5
    ds2 = build_decoder_stage(md, src, seed=1234, tile_size=64, tile_stride=48, extra_ts=(float(torch.arctan(torch.tensor(0.065) / 0.5)),))
    out2 = ds2.f([(0, 2, -1)], [lat_win])[0]
    assert rel_rms(out2.numpy(), g["decoder_ctx_0_2_m1_two_phases"]) < 1e-5
    md.close()


def test_latent_glue_vs_reference_golden(td, orc, golden):
    """process_latent_conditioning (NaN handling, engine-side portable-RNG fill) and the per-window latent arithmetic of
    build_latent_stage(coarse=...) against the reference's own _process_latent_conditioning / _latent_inference outputs."""
    from oracle.unet import tiny_config
    from terrain_diffusion_amd.sampling import process_latent_conditioning
    from terrain_diffusion_amd.pipeline import build_latent_stage
    from terrain_diffusion_amd.infinite_tensor import InfiniteTensor, TensorWindow
    U = orc["unet"]
    g = golden("latent_glue")
    means, stds, hist = g["cond_means"], g["cond_stds"], torch.from_numpy(g["histogram_raw"])
    o1 = process_latent_conditioning(torch.from_numpy(g["plc_in_n1"]), hist, means, stds, 0.0, seed=1234, seed_offset=3 * 65536 - 2)
    assert np.allclose(o1.numpy(), g["plc_out_n1"], rtol=1e-6, atol=1e-6)
    o3 = process_latent_conditioning(torch.from_numpy(g["plc_in_n3"]), hist.expand(3, -1), means, stds, torch.zeros(3), seed=1234, seed_offset=7)
    assert np.allclose(o3.numpy(), g["plc_out_n3"], rtol=1e-6, atol=2e-6)      # the RNG-filled entries are <= 1 ulp from numba's
    cfg = tiny_config(64, 1)
    m = td.EDMUnet2D(**cfg, dtype="fp32").load_state_dict(U.synth_state_dict(cfg, seed=77))
    dummy = InfiniteTensor((7, None, None), lambda ctx: torch.ones(7, 4, 4), TensorWindow(size=(7, 4, 4), stride=(7, 4, 4)), tensor_id="coarse_dummy")
    lat = build_latent_stage(m, seed=1234, coarse=dummy, histogram_raw=hist, cond_means=means, cond_stds=stds)
    ctxs = [(0, 2, -3), (0, -1, 0)]
    conds = list(torch.from_numpy(g["latent_cond_windows"]))
    t0 = float(torch.atan(torch.tensor(80.0) / 0.5))
    p0 = lat.infer(0, t0, ctxs, None, conds)
    assert rel_rms(torch.stack(p0).numpy(), g["latent_phase0"]) < 1e-5
    p1 = lat.infer(1, float(torch.arctan(torch.tensor(0.35) / 0.5)), ctxs, list(torch.from_numpy(g["latent_phase0"])), conds)
    assert rel_rms(torch.stack(p1).numpy(), g["latent_phase1_from_phase0_windows"]) < 1e-5
    m.close()


def test_cascade_coarse_latent_decoder_vs_oracle_chain(td, orc):
    """The three engine-backed stages chained exactly as WorldPipeline wires them (coarse (7,*,*) -> latent windows through the
    (7,4,4)/offset -1 conditioning window, two blended trig-flow phases -> decoder through the (6,T/8,T/8) window), against the same
    InfiniteTensor graph whose window functions are the CPU oracle's (oracle/stages.py, pinned to the reference window by window).
    fp32 engine mode; a 40x40 region of the decoder output pulls 4 coarse, 34 latent and 4 decoder windows through the graph."""
    from oracle import stages
    from oracle.unet import COARSE_CONFIG, DECODER_CONFIG, tiny_config
    from terrain_diffusion_amd.pipeline import build_coarse_stage, build_latent_stage, build_decoder_stage
    from terrain_diffusion_amd.infinite_tensor import InfiniteTensor, TensorWindow
    U = orc["unet"]
    seed = 4242
    means6 = [0.3, -0.2, 0.1, 0.0, 0.4, -0.1]; stds6 = [1.5, 0.8, 1.2, 0.9, 1.1, 0.7]; snr = [0.5, 0.4, 0.6, 0.3, 0.8]
    hist = torch.tensor([[0.1, 0.3, 0.2, 0.25, 0.15]])
    cm, cs_ = [0.2, 0.1, 0.0, -0.1, 0.3, 0.0, 0.66], [1.2, 1.1, 0.9, 1.0, 1.3, 0.8, 0.47]
    bcfg = tiny_config(64, 1)
    sdc, sdb, sdd = U.synth_state_dict(COARSE_CONFIG, seed=1), U.synth_state_dict(bcfg, seed=2), U.synth_state_dict(DECODER_CONFIG, seed=3)
    # ---- engine graph
    mc = td.EDMUnet2D(**COARSE_CONFIG, dtype="fp32").load_state_dict(sdc)
    mb = td.EDMUnet2D(**bcfg, dtype="fp32").load_state_dict(sdb)
    md = td.EDMUnet2D(**DECODER_CONFIG, dtype="fp32").load_state_dict(sdd)
    coarse = build_coarse_stage(mc, td.EDMDPMSolverMultistepScheduler(), seed=seed, cond_map_fn=stages.synthetic_coarse_map, coarse_means=means6,
                                coarse_stds=stds6, cond_snr=snr)
    lat = build_latent_stage(mb, seed=seed, coarse=coarse, histogram_raw=hist, cond_means=cm, cond_stds=cs_)
    dec = build_decoder_stage(md, lat, seed=seed, tile_size=64, tile_stride=48)
    got = torch.as_tensor(dec[:, 4:44, 2:42])
    # ---- the same graph on the oracle
    oc, ob, od = U.OracleUnet(COARSE_CONFIG, sdc), U.OracleUnet(bcfg, sdb), U.OracleUnet(DECODER_CONFIG, sdd)
    ocoarse = InfiniteTensor((7, None, None), lambda ctx: stages.coarse_inference(oc, ctx, seed=seed, cond_map_fn=stages.synthetic_coarse_map, means=means6,
                             stds=stds6, cond_snr=snr), TensorWindow(size=(7, 64, 64), stride=(7, 48, 48)), tensor_id="o_coarse")
    lwin, cwin = TensorWindow(size=(6, 64, 64), stride=(6, 32, 32)), TensorWindow(size=(7, 4, 4), stride=(7, 1, 1), offset=(0, -1, -1))
    kw = dict(seed=seed, histogram_raw=hist, cond_means=cm, cond_stds=cs_)
    t0, t1 = torch.atan(torch.tensor(80.0) / 0.5), torch.arctan(torch.tensor(0.35) / 0.5)
    ol0 = InfiniteTensor((6, None, None), lambda ctx, c: stages.latent_inference(ob, [ctx], None, [c], t0, seed_offset=5819, **kw)[0], lwin,
                         args=(ocoarse,), args_windows=(cwin,), tensor_id="o_lat0")
    ol1 = InfiniteTensor((6, None, None), lambda ctx, s, c: stages.latent_inference(ob, [ctx], [s], [c], t1, seed_offset=5820, **kw)[0], lwin,
                         args=(ol0, ocoarse), args_windows=(lwin, cwin), tensor_id="o_lat1")
    odec = InfiniteTensor((2, None, None), lambda ctx, l: stages.decoder_inference(od, ctx, torch.as_tensor(l), seed=seed, tile_size=64, tile_stride=48),
                          TensorWindow(size=(2, 64, 64), stride=(2, 48, 48)), args=(ol1,), args_windows=(TensorWindow(size=(6, 8, 8), stride=(6, 6, 6)),),
                          tensor_id="o_dec")
    ref = torch.as_tensor(odec[:, 4:44, 2:42])
    assert got.shape == ref.shape == (2, 40, 40)
    assert torch.equal(got[1], ref[1]) or torch.allclose(got[1], ref[1], rtol=1e-6, atol=1e-7)          # blend weights
    assert rel_rms((got[0] / got[1]).numpy(), (ref[0] / ref[1]).numpy()) < 1e-4
    for m_ in (mc, mb, md):
        m_.close()


def test_device_resident_cascade_matches_host_resident(td, orc, monkeypatch):
    """SURVEY.md Q15 / VERDICT round 1 item 9: the same coarse -> latent (two blended phases) -> decoder graph with every window kept in HBM
    (DeviceWindowTensor + DeviceTileStore, regions assembled by the engine's blend kernel) against the host-resident graph (the reference's
    `.cpu()` after every window).  Same window arithmetic, so: weight channel bit-identical, values to fp32 rounding of the blend (the
    kernel multiplies and adds per window in the same order; torch's host path rounds the product separately).  No tensor crosses to the
    host between the stages, and a store capped below the working set evicts, recomputes and reproduces the same bits."""
    from oracle import stages
    from oracle.unet import COARSE_CONFIG, DECODER_CONFIG, tiny_config
    from terrain_diffusion_amd.pipeline import build_coarse_stage, build_latent_stage, build_decoder_stage
    from terrain_diffusion_amd.infinite_tensor import DeviceTileStore
    U = orc["unet"]
    seed = 4242
    means6 = [0.3, -0.2, 0.1, 0.0, 0.4, -0.1]; stds6 = [1.5, 0.8, 1.2, 0.9, 1.1, 0.7]; snr = [0.5, 0.4, 0.6, 0.3, 0.8]
    hist = torch.tensor([[0.1, 0.3, 0.2, 0.25, 0.15]])
    cm, cs_ = [0.2, 0.1, 0.0, -0.1, 0.3, 0.0, 0.66], [1.2, 1.1, 0.9, 1.0, 1.3, 0.8, 0.47]
    bcfg = tiny_config(64, 1)
    mc = td.EDMUnet2D(**COARSE_CONFIG, dtype="fp32").load_state_dict(U.synth_state_dict(COARSE_CONFIG, seed=1))
    mb = td.EDMUnet2D(**bcfg, dtype="fp32").load_state_dict(U.synth_state_dict(bcfg, seed=2))
    md = td.EDMUnet2D(**DECODER_CONFIG, dtype="fp32").load_state_dict(U.synth_state_dict(DECODER_CONFIG, seed=3))

    def graph(resident, store=None):
        kw = dict(device_resident=resident, tile_store=store) if resident else {}
        coarse = build_coarse_stage(mc, td.EDMDPMSolverMultistepScheduler(), seed=seed, cond_map_fn=stages.synthetic_coarse_map, coarse_means=means6,
                                    coarse_stds=stds6, cond_snr=snr, **kw)
        lat = build_latent_stage(mb, seed=seed, coarse=coarse, histogram_raw=hist, cond_means=cm, cond_stds=cs_, **kw)
        return build_decoder_stage(md, lat, seed=seed, tile_size=64, tile_stride=48, **kw), lat, coarse
    host = torch.as_tensor(graph(False)[0][:, 4:44, 2:42])
    calls = []
    real_cpu = torch.Tensor.cpu
    dec, lat, coarse = graph(True, DeviceTileStore())   # (building the stages fetches their blend windows once: setup, not data flow)
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append(tuple(self.shape)), real_cpu(self, *a, **k))[1])
    got = dec[:, 4:44, 2:42]
    monkeypatch.setattr(torch.Tensor, "cpu", real_cpu)
    big = [s for s in calls if int(np.prod(s)) > 64]   # scalars / tiny index tensors aside, no window or region crossed to the host
    assert got.is_cuda and not big, big
    assert all(t.is_cuda for t in dec.tile_store._d.values())
    assert torch.equal(got[1].cpu(), host[1])
    assert rel_rms((got[0] / got[1]).cpu().numpy(), (host[0] / host[1]).numpy()) < 1e-6
    # streaming eviction: a store that holds ~3 decoder windows; every stage evicts and recomputes.  Recomputed windows ride in batches of a
    # different size, so bit-identity needs the engine's batch-invariant mode (kernel flavour / K order independent of the batch); without it
    # the recomputed windows agree to rounding.
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    small = DeviceTileStore(cache_size_bytes=3 * 2 * 64 * 64 * 4)
    got2 = graph(True, small)[0][:, 4:44, 2:42]
    assert small.evictions > 0
    assert rel_rms(got2.cpu().numpy(), got.cpu().numpy()) < 1e-5
    with pinned(eng, batch_invariant=1):
        ref_inv = graph(True, DeviceTileStore())[0][:, 4:44, 2:42]
        small = DeviceTileStore(cache_size_bytes=3 * 2 * 64 * 64 * 4)
        got_inv = graph(True, small)[0][:, 4:44, 2:42]
        assert small.evictions > 0 and torch.equal(got_inv, ref_inv)
    for m_ in (mc, mb, md):
        m_.close()


class _ArraySource:
    """sliceable stand-in for a stage tensor: a fixed array addressed in absolute coordinates (origin at `off`)."""

    def __init__(self, arr, off):
        self.arr, self.off = arr, off

    def __getitem__(self, idx):
        c, ys, xs = idx
        return self.arr[c, ys.start + self.off:ys.stop + self.off, xs.start + self.off:xs.stop + self.off]


def test_output_composition_elev_and_climate_vs_oracle(td, orc):
    """WorldPipeline._compute_elev / _compute_climate on the engine (tap-table gather kernels for the bilinear / anti-aliased
    resize and the Gaussian blur, fused de-normalise + add + signed square) against the CPU oracle (oracle/compose.py: F.interpolate / conv2d --
    torchvision's operators are parity-unpinned here, see the module headers).  Boxes straddle the origin and are not multiples of the
    latent compression; elevations are ~1e3 m, tolerance 1e-5 relative RMS."""
    from oracle import compose, rng
    from terrain_diffusion_amd import composition as cp
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    off = 1024
    g = torch.Generator().manual_seed(5)
    wres = torch.rand(2048, 2048, generator=g) * 1.5 + 0.2
    smooth = torch.from_numpy(rng.standard_normal(71, (2048 // 8, 2048 // 8)))
    smooth = torch.nn.functional.interpolate(smooth[None, None], scale_factor=8, mode="bicubic")[0, 0]
    res = torch.stack([(torch.randn(2048, 2048, generator=g) * 0.8 + smooth) * wres, wres])
    wlat = torch.rand(256, 256, generator=g) + 0.5
    lat = torch.cat([torch.randn(5, 256, 256, generator=g) * wlat, wlat[None]])
    R, L = _ArraySource(res, off), _ArraySource(lat, off // 8)
    for (i1, j1, i2, j2) in ((-37, 5, 220, 301), (100, -260, 356, -4), (3, 3, 67, 131)):
        ref = compose.compute_elev(R, L, i1, j1, i2, j2, 8, 0.0, 1.1678)
        got = cp.compute_elev(eng, R, L, i1, j1, i2, j2, 8, 0.0, 1.1678)
        assert got.is_cuda and got.shape == ref.shape == (i2 - i1, j2 - j1)
        err = rel_rms(got.cpu().numpy(), ref.numpy())
        print(f"compute_elev box {(i1, j1, i2, j2)}: rel-RMS vs oracle {err:.2e}, |elev| max {float(ref.abs().max()):.0f} m")
        assert err < 1e-5
    wc = torch.rand(256, 256, generator=g) + 0.5
    cmap = torch.randn(6, 256, 256, generator=g)
    cmap[0] = cmap[0] * 20 + 10        # sqrt-elevation channel: mixed land / ocean
    cmap[2] = cmap[2] * 8 + 12
    coarse = _ArraySource(torch.cat([cmap * wc, wc[None]]), 128)
    i1, j1, i2, j2 = -300, 40, 212, 700
    elev = compose.compute_elev(R, L, i1, j1, i2, j2, 8, 0.0, 1.1678)
    ref = compose.compute_climate(coarse, i1, j1, i2, j2, elev, 8)
    got = cp.compute_climate(coarse, i1, j1, i2, j2, elev.cuda(), 8)
    assert got.shape == ref.shape == (5, 512, 660)
    assert rel_rms(got.cpu().numpy(), ref.numpy()) < 1e-5


def test_bounded_decoder_and_coarse_twins_vs_reference(td, golden, orc):
    """SURVEY.md §2 ★ components: sample_decoder_diffusion_tiled / sample_decoder_consistency_tiled /
    sample_coarse_tiled (training/evaluation/sample_diffusion_decoder.py:44-211, sample_coarse.py:29-125) on the engine, against outputs of
    the reference functions themselves (tests/golden/bounded_twins.npz, fp32 engine mode, tolerance 1e-5 rel-RMS).
    Finding while generating the fixtures: the reference's decoder-diffusion and coarse samplers set the scheduler's timesteps once, outside
    their tile loops, so the step index runs off the sigma table on the second tile (IndexError, dpmsolver.py:512); only their single-tile
    form runs.  The consistency sampler is fine with many tiles.  The engine twins run any number of tiles; the multi-tile diffusion case is
    checked against a manual blend of single-tile runs."""
    from oracle import rng, tiling
    U = orc["unet"]
    g = golden("bounded_twins")
    md = td.EDMUnet2D(**U.DECODER_CONFIG, dtype="fp32").load_state_dict(U.synth_state_dict(U.DECODER_CONFIG, seed=2468))
    sch = td.EDMDPMSolverMultistepScheduler(sigma_min=0.002, sigma_max=80.0, sigma_data=0.5)
    noise = torch.from_numpy(rng.standard_normal(901, (2, 1, 40, 56)))
    cond = torch.from_numpy(rng.standard_normal(902, (2, 4, 40, 56)))
    sq = torch.from_numpy(rng.standard_normal(908, (2, 1, 40, 40)))
    csq = torch.from_numpy(rng.standard_normal(909, (2, 4, 40, 40)))
    got = td.sample_decoder_diffusion_tiled(md, sch, csq, sq * 80.0, num_steps=6)
    assert rel_rms(got.cpu().numpy(), g["dec_diffusion_b2_40x40_steps6"]) < 1e-5
    cond_lo = torch.from_numpy(rng.standard_normal(903, (2, 4, 16, 16)))
    noise32 = torch.from_numpy(rng.standard_normal(904, (2, 1, 32, 32)))
    got = td.sample_decoder_diffusion_tiled(md, sch, cond_lo, noise32 * 80.0, num_steps=4)
    assert rel_rms(got.cpu().numpy(), g["dec_diffusion_b2_32x32_condlo_steps4"]) < 1e-5
    sch.set_timesteps(20)
    got = td.sample_decoder_consistency_tiled(md, sch, cond, noise, 32, 24)
    assert rel_rms(got.cpu().numpy(), g["dec_consistency_b2_40x56_t32_s24_1step"]) < 1e-5
    got = td.sample_decoder_consistency_tiled(md, sch, cond, noise, 32, 24, intermediate_t=[float(np.arctan(0.35 / 0.5)), 0.2])
    assert rel_rms(got.cpu().numpy(), g["dec_consistency_b2_40x56_t32_s24_3step"]) < 1e-5
    # multi-tile diffusion (the reference cannot run it): equals the blend of the same tiles sampled one canvas at a time
    multi = td.sample_decoder_diffusion_tiled(md, sch, cond, noise * 80.0, 32, 24, num_steps=5).cpu()
    w = tiling.linear_weight_window(32)
    acc, wsum = torch.zeros(2, 1, 40, 56), torch.zeros(40, 56)
    for i0 in tiling.tile_starts(40, 32, 24):
        for j0 in tiling.tile_starts(56, 32, 24):
            one = td.sample_decoder_diffusion_tiled(md, sch, cond[..., i0:i0 + 32, j0:j0 + 32], noise[..., i0:i0 + 32, j0:j0 + 32] * 80.0, num_steps=5).cpu()
            acc[..., i0:i0 + 32, j0:j0 + 32] += one * w
            wsum[i0:i0 + 32, j0:j0 + 32] += w
    assert rel_rms(multi.numpy(), (acc / wsum).numpy()) < 1e-6
    md.close()
    # coarse twin, noises pinned to what the fixture generator fed the reference
    mc = td.EDMUnet2D(**U.COARSE_CONFIG, dtype="fp32").load_state_dict(U.synth_state_dict(U.COARSE_CONFIG, seed=4321))
    cimg = torch.from_numpy(rng.standard_normal(905, (1, 5, 64, 64)))
    snr = torch.tensor([[0.5, 0.4, 0.6, 0.3, 0.8]])
    got = td.sample_coarse_tiled(mc, sch, cimg, snr, steps=5, cond_noise=torch.from_numpy(rng.standard_normal(906, (1, 5, 64, 64))),
                                 init_noise=[torch.from_numpy(rng.standard_normal(907, (1, 6, 64, 64)))])
    assert rel_rms(got.cpu().numpy(), g["coarse_64x64_steps5"]) < 1e-5
    # two tiles, portable default noises: finite, deterministic, and the first tile's private corner equals the single-tile run on that crop
    big = torch.from_numpy(rng.standard_normal(910, (1, 5, 112, 64)))
    a = td.sample_coarse_tiled(mc, sch, big, snr, steps=5, tile_size=64, tile_stride=48, noise_seed=5)
    b = td.sample_coarse_tiled(mc, sch, big, snr, steps=5, tile_size=64, tile_stride=48, noise_seed=5)
    assert a.shape == (1, 6, 112, 64) and torch.isfinite(a).all() and torch.equal(a, b)
    mc.close()


def test_sharded_two_phase_consistency_on_engine(td, orc):
    """The multi-phase sharded sampler (parallel.sample_base_consistency_sharded: one window exchange per trig-flow phase, the next phase cut from
    each rank's own blended box) on the ENGINE: one rank == td.sample_base_consistency, and two ranks simulated in memory (same plans, seam lists
    and regional blends as the RCCL path) assemble the same canvas -- bit for bit in batch-invariant mode."""
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.parallel import ShardPlan, consistency_engine_fns, blend_region, sample_base_consistency_sharded
    from oracle import tiling
    eng = get_engine("cuda")
    with pinned(eng, batch_invariant=1):
        cfg = orc["unet"].tiny_config(64, 1)
        m = _model(td, orc, cfg, 77, "bf16")
        sch = td.EDMDPMSolverMultistepScheduler()
        H, W, S = 40, 56, 16
        cond = tiling.synthetic_cond_grid(len(tiling.tile_starts(H, S, S // 2)), len(tiling.tile_starts(W, S, S // 2)))
        kw = dict(cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0), histogram_raw=torch.zeros(1, 5))
        it = float(np.arctan(0.35 / 0.5))
        ref = td.sample_base_consistency(m, sch, (1, 5, H, W), cond, intermediate_t=it, tile_size=S, noise_seed=7, **kw)
        one = sample_base_consistency_sharded(m, sch, (1, 5, H, W), cond, intermediate_t=it, tile_size=S, noise_seed=7, gather_to=0, **kw)
        assert torch.equal(one, ref)
        for world in (2, 4):
            own, ext = ShardPlan(H, W, S, world), ShardPlan(H, W, S, world, extended=True)
            step_fn, blend_fn, norm_fn = consistency_engine_fns(m, own, cond, channels=5, noise_seed=7, noise_origin=(0, 0), max_batch=64, sigma_data=0.5, **kw)
            ts = (float(torch.atan(torch.tensor(80.0) / 0.5)), float(torch.tensor(it, dtype=torch.float32)))
            prev = [None] * world
            full = torch.empty((5, H, W), device="cuda")
            for k, t in enumerate(ts):
                last = k == len(ts) - 1
                plan = own if last else ext
                outs = [step_fn(own.windows[r], k, t, prev[r]) for r in range(world)]
                for r in range(world):
                    have = {w_: outs[plan.owner[w_]][own.windows[plan.owner[w_]].index(w_)] for w_ in plan.needed[r]}
                    region = blend_region(plan, r, have, blend_fn, norm_fn, 5, 2.0 if last else 1.0)
                    y0, y1, x0, x1 = plan.regions[r]
                    if last:
                        full[:, y0:y1, x0:x1] = region
                    else:
                        prev[r] = torch.stack([region[:, own.h_starts[ic] - y0:own.h_starts[ic] - y0 + S, own.w_starts[jc] - x0:own.w_starts[jc] - x0 + S]
                                               for ic, jc in own.windows[r]]).contiguous()
            assert torch.equal(full[None], ref), world
        m.close()
