"""Generates tests/golden/sampler_args.npz by RUNNING THE REFERENCE'S OWN MODULES: the bounded samplers with the three arguments the engine
used to refuse -- autoguidance on a model with conditioning-image channels, score scaling, custom weight windows.

    python tests/golden/make_sampler_args_golden.py

Needs the reference checkout (see make_golden.py, whose shim and helpers it imports unchanged).  Outputs and tiny inputs only; every model and
every input is reproducible from the portable RNG (oracle/rng.py) and oracle.unet.synth_state_dict by seed.

Each diffusion case is also run with the reference's models and inputs in float64; `e_ref:<case>` = rel-RMS(fp32 run, float64 run) is how well
the reference's own fp32 arithmetic is conditioned on that case, and is asserted <= 1e-6: the engine's fp32-mode bound of 1e-5 rel-RMS against
these goldens is then 10x or more above the reference's own rounding.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True          # tests/golden/ is not git-ignored: leave no cache of make_golden.py there
from make_golden import REF, _ref_model, extract_functions, install_shim, save  # noqa: E402

SCHED = (0.002, 80.0, 0.5)
DEC_STEPS = 5
DEC_CASES = {"plain": (1.0, 1.0), "guided": (1.5, 1.0), "alpha1p1": (1.0, 1.1), "alpha1p3": (1.0, 1.3), "guided_alpha1p1": (1.5, 1.1)}   # (guidance, alpha)
SCORE_SIGMAS = (80.0, 3.0, 0.5, 0.002)
SCORE_ALPHAS = (0.8, 1.1, 1.3)


def window_constant(size, device, dtype):
    return torch.ones(1, 1, size, size, device=device, dtype=dtype)


def window_sin2(size, device, dtype):
    """(sin^2(pi (i + 1/2) / S) + 0.05) outer-squared: strictly positive, not separable into the linear window"""
    i = torch.arange(size, device=device, dtype=dtype)
    r = torch.sin(math.pi * (i + 0.5) / size) ** 2 + 0.05
    return (r[:, None] * r[None, :])[None, None]


WINDOWS = {"const": window_constant, "sin2": window_sin2}


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def decoder_configs():
    from oracle.unet import DECODER_CONFIG
    main = dict(DECODER_CONFIG, layers_per_block=1)
    # the guide is the smaller model of the pair: the main model's 64-128-192-256 channels against 64-128-128-128.  (A guide of model_channels = 32 runs in
    # the reference but not in the engine, whose blocks take multiples of 64 channels; the narrowing is moved to the deep levels.)
    return main, dict(main, model_channel_mults=[1, 2, 2, 2])


def main():
    assert os.path.isdir(REF), "golden generation needs the reference checkout"
    install_shim()
    torch.manual_seed(0)
    from terrain_diffusion.scheduler.dpmsolver import EDMDPMSolverMultistepScheduler
    from terrain_diffusion.training.evaluation import sample_diffusion_decoder as sdd, sample_diffusion_base as sdb
    from oracle import rng, tiling
    from oracle.unet import synth_state_dict, tiny_config
    out = {}
    cfg_m, cfg_g = decoder_configs()
    md = _ref_model(cfg_m, synth_state_dict(cfg_m, seed=11))
    mg = _ref_model(cfg_g, synth_state_dict(cfg_g, seed=12))
    md64, mg64 = _ref_model(cfg_m, synth_state_dict(cfg_m, seed=11)).double(), _ref_model(cfg_g, synth_state_dict(cfg_g, seed=12)).double()
    sch = EDMDPMSolverMultistepScheduler(sigma_min=SCHED[0], sigma_max=SCHED[1], sigma_data=SCHED[2])

    # ---- decoder diffusion: b = 2, 32 x 32, one tile, 5 steps
    noise = torch.from_numpy(rng.standard_normal(921, (2, 1, 32, 32))) * 80.0
    cimg = torch.from_numpy(rng.standard_normal(922, (2, 4, 32, 32)))
    for name, (gs, alpha) in DEC_CASES.items():
        y = sdd.sample_decoder_diffusion_tiled(md, sch, cimg, noise, num_steps=DEC_STEPS, guidance_model=mg, guidance_scale=gs, score_scaling=alpha)
        y64 = sdd.sample_decoder_diffusion_tiled(md64, sch, cimg.double(), noise.double(), num_steps=DEC_STEPS, guidance_model=mg64, guidance_scale=gs, score_scaling=alpha)
        assert y.dtype == torch.float32 and y64.dtype == torch.float64
        e = rel_rms(y.numpy(), y64.numpy())
        print(f"decoder diffusion {name}: e_ref = {e:.2e}")
        assert e <= 1e-6, (name, e)
        out["dec_diffusion:" + name], out["e_ref:" + name] = y.numpy(), np.float64(e)

    # ---- _scale_score alone (pure function) on a seeded pair
    ns = extract_functions(os.path.join(REF, "terrain_diffusion/training/evaluation/sample_diffusion_decoder.py"), {"_scale_score"}, {"torch": torch})
    xs = torch.from_numpy(rng.standard_normal(923, (2, 3, 8, 8)))
    fs = torch.from_numpy(rng.standard_normal(924, (2, 3, 8, 8)))
    for si, sigma in enumerate(SCORE_SIGMAS):
        sig32 = torch.tensor(sigma, dtype=torch.float32)
        x = xs * torch.sqrt(sig32 * sig32 + 0.25)          # a sample at noise level sigma: data of scale sigma_data plus sigma noise
        out[f"score_x:{si}"] = x.numpy()
        for alpha in SCORE_ALPHAS:
            out[f"score:{si}:{alpha}"] = ns["_scale_score"](fs, x, sig32, 0.5, alpha=alpha).numpy()
    out["score_f"] = fs.numpy()

    # ---- decoder consistency: b = 2, 40 x 56, tiles 32 stride 24, one and three steps, both windows
    cn = torch.from_numpy(rng.standard_normal(925, (2, 1, 40, 56)))
    cc = torch.from_numpy(rng.standard_normal(926, (2, 4, 40, 56)))
    sch.set_timesteps(20)
    for wname, wfn in WINDOWS.items():
        out[f"dec_consistency_1step:{wname}"] = sdd.sample_decoder_consistency_tiled(md, sch, cc, cn, 32, 24, weight_window_fn=wfn).numpy()
        out[f"dec_consistency_3step:{wname}"] = sdd.sample_decoder_consistency_tiled(md, sch, cc, cn, 32, 24, intermediate_t=[float(np.arctan(0.35 / 0.5)), 0.2],
                                                                                      weight_window_fn=wfn).numpy()

    # ---- base diffusion: tiny base model, 32 x 32, tile 16, 6 steps, sin2 window (torch.randn replaced by the portable field, as gen_sampling does)
    cfg_b = tiny_config(64, 1)
    mb = _ref_model(cfg_b, synth_state_dict(cfg_b, seed=77))
    cond = tiling.synthetic_cond_grid(3, 3)
    base_kw = dict(cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0), histogram_raw=torch.zeros(1, 5))
    real_randn = torch.randn
    torch.randn = lambda shape, generator=None, device=None, dtype=None: tiling.initial_noise_field(42 + 5819, 32, 32, 5)
    try:
        out["base_diffusion:sin2"] = sdb.sample_base_diffusion(mb, sch, (1, 5, 32, 32), cond, steps=6, tile_size=16, weight_window_fn=window_sin2, **base_kw).numpy()
    finally:
        torch.randn = real_randn
    # ---- base consistency: two phases, constant window
    bn = [tiling.initial_noise_field(42 + 5819 + k, 32, 32, 5) for k in range(2)]
    out["base_consistency_2phase:const"] = sdb.sample_base_consistency(mb, sch, (1, 5, 32, 32), cond, intermediate_t=float(np.arctan(0.35 / 0.5)), tile_size=16,
                                                                        noise=bn, weight_window_fn=window_constant, **base_kw).detach().numpy()
    save("sampler_args", **out)


if __name__ == "__main__":
    main()
