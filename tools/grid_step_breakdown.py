#!/usr/bin/env python
"""Where a grid8 bench step goes on the host's clock: python tools/grid_step_breakdown.py [--steps 3] [--warmup 2]

The default bench workload (bench.py: 8x8 grid of 64x64 windows, 20 solver steps, bf16), run with engine option grid_fused = 0 (four engine calls per
window batch with the conditioning rows built on the host in between) and grid_fused = 1 (one td_sample_grid_batch call).  Every engine call is
synchronous (option "async" = 0: complete on return), so a host clock around a call is the time the GPU and the host spent on it.  Prints, per timed
step, the milliseconds in each part and in the rest of the step (Python glue: tile lists, torch.zeros of the canvas, set_timesteps)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import bench
    import terrain_diffusion_amd as td
    from terrain_diffusion_amd import sampling as S
    from terrain_diffusion_amd import noise as N
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.synthetic import synthetic_state_dict, synthetic_cond_grid

    dev = "cuda:0"
    eng = get_engine(dev)
    model = td.EDMUnet2D(**bench.BASE_CONFIG, dtype="bf16", device=dev)
    model.load_state_dict(synthetic_state_dict(model, seed=1234))
    sch = td.EDMDPMSolverMultistepScheduler(sigma_min=0.002, sigma_max=80.0, sigma_data=0.5)
    nt = len(S._tile_starts(288, 64, 32))
    cond = synthetic_cond_grid(nt, nt, device=dev)
    kw = dict(cond_means=torch.zeros(7), cond_stds=torch.ones(7), noise_level=torch.tensor(0.0), histogram_raw=torch.zeros(1, 5), steps=20, tile_size=64)

    acc = {}

    def timed(name, fn, after=None):
        def wrapper(*a, **k):
            t0 = time.perf_counter()
            r = fn(*a, **k)
            if after is not None:
                r = after(r)
            acc[name] = acc.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return r
        return wrapper

    class LibProxy:
        """the ctypes library with td_sample_grid_batch on the clock"""

        def __init__(self, real):
            self._real = real
            self.td_sample_grid_batch = timed("one call", real.td_sample_grid_batch)

        def __getattr__(self, name):
            return getattr(self._real, name)

    real_lib = S.lib()
    proxy = LibProxy(real_lib)
    N.gaussian_noise_patches = timed("noise", N.gaussian_noise_patches)
    S._tile_conditioning = timed("conditioning", S._tile_conditioning, after=lambda r: r.to(dev).contiguous())   # with its upload, as the sampler does next
    S.sample_tiles_edm = timed("sampler", S.sample_tiles_edm)
    S.blend_windows = timed("blend", S.blend_windows)
    S.blend_normalize = timed("normalise", S.blend_normalize)
    S.lib = lambda: proxy

    def step(i):
        out = td.sample_base_diffusion(model, sch, (1, 5, 288, 288), cond, noise_seed=42 + 5819, noise_origin=(0, 4096 * i), **kw)
        eng.synchronize()
        torch.cuda.synchronize()
        return out

    for fused, parts in ((0, ("noise", "conditioning", "sampler", "blend", "normalise")), (1, ("one call", "normalise"))):
        eng.set_option("grid_fused", fused)
        for i in range(args.warmup):
            step(i)
        print(f"grid_fused={fused}: ms per step -- " + ", ".join(parts) + ", rest, total")
        for i in range(args.steps):
            acc.clear()
            t0 = time.perf_counter()
            step(args.warmup + i)
            total = (time.perf_counter() - t0) * 1e3
            vals = [acc.get(p, 0.0) for p in parts]
            print(f"  step {i}: " + "  ".join(f"{p} {v:.3f}" for p, v in zip(parts, vals)) + f"  rest {total - sum(vals):.3f}  total {total:.3f}", flush=True)
    eng.set_option("grid_fused", 1)


if __name__ == "__main__":
    main()
