"""Device time of the validation-objective library (terrain_diffusion_amd.objective, libtd_objective.so) per entry point, on the two batch shapes
the reference trains on -- 256 items of 5 x 64 x 64 with 2 conditioning channels (the base model's latents) and 256 x 1 x 96 x 96 (the decoder's
residual) --, and the same quantities composed from plain torch operations on the same device tensors in the same process.  Prints one JSON
line per measurement; every line carries the hash of the library's sources.

    python tools/objective_bench.py [--items 256] [--reps 10] [--warmup 2] [--rounds 3]

Each measurement is --reps back-to-back enqueue-only calls between two events on the engine's stream (every input is on the device before the
timing starts, so a host enqueue gap would be included), repeated --rounds times: the median per call with the least and the largest round.
Beside each time stand the bytes per ELEMENT of `images` the kernel must move as it is built, the GB/s that gives and its share of the HBM rate:
  levels         with scale_sigma 8 per element of the listed channels (two float64 passes over them), else launch-bound: N rows of 6 values;
  noise          20 + 8 Cc / C: images and noise in, x and v out (5 planes of 4 B with the x of the image channels), cond_img in and out;
  logvar         reads K values three times per item and writes one: launch-bound;
  sqerr          8: model_output and v in; the N x C sums are nothing beside it;
  loss           reads N x C float64 sums: launch-bound;
  terrain_u8     4 in for the reduction, 4 in again and 3 x 1 out for the bytes: 11.
The yardstick `torch_*` forms the same quantities with torch operations in the reference's own spelling (diffusion.py:116-143, 173-182).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBPS = 8000.0           # the MI355X's HBM3E rate, 8 TB/s
SHAPES = ((5, 2, 64, 64), (1, 0, 96, 96))       # (C, Cc, H, W)
K = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    from terrain_diffusion_amd import objective as ob
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "objective_bench measures on the GPU; there is no CPU fallback"
    row = ge.OBJECTIVE_LIBS[0]
    sha = ge._sha16(ge.side_deps(row[0], row[1], row[3]))
    eng = get_engine("cuda")
    dev = torch.device("cuda", eng.device_id)
    N, sd = args.items, 0.5

    with eng.on_stream(torch.cuda.Stream(), asynchronous=True):
        st = torch.cuda.current_stream()

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            rounds = []
            for _ in range(args.rounds):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                for _ in range(args.reps):
                    fn()
                b.record(st)
                b.synchronize()
                rounds.append(a.elapsed_time(b) / args.reps)
            rounds.sort()
            return rounds[len(rounds) // 2], rounds[0], rounds[-1]

        for Cn, Cc, H, W in SHAPES:
            elems = N * Cn * H * W

            def emit(what, t, bytes_per_element=None, **line):
                ms, lo, hi = t
                if bytes_per_element is not None:
                    gbps = bytes_per_element * elems / (ms * 1e-3) / 1e9
                    line.update(bytes_per_element=round(bytes_per_element, 2), GBps=round(gbps, 1), hbm_share=round(gbps / HBM_GBPS, 4))
                print(json.dumps({"tool": "objective_bench", "what": what, "source_sha16": sha, "items": N, "shape": [Cn, Cc, H, W], "reps": args.reps,
                                  "rounds": args.rounds, "device_ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), **line}), flush=True)

            g = torch.Generator(device=dev).manual_seed(1)
            rn = lambda *s: torch.randn(*s, generator=g, device=dev)
            images, noise, out, z = rn(N, Cn, H, W) * 0.5, rn(N, Cn, H, W), rn(N, Cn, H, W), rn(N)
            cond = rn(N, Cc, H, W) if Cc else None
            ch = list(range(min(4, Cn)))
            freqs, phases, wf = rn(K) * 6.2831853, torch.rand(K, generator=g, device=dev) * 6.2831853, rn(K) / K ** 0.5
            terrain = rn(N, 1, H, W) * 300.0
            table = ob.noise_levels(z, sigma_data=sd, P_mean=-0.4, P_std=1.0)
            _, v = ob.add_noise(images, noise, table, sigma_data=sd, cond_img=cond)
            lv = ob.logvar(table, freqs, phases, wf)
            S = ob.squared_error(out, v, sigma_data=sd)
            emit("levels", timed(lambda: ob.noise_levels(z, sigma_data=sd, P_mean=-0.4, P_std=1.0)))
            emit("levels_scale_sigma", timed(lambda: ob.noise_levels(z, sigma_data=sd, P_mean=-0.4, P_std=1.0, images=images, scale_channels=ch)), 8.0 * len(ch) / Cn)
            emit("noise", timed(lambda: ob.add_noise(images, noise, table, sigma_data=sd, cond_img=cond)), 20.0 + 8.0 * Cc / Cn)
            emit("logvar", timed(lambda: ob.logvar(table, freqs, phases, wf)))
            emit("sqerr", timed(lambda: ob.squared_error(out, v, sigma_data=sd)), 8.0)
            emit("loss", timed(lambda: ob.v_loss(S, H, W, sigma_data=sd, logvar=lv, enqueue_only=True)))
            emit("terrain_u8", timed(lambda: ob.terrain_uint8(terrain)), 11.0 / Cn)

            def objective():
                tb = ob.noise_levels(z, sigma_data=sd, P_mean=-0.4, P_std=1.0)
                _, vv = ob.add_noise(images, noise, tb, sigma_data=sd, cond_img=cond)
                ob.v_loss(ob.squared_error(out, vv, sigma_data=sd), H, W, sigma_data=sd, logvar=ob.logvar(tb, freqs, phases, wf), enqueue_only=True)
            emit("objective_device_half", timed(objective), 28.0 + 8.0 * Cc / Cn)

            # the yardstick: the same quantities from torch operations, spelled as the reference spells them
            def torch_objective():
                sigma = (z.reshape(-1, 1, 1, 1) * 1.0 + -0.4).exp()
                t = torch.atan(sigma / sd)
                nz = noise * sd
                x = (torch.cos(t) * images + torch.sin(t) * nz) / sd
                if cond is not None:
                    x = torch.cat([x, cond], dim=1)
                y = torch.log(torch.tan(t.flatten()) / 8).outer(freqs) + phases
                logvar = torch.nn.functional.linear(y.cos() * 2 ** 0.5, wf[None]).reshape(-1, 1, 1, 1)
                vt = torch.cos(t) * nz - torch.sin(t) * images
                return x, (1 / (logvar.exp() * sd ** 2) * ((-sd * out - vt) ** 2) + logvar).mean()
            emit("torch_objective", timed(torch_objective))

            def torch_terrain():
                lo, hi = torch.amin(terrain, dim=(1, 2, 3), keepdim=True), torch.amax(terrain, dim=(1, 2, 3), keepdim=True)
                rng = torch.maximum(hi - lo, torch.tensor(255.0, device=dev))
                return torch.clamp(((terrain - (lo + hi) / 2) / rng + 0.5) * 255, 0, 255).repeat(1, 3, 1, 1).to(torch.uint8)
            emit("torch_terrain_u8", timed(torch_terrain))


if __name__ == "__main__":
    main()
