"""Device time of the river-map library (terrain_diffusion_amd.rivers, libtd_rivers.so) beside its yardstick, libtd_relief.so's render, at the
sizes a rendered region has.  Prints one JSON line per measurement.

    python tools/rivers_bench.py [--reps 10] [--warmup 2] [--rounds 3] [--sizes 1024 2048]

Method, the same for every figure: the mean of --reps back-to-back enqueue-only calls between two events on the engine's stream (inputs and
outputs are on the device before the timing starts; no host synchronisation inside the window).  Each measurement is taken --rounds times,
the variants of one size alternating, and reported as the median with the spread (min .. max) of the rounds: a difference inside the spread
is no difference.  At H = W = size:
  relief_map            libtd_relief.so's td_relief_map: the yardstick, the code path the parent of this library had;
  overlay_none          td_rivers_relief with rgb, biome and flow null (the same arithmetic, the overlay branches compiled in);
  overlay_biome_flow    td_rivers_relief with a biome image and a flow image (8 more bytes read per pixel);
  smooth_3              td_rivers_smooth, 3 iterations, with its achieved bytes/s against the 8 bytes per pixel and iteration it has to move
                        (one fp32 read, one fp32 write; the four neighbours come from cache).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    args = ap.parse_args()
    import numpy as np
    import torch
    import _relief_twin as twin
    from terrain_diffusion_amd import relief, rivers
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "rivers_bench measures on the GPU; there is no CPU fallback"
    eng = get_engine("cuda")
    dev = torch.device("cuda", eng.device_id)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    with eng.on_stream(torch.cuda.Stream(), asynchronous=True):
        st = torch.cuda.current_stream()

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(args.reps):
                fn()
            b.record(st)
            b.synchronize()
            return a.elapsed_time(b) / args.reps

        for n in args.sizes:
            rng = np.random.default_rng(n)
            e = up(twin.land_and_sea(n, n, 7))
            flow = up(np.floor(rng.random((n, n), dtype=np.float32) ** 4 * 40).astype(np.float32))
            biome = up(rng.integers(0, 31, size=(n, n)).astype(np.int32))
            out3 = torch.empty((n, n, 3), dtype=torch.float32, device=dev)
            common = (315.0, 6.0, 1.2, 90, 1.0, None, None)
            variants = {
                "relief_map": lambda: relief._enqueue(eng, e, out3, None, *common),
                "overlay_none": lambda: rivers._enqueue(eng, e, out3, None, None, None, None, 7, *common),
                "overlay_biome_flow": lambda: rivers._enqueue(eng, e, out3, None, None, biome, flow, 7, *common),
                "smooth_3": lambda: rivers.smooth_bumps(e, iterations=3, engine=eng),
            }
            ms = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    ms[k].append(timed(fn))
            for k, v in ms.items():
                med = statistics.median(v)
                line = dict(tool="rivers_bench", what=k, H=n, W=n, reps=args.reps, rounds=args.rounds, device_ms=round(med, 4),
                            device_ms_min=round(min(v), 4), device_ms_max=round(max(v), 4), device=torch.cuda.get_device_name(dev),
                            method="mean of back-to-back enqueue-only calls between two stream events; median of rounds")
                if k == "smooth_3":
                    line["achieved_TBps_of_8B_per_px_iter"] = round(8.0 * 3 * n * n / (med * 1e-3) / 1e12, 3)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
