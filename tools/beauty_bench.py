"""Device time of the spectrum library (terrain_diffusion_amd.beauty, libtd_spectrum.so): the transform with its ring means at 512 x 512,
2048 x 2048 and 4096 x 4096 for B = 1 and B = 8, the decode, and the whole calculate_beauty_score at the reference's chunk size.  Prints one
JSON line per measurement; every line carries the hash of the library's sources.

    python tools/beauty_bench.py [--reps 10] [--warmup 2] [--rounds 3] [--sizes 512 2048 4096] [--batches 1 8]

Each measurement is --reps back-to-back enqueue-only calls between two events on the engine's stream (inputs are on the device before the timing
starts, so a host enqueue gap would be included), repeated --rounds times: the median per call with the least and the largest round.  Beside
each time stand the bytes per pixel the kernels must move as they are built, the GB/s that gives and its share of the HBM rate:
  fft2 + bins    20 B / pixel: the row pass reads the plane (4) and writes the half spectrum (4: 8 bytes per coefficient, half as many
                 coefficients as pixels), the column pass reads it (4) and writes log|F| (4), the bins read log|F| (4) and the byte map (1, shared
                 by the planes of a batch and left to the caches); the twiddles stay in the caches;
  decode         12 B / pixel: the residual in, the plane out, the plane in again for the centred squares; the low band stays in the caches;
  score          the whole calculate_beauty_score, its one read-back included (one host synchronisation per call).
The yardstick is torch.fft.rfft2 on the device for the same planes in the same process (rocFFT behind it), which produces the half spectrum
only: 8 B / pixel.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBPS = 8000.0           # the MI355X's HBM3E rate, 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048, 4096])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    from terrain_diffusion_amd import beauty as bt
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "beauty_bench measures on the GPU; there is no CPU fallback"
    row = ge.SPECTRUM_LIBS[0]
    sha = ge._sha16(ge.side_deps(row[0], row[1], row[3]))
    eng = get_engine("cuda")
    dev = torch.device("cuda", eng.device_id)

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

        def emit(what, t, bytes_per_pixel=None, pixels=None, **line):
            ms, lo, hi = t
            if bytes_per_pixel is not None:
                gbps = bytes_per_pixel * pixels / (ms * 1e-3) / 1e9
                line.update(bytes_per_pixel=bytes_per_pixel, GBps=round(gbps, 1), hbm_share=round(gbps / HBM_GBPS, 4))
            print(json.dumps({"tool": "beauty_bench", "what": what, "source_sha16": sha, "reps": args.reps, "rounds": args.rounds,
                              "device_ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), **line}), flush=True)

        gen = torch.Generator(device=dev).manual_seed(5)
        for S in args.sizes:
            for B in args.batches:
                x = torch.rand((B, S, S), generator=gen, device=dev) * 900.0
                bt.bin_map(S, S, bt.SCORE_BINS, dev)           # built and uploaded before the timing starts
                t = timed(lambda: bt.radial_spectrum(x, bt.SCORE_BINS, engine=eng))
                emit("fft2_bins", t, 20.0, B * S * S, B=B, H=S, W=S, bins=bt.SCORE_BINS)
                t = timed(lambda: bt.fft2(x, spectrum=True, logabs=False, engine=eng))
                emit("fft2_half_spectrum", t, 12.0, B * S * S, B=B, H=S, W=S)
                t = timed(lambda: torch.fft.rfft2(x))
                emit("torch_rfft2", t, 8.0, B * S * S, B=B, H=S, W=S)
                del x
        S = max(args.sizes)
        low = torch.rand((1, S // 8, S // 8), generator=gen, device=dev) * 30.0 - 8.0
        res = torch.rand((1, S, S), generator=gen, device=dev) - 0.5
        t = timed(lambda: bt.decode_terrain(low, res, return_stats=True, engine=eng))
        emit("decode", t, 12.0, S * S, B=1, H=S, W=S, h=S // 8, w=S // 8)
        t = timed(lambda: bt.calculate_beauty_score(low[0], res[0], engine=eng))
        emit("calculate_beauty_score", t, H=S, W=S, h=S // 8, w=S // 8, score=bt.calculate_beauty_score(low[0], res[0], engine=eng))


if __name__ == "__main__":
    main()
