"""Device time of the dataset-preparation library (terrain_diffusion_amd.dataset, libtd_dataset.so) at the reference's chunk size: a 4096 x 4096
DEM with 30 % voids, a 512 x 512 low band (r = 8), sigma 5.  Prints one JSON line per measurement.

    python tools/dataset_bench.py [--reps 10] [--warmup 2] [--rounds 3] [--size 4096] [--lowres 512]

Each measurement is --reps back-to-back enqueue-only calls between two events on the engine's stream (inputs are on the device before the timing
starts, so a host enqueue gap would be included), repeated --rounds times: the median per call with the least and the largest round.  Beside
each time stand the bytes per pixel the kernels must move as they are built and the GB/s that gives:
  fill_voids     16.2 B / pixel at 30 % voids: the column pass reads the DEM (4) and writes and re-reads the byte plane of column distances (2),
                 the row pass reads the DEM (4), the byte plane (1) and the base at the voids (1.2) and writes the result (4); halo reads are
                 left to the caches.  Voids come scattered (short searches) and as 64 x 64 blocks (searches up to the radius);
  block_median   4 + 4 / r^2 B / pixel: every value once, one median per block;
  residual       8 B / pixel: x in, the residual out; the low band stays in the caches;
  land_counts    4 B / pixel of the low band;
  moments        8 B / value: two passes over one plane;
  prepare_chunks the whole routine, its read-back of the land counts included (one host synchronisation per call).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def void_mask(shape, kind, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    if kind == "scattered":
        return rng.random(shape) < 0.3
    blocks = rng.random((shape[0] // 64, shape[1] // 64)) < 0.3
    return np.kron(blocks, np.ones((64, 64), bool)).astype(bool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--lowres", type=int, default=512)
    args = ap.parse_args()
    import numpy as np
    import torch
    from terrain_diffusion_amd import dataset as ds
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "dataset_bench measures on the GPU; there is no CPU fallback"
    eng = get_engine("cuda")
    dev = torch.device("cuda", eng.device_id)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    S, L = args.size, args.lowres
    r = S // L
    sigma = 5.0

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
                line.update(bytes_per_pixel=round(bytes_per_pixel, 3), GBps=round(bytes_per_pixel * pixels / (ms * 1e-3) / 1e9, 1))
            print(json.dumps({"tool": "dataset_bench", "what": what, "reps": args.reps, "rounds": args.rounds, "device_ms": round(ms, 4),
                              "min_ms": round(lo, 4), "max_ms": round(hi, 4), **line}), flush=True)

        rng = np.random.default_rng(3)
        ii = np.arange(S, dtype=np.float32)
        dem = (800.0 * np.sin(ii[:, None] / 301.0) * np.cos(ii[None, :] / 211.0) + rng.standard_normal((S, S)) * 20.0).astype(np.float32)
        base = up(np.full((S, S), -40.0, np.float32) - np.abs(dem) * 0.1)
        filled = None
        for kind in ("scattered", "blocks"):
            a = dem.copy()
            mask = void_mask((S, S), kind, 2)
            a[mask] = np.nan
            da = up(a)
            t = timed(lambda: ds.fill_voids(da, base, 32, True, engine=eng))
            filled, count = ds.fill_voids(da, base, 32, True, return_count=True, engine=eng)
            share = float(mask.mean())
            emit("fill_voids", t, 15.0 + 4.0 * share, S * S, H=S, W=S, radius=32, voids=kind, void_share=round(share, 4), void_count=int(count))
        t = timed(lambda: ds.block_median(filled, r, engine=eng))
        emit("block_median", t, 4.0 + 4.0 / (r * r), S * S, H=S, W=S, r=r)
        low = ds.laplacian_encode(filled, L, sigma, engine=eng)[1]
        out = torch.empty_like(filled)
        t = timed(lambda: ds.residual(filled, low, out=out, engine=eng))
        emit("residual", t, 8.0, S * S, H=S, W=S, h=L, w=L)
        t = timed(lambda: ds.laplacian_encode(filled, L, sigma, engine=eng))
        emit("laplacian_encode", t, H=S, W=S, h=L, w=L, sigma=sigma)
        t = timed(lambda: ds.land_counts(low, 1, engine=eng))
        emit("land_counts", t, 4.0, L * L, h=L, w=L, num_chunks=1)
        t = timed(lambda: ds.moments(filled, engine=eng))
        emit("moments", t, 8.0, S * S, C=1, n=S * S)
        t = timed(lambda: ds.prepare_chunks(da, base, L, sigma, engine=eng))
        emit("prepare_chunks", t, H=S, W=S, lowres_size=L, lowres_sigma=sigma, voids="blocks")


if __name__ == "__main__":
    main()
