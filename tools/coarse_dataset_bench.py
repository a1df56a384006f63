"""Device time of the coarse-dataset library (terrain_diffusion_amd.coarse_dataset, libtd_coarse.so) at the reference's sizes: one latitude band
of ETOPO at 30 arc-seconds, 1600 x 43200, shrunk to cos 30 degrees of its width and cut into 26-pixel tiles; fill_oceans on the resulting
61 x 1438 plane of tile means with about 70 % ocean, and on 1024 x 1024; the crop scores of 4096 crops of 16 x 16.  Prints one JSON line per
measurement.

    python tools/coarse_dataset_bench.py [--reps 5] [--warmup 1] [--rounds 3] [--rows 1600] [--width 43200]

The resize, the tile statistics and the crop scores are --reps back-to-back enqueue-only calls between two events on the engine's stream,
repeated --rounds times: the median per call with the least and the largest round.  Beside each time stand the bytes the kernels must move as
they are built and the GB/s that gives:
  area_resize   4 B per input pixel read, 4 B per output pixel written;
  tile_stats    4 B per pixel read (the outputs are one value per tile);
  crop_scores   4 c^2 B per crop.
fill_oceans is measured twice.  `fill_oceans` is the synchronous call as build_coarse_bands makes it (wall clock around the call, which completes on
return: the host reads the stop flag every 32 iterations), with the iteration counts it reports and the time per iteration that gives, setup and
read-backs included.  `fill_oceans_64` is an enqueue-only call with maxiter = 64, fewer than the fine level needs, between two events: 64 fine
iterations and up to 64 coarse ones, and the device time per fine iteration that gives (the coarse level's launches included).  The solver moves
90 B per pixel of the plane and iteration as it is built: pass 1 reads the code byte, z and p (neighbours through the caches) and writes p' and q
(33 B), pass 2 reads the code byte, p, q, x and r and writes x, r and z (57 B); land pixels cost their code byte only, so the figure is per
unknown.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOLVER_BYTES = 90.0


def terrain(shape, ocean_share, seed):
    """land values around 150 with a smooth coastline, NaN on the `ocean_share` lowest part of a smooth field"""
    import numpy as np
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    field = np.sin(ii / 5.3) * np.cos(jj / 7.1) + 0.6 * np.sin((ii + jj) / 11.0) + 0.5 * np.cos((ii - 2 * jj) / 17.0) + 0.15 * rng.standard_normal(shape)
    a = 150.0 + 40.0 * np.sin(ii / 9.0) * np.cos(jj / 6.0) + 5.0 * rng.standard_normal(shape)
    a[field < np.quantile(field, ocean_share)] = np.nan
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1600)
    ap.add_argument("--width", type=int, default=43200)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    from terrain_diffusion_amd import coarse_dataset as cd
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "coarse_dataset_bench measures on the GPU; there is no CPU fallback"
    eng = get_engine("cuda")
    dev = torch.device("cuda", eng.device_id)
    sha = ge._sha16(ge.side_deps("coarse", "coarse_csrc", "td_coarse.h"))
    H, W, t = args.rows, args.width, cd.TILE_PX
    w = cd.band_width(W, 30.0)

    def emit(what, ms, lo, hi, nbytes=None, **line):
        if nbytes is not None:
            line.update(MB=round(nbytes / 1e6, 2), GBps=round(nbytes / (ms * 1e-3) / 1e9, 1))
        print(json.dumps({"tool": "coarse_dataset_bench", "source_sha16": sha, "what": what, "device_ms": round(ms, 4), "min_ms": round(lo, 4),
                          "max_ms": round(hi, 4), **line}), flush=True)

    with eng.on_stream(torch.cuda.Stream(), asynchronous=True):
        st = torch.cuda.current_stream()

        def timed(fn, reps=args.reps):
            for _ in range(args.warmup):
                fn()
            rounds = []
            for _ in range(args.rounds):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                for _ in range(reps):
                    fn()
                b.record(st)
                b.synchronize()
                rounds.append(a.elapsed_time(b) / reps)
            rounds.sort()
            return rounds[len(rounds) // 2], rounds[0], rounds[-1]

        g = torch.Generator(device=dev).manual_seed(1)
        band = torch.randn((H, W), generator=g, device=dev) * 900.0 + 200.0
        emit("area_resize", *timed(lambda: cd.area_resize_width(band, w, "signed_sqrt", engine=eng)), nbytes=4.0 * H * (W + w), H=H, W_in=W, W_out=w,
             load_rule="signed_sqrt")
        scaled = cd.area_resize_width(band, w, "signed_sqrt", engine=eng)
        emit("tile_stats_mean_quantile", *timed(lambda: cd.tile_stats(scaled, t, stats=("mean", "quantile"), engine=eng)), nbytes=4.0 * (H // t * t) * (w // t * t),
             Hs=H, Ws=w, t=t, tiles=[H // t, w // t])
        emit("tile_stats_nanmean", *timed(lambda: cd.tile_stats(scaled, t, stats=("nanmean",), engine=eng)), nbytes=4.0 * (H // t * t) * (w // t * t),
             Hs=H, Ws=w, t=t)
        plane = torch.randn((H // t, w // t), generator=g, device=dev)
        c, n_crops = 16, 4096
        off = torch.stack([torch.randint(0, H // t - c + 1, (n_crops,), generator=g, device=dev),
                           torch.randint(0, w // t - c + 1, (n_crops,), generator=g, device=dev)], 1).to(torch.int32)
        emit("crop_scores", *timed(lambda: cd.crop_scores(plane, 3.7, 21.5, off, c, engine=eng)), nbytes=4.0 * c * c * n_crops, N=n_crops, c=c)

    for name, shape in (("band", (H // t, w // t)), ("square", (1024, 1024))):
        a = torch.from_numpy(terrain(shape, 0.7, 7)).to(dev)
        unknowns = int(torch.isnan(a).sum())
        cd.fill_oceans_device(a, tol=cd.FILL_TOL, engine=eng)
        walls = []
        for _ in range(args.rounds):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out, info = cd.fill_oceans_device(a, tol=cd.FILL_TOL, return_info=True, engine=eng)
            torch.cuda.synchronize(dev)
            walls.append((time.perf_counter() - t0) * 1e3)
        walls.sort()
        info = info.cpu().tolist()
        iters = info[0] + info[2]
        emit("fill_oceans", walls[len(walls) // 2], walls[0], walls[-1], plane=name, H=shape[0], W=shape[1], unknowns=unknowns, info=info,
             ms_per_iteration=round(walls[len(walls) // 2] / max(iters, 1), 5), clock="wall")
        with eng.on_stream(torch.cuda.Stream(), asynchronous=True):
            st = torch.cuda.current_stream()
            rounds = []
            for _ in range(args.rounds + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                cd.fill_oceans_device(a, tol=cd.FILL_TOL, maxiter=64, enqueue_only=True, engine=eng)
                e1.record(st)
                e1.synchronize()
                rounds.append(e0.elapsed_time(e1))
            rounds = sorted(rounds[1:])
        ms = rounds[len(rounds) // 2]
        emit("fill_oceans_64", ms, rounds[0], rounds[-1], plane=name, H=shape[0], W=shape[1], unknowns=unknowns, ms_per_iteration=round(ms / 64, 5),
             bytes_per_unknown_iteration=SOLVER_BYTES, GBps_fine=round(SOLVER_BYTES * unknowns * 64 / (ms * 1e-3) / 1e9, 1))


if __name__ == "__main__":
    main()
