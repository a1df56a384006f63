"""Device time of the custom-map import library (terrain_diffusion_amd.custom_world, libtd_custom.so) at the sizes a user's map has.  Prints
one JSON line per measurement.

    python tools/custom_world_bench.py [--reps 10] [--warmup 2] [--cells 50000] [--skip-large]

Measurements, CUDA-event times on the engine's stream averaged over --reps calls (inputs are on the device before the timing starts):
  rasterize     a 2048 x 1024 raster of --cells Voronoi cells (tests/_custom_twin.voronoi_cells: every pixel is covered once);
  fill_nearest  the nearest-valid fill at 2048 x 1024 and at 4096 x 4096 with 30 % holes, once scattered pixel by pixel (the search radius of
                a hole is a few pixels) and once as 64 x 64 blocks (the radius reaches 64 and more): the work per hole grows with the
                distance to its nearest valid pixel;
  elev_int16    the export's conversion of a 2048 x 2048 chunk.
The fill's model is the integer work it does, not bytes: per hole one scan of the columns within its search radius, about 6 integer
operations per column visited.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def holes(shape, kind, seed):
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
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--skip-large", action="store_true", help="leave the 4096 x 4096 fills out")
    args = ap.parse_args()
    import numpy as np
    import torch
    import _custom_twin as twin
    from terrain_diffusion_amd import custom_world as cw
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "custom_world_bench measures on the GPU; there is no CPU fallback"
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

        def emit(**line):
            print(json.dumps({"tool": "custom_world_bench", "reps": args.reps, **line}), flush=True)

        H, W = 1024, 2048
        sites, vertices, rings = twin.voronoi_cells(args.cells, W, H, seed=1)
        xy, offsets = twin.csr_of(vertices, rings)
        dxy, doff, dval = up(xy), up(offsets), up(np.arange(args.cells, dtype=np.float32))
        ms = timed(lambda: cw.rasterize_cells(dxy, doff, dval, (H, W), float("nan"), engine=eng))
        out = cw.rasterize_cells(dxy, doff, dval, (H, W), float("nan"), engine=eng)
        emit(what="rasterize", H=H, W=W, cells=args.cells, vertices=int(len(xy)), device_ms=round(ms, 4), uncovered_pixels=int(torch.isnan(out).sum()))

        for shape in ((1024, 2048),) + (() if args.skip_large else ((4096, 4096),)):
            for kind in ("scattered", "blocks"):
                mask = holes(shape, kind, 2)
                a = np.random.default_rng(3).standard_normal(shape).astype(np.float32)
                a[mask] = np.nan
                da = up(a)
                ms = timed(lambda: cw._fill(eng, dev, da, float("nan"), False))
                _, _, valid = cw._fill(eng, dev, da, float("nan"), False)
                emit(what="fill_nearest", H=shape[0], W=shape[1], holes=kind, hole_share=round(float(mask.mean()), 4), device_ms=round(ms, 4),
                     valid_pixels=int(valid))

        e = up((np.random.default_rng(4).standard_normal((2048, 2048)) * 20000).astype(np.float32))
        ms = timed(lambda: cw.elevation_int16(e, engine=eng))
        emit(what="elev_int16", H=2048, W=2048, device_ms=round(ms, 4), achieved_TBps=round(6.0 * e.numel() / (ms * 1e-3) / 1e12, 3))


if __name__ == "__main__":
    main()
