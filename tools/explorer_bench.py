"""Device time of the explorer views (terrain_diffusion_amd.explorer, libtd_explorer.so) on a synthetic world: a 100 x 100 coarse view with
two filters, a 1024^2 detail image in each mode, a 1024^2 raw tile and the land-tile search on a 600 x 600 window (the sampler's default).
Prints one JSON line per workload.

    python tools/explorer_bench.py [--reps 30] [--warmup 5] [--detail 1024] [--window 300]

device_ms is the median over --reps calls of the HIP-event time of the kernels one call enqueues on the engine's stream (the world.coarse /
world.get reads are made once, outside the timing; the device-to-host copy of the result is not included).  call_ms is the median wall time
of the whole drop-in, result on the host, and host_copies the device-to-host copies it makes per call (each is one host synchronisation;
relief mode adds relief_map's NaN check).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class FieldWorld:
    """Smooth fields of the absolute index, built on the device; every read is answered from the first one's tensors."""
    native_resolution, seed = 90.0, 1

    def __init__(self):
        self.memo, self.coarse = {}, self

    def __getitem__(self, idx):
        import torch
        _, si, sj = idx
        key = ("c", si.start, si.stop, sj.start, sj.stop)
        if key not in self.memo:
            ii, jj = torch.meshgrid(torch.arange(si.start, si.stop, device="cuda", dtype=torch.float64),
                                    torch.arange(sj.start, sj.stop, device="cuda", dtype=torch.float64), indexing="ij")
            a = torch.sin(0.131 * ii + 0.217 * jj) + 0.6 * torch.cos(0.093 * ii - 0.171 * jj)
            b = torch.sin(0.071 * ii - 0.113 * jj + 1.0)
            w = 1.0 + 0.45 * torch.sin(0.31 * ii + 0.23 * jj)
            vals = torch.stack([38 * a, 30 * a - 6, 11 + 17 * b, 600 + 450 * a * b, 900 * (a + 0.4), 55 + 40 * b])
            self.memo[key] = torch.cat([vals * w, w[None]]).float()
        return self.memo[key]

    def get(self, i1, j1, i2, j2, with_climate=True):
        import torch
        key = ("g", i1, j1, i2, j2)
        if key not in self.memo:
            ii, jj = torch.meshgrid(torch.arange(i1, i2, device="cuda", dtype=torch.float64), torch.arange(j1, j2, device="cuda", dtype=torch.float64),
                                    indexing="ij")
            elev = 1400 * torch.sin(ii / 53.0) * torch.cos(jj / 71.0) + 900 * torch.sin((ii + 2 * jj) / 23.0) + 600 * torch.cos(jj / 9.0 - ii / 13.0) + 300
            clim = torch.stack([12 + 18 * torch.sin(ii / 97.0) + 6 * torch.cos(jj / 41.0), 700 + 600 * torch.sin(jj / 61.0),
                                900 + 850 * torch.cos(ii / 37.0 + jj / 89.0), 60 + 50 * torch.sin(ii / 29.0 + jj / 17.0), 0.0065 + 0 * ii])
            self.memo[key] = {"elev": elev.float(), "climate": clim.float()}
        return self.memo[key]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--detail", type=int, default=1024)
    ap.add_argument("--window", type=int, default=300)
    args = ap.parse_args()
    import torch
    from terrain_diffusion_amd import explorer as ex
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "explorer_bench measures on the GPU; there is no CPU fallback"
    eng = get_engine("cuda")
    dev = torch.device("cuda", eng.device_id)
    world = FieldWorld()
    n, win = args.detail, args.window
    region = world.get(-n // 2, -n // 2, n // 2, n // 2)
    elev, temp = region["elev"], region["climate"][0].contiguous()
    filters = {0: (0.0, None), 2: (None, 20.0)}

    def coarse_view():
        planes, _ = ex._channels(eng, dev, world.coarse[:, -50:50, -50:50], 2, 1e-8, True)
        ex._colorize(eng, dev, planes[4], "viridis", True, None, None, [(planes[0], 0.0, None), (planes[2], None, 20.0)], True)

    def land():
        planes, _ = ex._channels(eng, dev, world.coarse[:, -win:win, -win:win], 2, 0.0, True)
        ex._land(eng, dev, planes[0], 2, 0.5, True)

    work = [
        ("coarse_image_100x100_2_filters", coarse_view, lambda: ex.coarse_image(world, 4, filters=filters)),
        (f"detail_image_elevation_{n}", lambda: ex._colorize(eng, dev, elev, "terrain", False, None, None, (), True),
         lambda: ex.detail_image(world, detail_size=n, mode="elevation")),
        (f"detail_image_temperature_{n}", lambda: ex._colorize(eng, dev, temp, "RdBu_r", False, None, None, (), True),
         lambda: ex.detail_image(world, detail_size=n, mode="temperature")),
        (f"detail_image_relief_{n}", lambda: ex._quantize(eng, dev, ex._relief_enqueue(eng, dev, elev, 90.0), True),
         lambda: ex.detail_image(world, detail_size=n, mode="relief")),
        (f"detail_raw_{n}", lambda: ex._raw(eng, dev, elev, temp, True), lambda: ex.detail_raw(world, detail_size=n)),
        (f"land_tiles_{2 * win}x{2 * win}", land, lambda: ex.sample_land_tiles(world, win, 1024, 0.5, 10)),
    ]
    for name, enqueue, call in work:
        with eng.on_stream(torch.cuda.Stream(), asynchronous=True):
            st = torch.cuda.current_stream()
            for _ in range(args.warmup):
                enqueue()
            times = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                enqueue()
                b.record(st)
                b.synchronize()
                times.append(a.elapsed_time(b))
        for _ in range(args.warmup):
            call()
        copies0, wall = ex.HOST_COPIES, []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"tool": "explorer_bench", "workload": name, "reps": args.reps, "device_ms": round(statistics.median(times), 4),
                          "device_ms_min": round(min(times), 4), "call_ms": round(statistics.median(wall), 3),
                          "host_copies": (ex.HOST_COPIES - copies0) / args.reps}), flush=True)


if __name__ == "__main__":
    main()
