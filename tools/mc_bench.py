"""Device time of the Minecraft terrain library (terrain_diffusion_amd.minecraft, libtd_mc.so) per stage, for scale in {1, 2, 4, 8} and output
side in {256, 1024, 4096}, on a crop-consistent synthetic world (smooth fields of the absolute pixel: sea and land, steep ridges, every
climate band).  Prints one JSON line per (scale, side).

    python tools/mc_bench.py [--scales 1 2 4 8] [--sides 256 1024 4096] [--reps 20] [--warmup 3] [--twin-max-side 1024]

Stages, CUDA-event times on the engine's stream averaged over --reps calls (the world.get windows are fetched once, outside the timing):
  upsample  the padded elevation and the 5 climate channels of the requested box (scale > 1; none at scale 1);
  finish    the fused Sobel + detail noise (noise_scale 1) + biome classifier, built-in noise;
  payload   the int16 elevation + biome buffer on the device (the one device-to-host copy is not included).
cpu_standin_s is the NumPy twin's host time for the same request (tests/_mc_twin.py, one thread): a CPU stand-in for the reference's host tail,
whose own path needs pyfastnoiselite and cannot be timed here.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NOMINAL_HBM_BPS = 8.0e12     # MI355X HBM3E, spec
NOMINAL_FP32_FLOPS = 157e12  # MI355X vector fp32, spec


def model(scale):
    """Bytes and ALU model per output pixel (not measured):
      upsample  writes the padded elevation (~4 B) and 5 climate channels (20 B); the native window is tiny and cached        = 24 B
      finish    reads elev_padded (4 B + halo), 4 climate channels (16 B), writes elev (4 B, when noise > 0) and the biome (2 B) = 26 B
      payload   reads elev and biome (6 B), writes 2 x int16 (4 B)                                                             = 10 B
    ALU: about 12 single-octave Perlin evaluations (7 classifier, 5 detail; at scale 1 only the 7) of ~45 flop each, the Sobel, the
    climate variables and the decision tree (~150 flop), and a float64 asin."""
    perlin = 12 if scale > 1 else 7
    return ({"upsample": 24.0 if scale > 1 else 0.0, "finish": 26.0 if scale > 1 else 22.0, "payload": 10.0},
            {"perlin_evals": perlin, "flop": perlin * 45 + 150})


class FieldWorld:
    native_resolution = 90.0

    def get(self, i1, j1, i2, j2, with_climate=True):
        import numpy as np
        import torch
        ii, jj = np.meshgrid(np.arange(i1, i2, dtype=np.float64), np.arange(j1, j2, dtype=np.float64), indexing="ij")
        elev = 1400 * np.sin(ii / 53.0) * np.cos(jj / 71.0) + 900 * np.sin((ii + 2 * jj) / 23.0) + 600 * np.cos(jj / 9.0 - ii / 13.0) + 300
        clim = np.stack([12 + 18 * np.sin(ii / 97.0) + 6 * np.cos(jj / 41.0), 700 + 600 * np.sin(jj / 61.0),
                         900 + 850 * np.cos(ii / 37.0 + jj / 89.0), 60 + 50 * np.sin(ii / 29.0 + jj / 17.0), 0.0065 + 0 * ii])
        return {"elev": torch.from_numpy(elev.astype(np.float32)).cuda(),
                "climate": torch.from_numpy(clim.astype(np.float32)).cuda() if with_climate else None}


class Cached:
    """world.get answered from the first call's tensors: the benchmark times the library, not the world."""

    def __init__(self, world):
        self.world, self.native_resolution, self.memo = world, world.native_resolution, {}

    def get(self, *box, with_climate=True):
        key = (*box, with_climate)
        if key not in self.memo:
            self.memo[key] = self.world.get(*box, with_climate=with_climate)
        return self.memo[key]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--twin-max-side", type=int, default=1024, help="time the NumPy twin up to this side (it is slow)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import _mc_twin as twin
    from terrain_diffusion_amd import minecraft as mc
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "mc_bench measures on the GPU; there is no CPU fallback"
    eng = get_engine("cuda")
    for s in args.scales:
        for n in args.sides:
            world = Cached(FieldWorld())
            i1, j1 = -n // 2 + 7, 3 - n // 3
            i2, j2 = i1 + n, j1 + n
            H = W = n
            nr = world.native_resolution
            with eng.on_stream(torch.cuda.Stream(), asynchronous=True):
                st = torch.cuda.current_stream()
                dev = torch.device("cuda", eng.device_id)

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

                elev_b = torch.empty((H, W), dtype=torch.float32, device=dev)
                biome = torch.empty((H, W), dtype=torch.int16, device=dev)
                payload = torch.empty(2 * H * W, dtype=torch.int16, device=dev)
                stream = eng.stream
                if s > 1:
                    _, _, padded, climate = mc._upsampled(world, i1, j1, i2, j2, s, H, W, eng)
                    en, cn = mc._fetch(world, mc._native_box(i1, j1, i2, j2, s, 2), True, dev)
                    r0 = 2 * s + (i1 - (i1 // s) * s)
                    c0 = 2 * s + (j1 - (j1 // s) * s)
                    up_ms = timed(lambda: (mc._upsample(en[None], s, r0 - 1, c0 - 1, H + 2, W + 2, eng, dev),
                                           mc._upsample(cn, s, r0, c0, H, W, eng, dev)))
                    elev_in = padded[1:-1, 1:-1]
                    fin = lambda: mc._finish(eng, dev, elev_in, padded, climate, H, W, i1, j1, None, 1.0, nr / s, nr, nr / s, elev_b, biome)
                else:
                    up_ms = 0.0
                    padded, _ = mc._fetch(world, (i1 - 1, j1 - 1, i2 + 1, j2 + 1), False, dev)
                    elev_b, climate = mc._fetch(world, (i1, j1, i2, j2), True, dev)
                    fin = lambda: mc._finish(eng, dev, elev_b, padded, climate, H, W, i1, j1, None, 0.0, nr, nr, nr, None, biome)
                fin_ms = timed(fin)
                import ctypes as C
                pay_ms = timed(lambda: mc.check(mc.lib().td_mc_payload(C.c_void_p(stream), C.c_void_p(elev_b.data_ptr()),
                                                                        C.c_void_p(biome.data_ptr()), H, W, C.c_void_p(payload.data_ptr()), 0)))
            ms = {"upsample": up_ms, "finish": fin_ms, "payload": pay_ms}
            bpp, alu = model(s)
            px = H * W
            line = {"tool": "mc_bench", "scale": s, "H": H, "W": W, "reps": args.reps, "device_ms": {k: round(v, 4) for k, v in ms.items()},
                    "device_ms_total": round(sum(ms.values()), 4), "model_bytes_per_px": bpp, "model_alu_per_px": alu,
                    "achieved_TBps": {k: round(bpp[k] * px / (ms[k] * 1e-3) / 1e12, 3) for k in ms if ms[k] > 0},
                    "finish_frac_nominal_fp32": round(alu["flop"] * px / (fin_ms * 1e-3) / NOMINAL_FP32_FLOPS, 3)}
            if n <= args.twin_max_side:
                t0 = time.perf_counter()
                planes = twin.noise_planes(i1, j1, H, W)
                if s == 1:
                    wins = [tuple(None if v is None else v.cpu().numpy() for v in (world.get(i1 - 1, j1 - 1, i2 + 1, j2 + 1, with_climate=False)["elev"], None)),
                            tuple(None if v is None else v.cpu().numpy() for v in (world.get(i1, j1, i2, j2)["elev"], world.get(i1, j1, i2, j2)["climate"]))]
                else:
                    b = mc._native_box(i1, j1, i2, j2, s, 2)
                    g = world.get(*b)
                    wins = [(g["elev"].cpu().numpy(), g["climate"].cpu().numpy())]
                t1 = time.perf_counter()
                twin.minecraft_terrain(wins, i1, j1, i2, j2, s, 1.0, nr, planes)
                line["cpu_standin_s"] = round(time.perf_counter() - t1 + (t1 - t0), 3)
                line["cpu_standin"] = "NumPy twin on the host (one thread), not the reference"
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
