"""Device time of the shaded-relief renderer (terrain_diffusion_amd.relief_map, libtd_relief.so) at 1024^2 and 4096^2 on seeded land-and-sea
canvases, with the bytes of its traffic model and the fraction of nominal HBM bandwidth that gives.  Prints one JSON line per size.

    python tools/relief_bench.py [--sizes 1024 4096] [--reps 100] [--warmup 10] [--reference PATH]

--reference PATH (a terrain-diffusion checkout with matplotlib and scipy importable) adds the reference's own get_relief_map on the host CPU,
labelled as host-measured.  Kernel split between the two passes: run this under `rocprofv3 --kernel-trace --stats -- python tools/relief_bench.py`
in a call of its own; the kernels are td::relief_blur_rows_kernel (pass 1) and td::relief_shade_kernel (pass 2).
"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NOMINAL_HBM_BPS = 8.0e12   # MI355X HBM3E, spec


def traffic_bytes(H, W, rl=24, rs=5):
    """Traffic model per render (not measured):
      pass 1 reads the elevation once (4 B/px) and writes the two axis-0-blurred planes (8 B/px);
      pass 2 reads those planes times its halo factor -- (16 + 2) rows by (128 + 2 + 2 R) columns staged per 128 x 16 tile, R = max(rl, rs) --
      plus the elevation again (4 B/px), and writes RGB (12 B/px).
    About 36 B/px at the default radii: 604 MB at 4096^2."""
    R = max(rl, rs)
    halo = (16 + 2) * (128 + 2 + 2 * R) / (16 * 128)
    per_px = 4 + 8 + 8 * halo + 4 + 12
    return int(per_px * H * W), per_px


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reference", default=None, help="terrain-diffusion checkout: also time its get_relief_map on the host CPU")
    args = ap.parse_args()
    import numpy as np
    import torch
    import _relief_twin as twin
    from terrain_diffusion_amd import relief_map
    from terrain_diffusion_amd.relief import _enqueue
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "relief_bench measures on the GPU; there is no CPU fallback"
    ref = None
    if args.reference and os.path.exists(args.reference):
        spec = importlib.util.spec_from_file_location("reference_relief_map", os.path.join(args.reference, "terrain_diffusion", "inference", "relief_map.py"))
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
    eng = get_engine("cuda")
    for n in args.sizes:
        host = twin.land_and_sea(n, n, 1000 + n)
        e = torch.from_numpy(host).cuda()
        with eng.on_stream(torch.cuda.Stream(), asynchronous=True):   # enqueue-only: the timed window holds GPU work, not host syncs
            s = torch.cuda.current_stream()
            out = relief_map(e, engine=eng)
            for _ in range(args.warmup):
                _enqueue(eng, e, out, None, 315.0, 6.0, 1.2, 90, 1.0, None, None)
            t0, t1, t2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            # the two kernels back to back (relief_map's NaN check, one host sync per call, left out) ...
            t0.record(s)
            for _ in range(args.reps):
                _enqueue(eng, e, out, None, 315.0, 6.0, 1.2, 90, 1.0, None, None)
            t1.record(s)
            t1.synchronize()
            # ... and the public call, NaN check included
            host_t = time.perf_counter()
            for _ in range(args.reps):
                relief_map(e, engine=eng)
            t2.record(s)
            t2.synchronize()
            call_ms = (time.perf_counter() - host_t) * 1e3 / args.reps
        ms = t0.elapsed_time(t1) / args.reps
        assert torch.equal(out, relief_map(e, engine=eng))
        nbytes, per_px = traffic_bytes(n, n)
        line = {"tool": "relief_bench", "H": n, "W": n, "reps": args.reps, "device_ms_per_render": round(ms, 4), "call_ms_host_clock": round(call_ms, 4),
                "model_bytes": nbytes, "model_bytes_per_px": round(per_px, 2), "achieved_TBps": round(nbytes / (ms * 1e-3) / 1e12, 3),
                "frac_nominal_hbm": round(nbytes / (ms * 1e-3) / NOMINAL_HBM_BPS, 3), "floor_us_at_nominal": round(nbytes / NOMINAL_HBM_BPS * 1e6, 1)}
        if ref is not None:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t = time.perf_counter()
                ref.get_relief_map(host, None, None, None)
                line["reference_host_cpu_s"] = round(time.perf_counter() - t, 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
