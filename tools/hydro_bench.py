"""Device time of the hydrology library (terrain_diffusion_amd.hydrology, libtd_hydro.so) per stage at 1024^2 and 4096^2 on seeded rugged
land-and-sea canvases (pits, a plateau, NaN holes), with the fill's pass count, the accumulation's longest flow path, and the bytes of a traffic
model per stage over the time.  Prints one JSON line per size.

    python tools/hydro_bench.py [--sizes 1024 4096] [--reps 20] [--warmup 3]

Stages: d8 (flow_directions), accumulation (flow_accumulation_map over the d8 of the filled canvas, its 4-byte uphill-edge read included),
indicator (max-pool 1 and log1p of that accumulation), fill (fill_depressions of the raw canvas: relaxation passes, each batch of 8 ending in a
host read of the convergence flags).  Times are CUDA-event times on the engine's stream, averaged over --reps calls.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NOMINAL_HBM_BPS = 8.0e12   # MI355X HBM3E, spec


def model_bytes_per_cell(passes):
    """Traffic model per cell (not measured):
      d8           reads z (4 B; the 8 neighbours hit in cache), writes receiver, kmax, is_sink (6 B)                       = 10 B
      accumulation init reads z, writes the 8-B word; edges read z, receiver, is_sink, z[receiver], write next, one 8-B
                   atomic; walk reads the word and next, one 8-B atomic per edge; out reads the word, writes fp32         = 69 B
      indicator    reads acc, writes fp32 (k = 1)                                                                            = 8 B
      fill         init reads h (+ neighbours in cache), writes d and hw (12 B); per pass, every tile active (an upper
                   bound: tiles whose neighbourhood did not change are skipped), reads d and hw over 66^2 / 64^2 cells and
                   writes d (4 B) = 12.5 B; out reads h and d, writes d (12 B)                                                = 24 + 12.5 passes B"""
    return {"d8": 10.0, "accumulation": 69.0, "indicator": 8.0, "fill": 24.0 + (8.0 * 66.0 * 66.0 / (64.0 * 64.0) + 4.0) * passes}


def longest_path(receiver, sink, z):
    """Longest chain of counted edges (cells), by pointer doubling on the device."""
    import torch
    N = receiver.numel()
    idx = torch.arange(N, device=receiver.device)
    zf = z.reshape(-1)
    r = receiver.reshape(-1).long()
    counted = (zf > 0) & ~sink.reshape(-1) & (zf[r] > 0)
    nxt = torch.where(counted, r, idx)
    dist = counted.long()
    while True:
        nn = nxt[nxt]
        dist = dist + dist[nxt]          # a terminal cell points at itself with distance 0
        if torch.equal(nn, nxt):
            break
        nxt = nn
    return int(dist.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import _hydro_twin as twin
    from terrain_diffusion_amd import fill_depressions, flow_accumulation_map, flow_directions, flow_indicator
    from terrain_diffusion_amd.hydrology import _indicator_of
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "hydro_bench measures on the GPU; there is no CPU fallback"
    eng = get_engine("cuda")
    dev = torch.device("cuda", eng.device_id)
    for n in args.sizes:
        z = torch.from_numpy(twin.rugged(n, n, 2000 + n)).cuda()
        filled, passes = fill_depressions(z, return_passes=True)
        with eng.on_stream(torch.cuda.Stream(), asynchronous=True):
            s = torch.cuda.current_stream()

            def timed(fn):
                for _ in range(args.warmup):
                    fn()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for _ in range(args.reps):
                    fn()
                b.record(s)
                b.synchronize()
                return a.elapsed_time(b) / args.reps

            rec, _, sink = flow_directions(filled, engine=eng)
            acc = flow_accumulation_map(filled, rec, sink, engine=eng)
            ms = {"d8": timed(lambda: flow_directions(filled, engine=eng)),
                  "accumulation": timed(lambda: flow_accumulation_map(filled, rec, sink, engine=eng)),
                  "indicator": timed(lambda: _indicator_of(acc, 1, eng, dev)),
                  "fill": timed(lambda: fill_depressions(z, engine=eng))}
            ind_ms = timed(lambda: flow_indicator(filled, engine=eng))
        per_cell = model_bytes_per_cell(passes)
        cells = n * n
        line = {"tool": "hydro_bench", "H": n, "W": n, "reps": args.reps, "fill_passes": passes,
                "longest_flow_path_cells": longest_path(rec, sink, filled), "max_upstream_cells": int(acc.max()),
                "device_ms": {k: round(v, 4) for k, v in ms.items()}, "plot_flow_indicator_device_ms": round(ind_ms, 4),
                "model_bytes_per_cell": {k: round(v, 1) for k, v in per_cell.items()},
                "achieved_TBps": {k: round(per_cell[k] * cells / (ms[k] * 1e-3) / 1e12, 3) for k in ms},
                "frac_nominal_hbm": {k: round(per_cell[k] * cells / (ms[k] * 1e-3) / NOMINAL_HBM_BPS, 3) for k in ms}}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
