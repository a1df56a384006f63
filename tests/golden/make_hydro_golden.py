"""Generates tests/golden/hydro.npz by RUNNING THE REFERENCE'S OWN postprocessing.py (terrain_diffusion/inference/postprocessing.py: d8_flow,
flow_accumulation, plot_flow_indicator, fill_depressions_priority_flood).

Needs a checkout of the reference (and the matplotlib / torch it imports); the fixture does not.  The module is loaded by path, so nothing else
of the reference is imported.  Only inputs, keywords, outputs and the numpy version are stored, never source text:

    python tests/golden/make_hydro_golden.py --reference PATH_TO_REFERENCE_CHECKOUT      (or TD_REFERENCE=PATH)

Each case is {"name", "fn" (fill | d8 | acc | indicator), "input", "kwargs"}.  Outputs: fill -> out_<name> fp32; d8 -> receiver_<name>
(rr * W + cc, int32), kmax_<name> (uint8), sink_<name> (bool); acc -> out_<name> fp32 (over the reference's d8_flow of the same input with
its default tol); indicator -> out_<name> fp32.
"""
import argparse
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _hydro_twin as twin  # noqa: E402

OUT = os.path.join(HERE, "hydro.npz")
NODATA = 777.5


def inputs(ref):
    raw = twin.rugged(97, 131, 61)
    small = twin.rugged(64, 80, 62, sea=0.35)
    nod = small.copy()
    nod[10:14, 30:36] = np.float32(NODATA)
    nod[50, 70] = np.float32(NODATA)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        filled = ref.fill_depressions_priority_flood(raw)
    return {
        "raw": raw,
        "filled": filled,
        "small": small,
        "nodata": nod,
        "all_ocean": twin.land_and_sea(16, 20, 63, sea=1.0) - np.float32(50.0),
        "all_land": twin.land_and_sea(24, 32, 64, sea=0.0) + np.float32(150.0),
        "t1x9": twin.land_and_sea(1, 9, 65, sea=0.3),
        "t9x1": twin.land_and_sea(9, 1, 66, sea=0.3),
        "t2x2": np.array([[5.0, 3.0], [4.0, 2.5]], np.float32),
        "t7x5": twin.land_and_sea(7, 5, 67, sea=0.3),
    }


def cases():
    c = []
    for i in ("raw", "small", "all_ocean", "all_land", "t1x9", "t9x1", "t2x2", "t7x5"):
        c.append((f"fill_{i}", "fill", i, {}))
    c += [("fill_raw_conn4", "fill", "raw", {"connectivity": 4}), ("fill_raw_eps0", "fill", "raw", {"epsilon": 0.0}),
          ("fill_raw_eps001", "fill", "raw", {"epsilon": 0.01}), ("fill_nodata", "fill", "nodata", {"nodata": NODATA}),
          ("fill_t7x5_conn4", "fill", "t7x5", {"connectivity": 4})]
    for i in ("raw", "filled", "small", "all_ocean", "all_land", "t1x9", "t9x1", "t2x2", "t7x5"):
        c.append((f"d8_{i}", "d8", i, {}))
        c.append((f"acc_{i}", "acc", i, {}))
    c.append(("d8_raw_tol05", "d8", "raw", {"tol": 0.5}))
    c += [("ind_raw", "indicator", "raw", {}), ("ind_raw_k2", "indicator", "raw", {"max_pool_kernel": 2}),
          ("ind_raw_k3", "indicator", "raw", {"max_pool_kernel": 3}), ("ind_filled_k2", "indicator", "filled", {"max_pool_kernel": 2}),
          ("ind_small_k3", "indicator", "small", {"max_pool_kernel": 3}), ("ind_t7x5_k2", "indicator", "t7x5", {"max_pool_kernel": 2}),
          ("ind_all_ocean", "indicator", "all_ocean", {})]
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"), help="root of a terrain-diffusion checkout")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set TD_REFERENCE")
    path = os.path.join(args.reference, "terrain_diffusion", "inference", "postprocessing.py")
    spec = importlib.util.spec_from_file_location("reference_postprocessing", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    ins = inputs(ref)
    data = {f"in_{k}": v for k, v in ins.items()}
    index = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for name, fn, key, kw in cases():
            z = ins[key].copy()
            W = z.shape[1]
            if fn == "fill":
                out = ref.fill_depressions_priority_flood(z, **kw)
                assert out.dtype == np.float32
                data[f"out_{name}"] = out
            elif fn == "d8":
                rr, cc, sink, kmax = ref.d8_flow(z, **kw)
                data[f"receiver_{name}"] = (rr * W + cc).astype(np.int32)
                data[f"kmax_{name}"] = kmax.astype(np.uint8)
                data[f"sink_{name}"] = sink.astype(bool)
            elif fn == "acc":
                rr, cc, sink, _ = ref.d8_flow(z)
                out = ref.flow_accumulation(z, rr, cc, sink)
                assert out.dtype == np.float32
                data[f"out_{name}"] = out
            else:
                out = ref.plot_flow_indicator(z, **kw)
                assert out.dtype == np.float32
                data[f"out_{name}"] = out
            index.append({"name": name, "fn": fn, "input": f"in_{key}", "kwargs": kw})
    data["cases"] = np.array(json.dumps(index))
    data["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(index)} cases")


if __name__ == "__main__":
    main()
