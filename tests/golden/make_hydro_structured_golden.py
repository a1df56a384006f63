"""Generates tests/golden/hydro_structured.npz by RUNNING THE REFERENCE'S OWN postprocessing.py (d8_flow, flow_accumulation,
plot_flow_indicator, fill_depressions_priority_flood) on the closed-form terrains of tests/_hydro_shapes.py: serpentine channels, one long
downhill chain, a comb, and integer surfaces on which d8 slopes tie.  tests/golden/hydro.npz and its maker stay as they are.

Needs a checkout of the reference (and the matplotlib / torch it imports); the fixture does not.  The module is loaded by path, so nothing else
of the reference is imported.  Only inputs, keywords, outputs and the numpy version are stored, never source text:

    python tests/golden/make_hydro_structured_golden.py --reference PATH_TO_REFERENCE_CHECKOUT      (or TD_REFERENCE=PATH)

The case index has make_hydro_golden.py's format, {"name", "fn" (fill | d8 | acc | indicator), "input", "kwargs"}, and the same outputs: fill
-> out_<name> fp32; d8 -> receiver_<name> (rr * W + cc, int32), kmax_<name> (uint8), sink_<name> (bool); acc -> out_<name> fp32; indicator
-> out_<name> fp32.  One addition: an acc case's kwargs are those of the d8_flow whose receivers it accumulates over (hydro.npz has none, so
it reads the same way) -- the steps surface is routed with tol = 0.5.
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
import _hydro_shapes as shapes  # noqa: E402

OUT = os.path.join(HERE, "hydro_structured.npz")
N_TIE = 33


def inputs(ref):
    ins = {
        "serp64": shapes.serpentine(64, 64),          # one tile
        "serp64x65": shapes.serpentine(64, 65),       # a second tile one cell wide
        "serp65x64": shapes.serpentine(65, 64),       # a second tile one cell high
        "serp130": shapes.serpentine(130, 130),       # 3 x 3 tiles, the edge tiles 2 cells wide
        "pit_linf257": shapes.pit_linf(257),
        "comb": shapes.comb(),
        "ramp64": shapes.ramp_serpentine(64, 64),
        "ramp130": shapes.ramp_serpentine(130, 130),
    }
    for name, make in shapes.TIE_SURFACES.items():
        ins[f"{name}{N_TIE}"] = make(N_TIE)
    ins["serp64_filled"] = ref.fill_depressions_priority_flood(ins["serp64"])   # slopes of about eps against tol
    return ins


def cases():
    c = [("fill_serp64", "fill", "serp64", {}), ("fill_serp64_conn4", "fill", "serp64", {"connectivity": 4}),
         ("fill_serp64_eps0", "fill", "serp64", {"epsilon": 0.0}), ("fill_serp64_eps001", "fill", "serp64", {"epsilon": 0.01}),
         ("fill_serp64x65", "fill", "serp64x65", {}), ("fill_serp65x64", "fill", "serp65x64", {}), ("fill_serp130", "fill", "serp130", {}),
         ("fill_pit_linf257", "fill", "pit_linf257", {})]
    routed = [(f"{name}{N_TIE}", f"{name}{N_TIE}", {}) for name in shapes.TIE_SURFACES]
    routed += [("pit_linf257", "pit_linf257", {}), (f"steps{N_TIE}_tol05", f"steps{N_TIE}", {"tol": 0.5}), ("comb", "comb", {}),
               ("ramp64", "ramp64", {}), ("ramp130", "ramp130", {}), ("serp64_filled", "serp64_filled", {})]
    for name, key, kw in routed:
        c.append((f"d8_{name}", "d8", key, kw))
        c.append((f"acc_{name}", "acc", key, kw))
    c += [("ind_comb_k3", "indicator", "comb", {"max_pool_kernel": 3}), ("ind_pit_linf257_k2", "indicator", "pit_linf257", {"max_pool_kernel": 2})]
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"), help="root of a terrain-diffusion checkout")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set TD_REFERENCE")
    path = os.path.join(args.reference, "terrain_diffusion", "inference", "postprocessing.py")
    spec = importlib.util.spec_from_file_location("reference_postprocessing", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ins = inputs(ref)
        data = {f"in_{k}": v for k, v in ins.items()}
        index = []
        for name, fn, key, kw in cases():
            z = ins[key].copy()
            assert z.dtype == np.float32
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
                rr, cc, sink, _ = ref.d8_flow(z, **kw)
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
    np.savez_compressed(args.out, **data)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(index)} cases")


if __name__ == "__main__":
    main()
