"""Generates tests/golden/rivers.npz by RUNNING THE REFERENCE'S OWN get_relief_map (terrain_diffusion/inference/relief_map.py:64-199, with its
biome, flow and rgb inputs) and smooth_river_bumps (terrain_diffusion/inference/postprocessing.py:87-135).

Needs a checkout of the reference (and the matplotlib / scipy / torch its two modules import); the fixture does not.  The modules are loaded
by path, so nothing else of the reference is imported.  Only inputs, keywords and outputs are stored, never source text:

    python tests/golden/make_rivers_golden.py --reference PATH_TO_REFERENCE_CHECKOUT      (or TD_REFERENCE=PATH)

Relief outputs are rounded to multiples of 2^-16 (at most 7.6e-6 off, inside the tests' 5e-5 / 1e-4 bounds) so that the compressed file stays
small; smoothing outputs are stored as they are.  Flows are the reference's own flow_accumulation of its own depression fill and D8 routing:
integer-valued, so none lies within an ulp of a threshold.  They are routed on the elevation LIFTED by some metres, so that rivers reach into
what the picture colours as ocean, and before the NaN holes are cut, so that rivers cross the holes.  Elevations are seeded
_relief_twin.land_and_sea canvases rounded to 1/8 m.  Each smoothing case also stores e_ref =
max |reference output - D64|, D64 = tests/_rivers_twin.smooth_d64 (the same formula in float64 from the same fp32 input): the reference's
own rounding error, which the GPU test's bound is a multiple of.
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
import _rivers_twin as twin  # noqa: E402

OUT = os.path.join(HERE, "rivers.npz")
QUANT = 2.0 ** -16


def load(reference, name):
    path = os.path.join(reference, "terrain_diffusion", "inference", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def flow_of(post, elev, lift):
    """the reference's flow accumulation of elev + lift (NaN -> ocean), depressions filled first so that rivers run to the coast"""
    z = np.nan_to_num(elev, nan=-1.0) + np.float32(lift)
    z = post.fill_depressions_priority_flood(z)
    rr, cc, sink, _ = post.d8_flow(z)
    a = post.flow_accumulation(z, rr, cc, sink)
    assert a.dtype == np.float32 and np.array_equal(a, np.round(a))
    return a


def biome_ids(shape, seed):
    """patches of ids from -2 to 34 with a block of zeros"""
    rng = np.random.default_rng(seed)
    H, W = shape
    coarse = rng.integers(-2, 35, size=((H + 3) // 4, (W + 4) // 5))
    b = np.kron(coarse, np.ones((4, 5), np.int64))[:H, :W].astype(np.int32)
    b[H // 3:H // 3 + max(1, H // 4), W // 4:W // 4 + max(1, W // 3)] = 0
    return b


def colours(shape, seed):
    """a caller's base colours: random 4 x 5 patches (they compress; the picture multiplies them pixel by pixel all the same)"""
    H, W = shape
    coarse = np.random.default_rng(seed).random(((H + 3) // 4, (W + 4) // 5, 3), dtype=np.float32)
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, 4, axis=0), 5, axis=1)[:H, :W])


def terrain(H, W, seed, **kw):
    """seeded land_and_sea, rounded to multiples of 1/8 m (the file stays below the size limit for a committed fixture)"""
    return (np.round(twin.land_and_sea(H, W, seed, **kw) * np.float32(8)) / np.float32(8)).astype(np.float32)


def holed(small, flow):
    """`small` with NaN holes: a block around the strongest river pixel on land and a second block (rivers cross both), a corner (its
    wrapped neighbours are the opposite edges), a last-row cell (the upper neighbour of row 0), a last-column cell and a single cell"""
    h = small.copy()
    y, x = np.unravel_index(np.argmax(np.where(small > 50, flow, 0)), small.shape)
    h[max(0, y - 2):y + 3, max(0, x - 6):x + 7] = np.nan
    h[5:9, 10:30] = np.nan
    h[0, 0] = h[63, 17] = h[40, 79] = h[40, 3] = np.nan
    return h


def relief_cases(post):
    """(name, elevation, {rgb, biome, flow}, keywords)."""
    canvas, small, t75, t29 = terrain(160, 224, 11), terrain(64, 80, 12), terrain(7, 5, 16), terrain(2, 9, 17)
    f_canvas, f_small = flow_of(post, canvas, 400.0), flow_of(post, small, 400.0)
    f75, f29 = flow_of(post, t75, 5000.0), flow_of(post, t29, 5000.0)
    holes_pos = holed(small, f_small)
    neg = terrain(64, 80, 14, sea=0.8)
    f_neg = flow_of(post, neg, 3000.0)
    holes_neg = neg.copy()
    holes_neg[20:26, 50:61] = np.nan
    y, x = np.unravel_index(np.argmax(f_neg), neg.shape)
    holes_neg[max(0, y - 3):y + 4, max(0, x - 3):x + 4] = np.nan   # a hole on a river: the (negative) median's ocean colour replaces it
    ocean = terrain(64, 80, 15, sea=1.0) - np.float32(50.0)
    f_ocean = flow_of(post, ocean, 20000.0)
    b_canvas, b_small = biome_ids(canvas.shape, 31), biome_ids(small.shape, 32)
    b75, b29 = biome_ids((7, 5), 33), biome_ids((2, 9), 34)
    c_small, c75, c29 = colours(small.shape, 41), colours((7, 5), 42), colours((2, 9), 43)
    return [
        ("biome_flow_canvas", canvas, dict(biome=b_canvas, flow=f_canvas), dict(resolution=30, relief=0.6, azimuths=(200.0,))),
        ("flow_small", small, dict(flow=f_small), {}),
        ("biome_small", small, dict(biome=b_small), {}),
        ("biome_flow_small", small, dict(biome=b_small, flow=f_small), dict(flow_threshold=3)),
        ("rgb_flow_small", small, dict(rgb=c_small, flow=f_small), dict(flow_threshold=2.5)),
        ("rgb_biome_small", small, dict(rgb=c_small, biome=b_small), dict(vmin=300.0, vmax=1200.0)),
        ("nan_pos_median", holes_pos, dict(flow=f_small), dict(flow_threshold=3)),
        ("nan_neg_median", holes_neg, dict(flow=f_neg), dict(flow_threshold=3)),
        ("all_ocean_flow", ocean, dict(flow=f_ocean), {}),
        ("flow_7x5", t75, dict(flow=f75), {}),
        ("flow_7x5_t3", t75, dict(flow=f75), dict(flow_threshold=3)),
        ("biome_flow_7x5", t75, dict(biome=b75, flow=f75), dict(flow_threshold=2.5)),
        ("rgb_flow_7x5", t75, dict(rgb=c75, flow=f75), dict(flow_threshold=3)),
        ("flow_2x9_t3", t29, dict(flow=f29), dict(flow_threshold=3)),
        ("flow_2x9_t2p5", t29, dict(flow=f29), dict(flow_threshold=2.5)),
        ("biome_2x9", t29, dict(biome=b29), {}),
        ("rgb_biome_2x9", t29, dict(rgb=c29, biome=b29), {}),
    ]


def smooth_cases(post):
    """(name, height, keywords)."""
    canvas, small, t75, t29 = terrain(160, 224, 11), terrain(64, 80, 12), terrain(7, 5, 16), terrain(2, 9, 17)
    holes = holed(small, flow_of(post, small, 400.0))   # the relief cases' holed image
    h75, h29 = t75.copy(), t29.copy()
    h75[0, 0] = h75[6, 2] = h75[3, 3] = np.nan
    h29[1, 8] = h29[0, 4] = np.nan
    k = np.float32(0.02)
    return [
        ("default_canvas", canvas, {}),
        ("default_small", small, {}),
        ("default_7x5", t75, {}),
        ("default_2x9", t29, {}),
        ("gentle_small", small * k, {}),
        ("gentle_7x5", t75 * k, {}),
        ("it0_7x5", t75, dict(iterations=0)),
        ("it0_holes_2x9", h29, dict(iterations=0)),
        ("it1_small", small, dict(iterations=1)),
        ("it8_holes_small", holes, dict(iterations=8)),
        ("it8_gentle_2x9", t29 * k, dict(iterations=8)),
        ("thresh200_small", small, dict(slope_thresh=200)),
        ("strength02_holes_small", holes, dict(smooth_strength=0.2)),
        ("strength02_7x5", t75, dict(smooth_strength=0.2)),
        ("holes_gentle_7x5", h75 * k, {}),
        ("holes_2x9", h29, {}),
        ("holes_gentle_2x9", h29 * k, dict(iterations=8)),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"), help="root of a terrain-diffusion checkout")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set TD_REFERENCE")
    rel, post = load(args.reference, "relief_map"), load(args.reference, "postprocessing")

    data, index, inputs = {}, [], {}

    def store(a):
        key = next((k for k, v in inputs.items() if v.shape == a.shape and v.dtype == a.dtype and np.array_equal(v, a, equal_nan=a.dtype.kind == "f")), None)
        if key is None:
            key = f"in_{len(inputs)}"
            inputs[key] = data[key] = a
        return key

    for name, elev, over, kw in relief_cases(post):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            out = rel.get_relief_map(elev, None, over.get("biome"), over.get("flow"), rgb=over.get("rgb"), **kw)
        assert out.dtype == np.float32 and out.shape == elev.shape + (3,), name
        data[f"out_{name}"] = (np.round(out.astype(np.float64) / QUANT) * QUANT).astype(np.float32)
        index.append({"name": name, "fn": "relief", "input": store(elev), "overlays": {k: store(v) for k, v in over.items()},
                      "kwargs": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}})
    for name, h, kw in smooth_cases(post):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            out = post.smooth_river_bumps(h, **kw)
        assert out.dtype == np.float32 and out.shape == h.shape, name
        d64 = twin.smooth_d64(h, **kw)
        assert np.array_equal(np.isnan(out), np.isnan(d64)), name
        e_ref = float(np.nanmax(np.abs(out.astype(np.float64) - d64)))
        data[f"out_{name}"] = out
        index.append({"name": name, "fn": "smooth", "input": store(h), "kwargs": kw, "e_ref": e_ref})
        print(f"{name:22s} e_ref {e_ref:.3e}  max|h| {np.nanmax(np.abs(h)):.4g}  max|out - in| {np.nanmax(np.abs(out - h)):.4g}")
    data["cases"] = np.array(json.dumps(index))
    data["biome_palette"] = rel._biome_palette()
    data["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(index)} cases")


if __name__ == "__main__":
    main()
