"""Generates tests/golden/relief.npz by RUNNING THE REFERENCE'S OWN relief_map.py (terrain_diffusion/inference/relief_map.py:64-199).

Needs a checkout of the reference (and the matplotlib / scipy it imports); the fixture does not.  The module is loaded by path, so nothing
else of the reference is imported.  Only inputs, keywords and outputs are stored, never source text:

    python tests/golden/make_relief_golden.py --reference PATH_TO_REFERENCE_CHECKOUT      (or TD_REFERENCE=PATH)

Outputs are rounded to multiples of 2^-16 (at most 7.6e-6 off, inside the tests' 5e-5 / 1e-4 bounds) so that the compressed file stays small.
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
import _relief_twin as twin  # noqa: E402

OUT = os.path.join(HERE, "relief.npz")
QUANT = 2.0 ** -16


def cases():
    """(name, input, keywords)."""
    canvas = twin.land_and_sea(160, 224, 11)
    small = twin.land_and_sea(64, 80, 12)
    land = twin.land_and_sea(64, 80, 13, sea=0.0) + np.float32(150.0)
    holes_pos = small.copy()
    holes_pos[5:9, 10:30] = np.nan
    holes_pos[40, 3] = np.nan
    holes_neg = twin.land_and_sea(64, 80, 14, sea=0.8)
    holes_neg[20:26, 50:61] = np.nan
    ocean = twin.land_and_sea(48, 64, 15, sea=1.0) - np.float32(50.0)
    return [
        ("default", canvas, {}),
        ("params", canvas, dict(resolution=30, relief=0.6, sigma_large=3.0, sigma_small=0.8, azimuths=(200.0,))),
        ("all_land", land, {}),
        ("explicit_range", small, dict(vmin=300.0, vmax=1200.0)),
        ("nan_pos_median", holes_pos, {}),
        ("nan_neg_median", holes_neg, {}),
        ("constant", np.full((16, 20), 123.5, np.float32), {}),
        ("all_ocean", ocean, {}),
        ("tiny_7x5", twin.land_and_sea(7, 5, 16), {}),
        ("tiny_2x9", twin.land_and_sea(2, 9, 17), {}),
        ("narrow_31x97", twin.land_and_sea(31, 97, 18), {}),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"), help="root of a terrain-diffusion checkout")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set TD_REFERENCE")
    path = os.path.join(args.reference, "terrain_diffusion", "inference", "relief_map.py")
    spec = importlib.util.spec_from_file_location("reference_relief_map", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import matplotlib.pyplot as plt
    from scipy.ndimage import gaussian_filter

    data, index = {}, []
    inputs = {}
    for name, elev, kw in cases():
        key = next((k for k, v in inputs.items() if v.shape == elev.shape and np.array_equal(v, elev, equal_nan=True)), None)
        if key is None:
            key = f"in_{len(inputs)}"
            inputs[key] = elev
            data[key] = elev
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            out = mod.get_relief_map(elev, None, None, None, **kw)
        assert out.dtype == np.float32 and out.shape == elev.shape + (3,)
        data[f"out_{name}"] = (np.round(out.astype(np.float64) / QUANT) * QUANT).astype(np.float32)
        index.append({"name": name, "input": key, "kwargs": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}})
    data["cases"] = np.array(json.dumps(index))
    data["terrain_lut"] = plt.get_cmap("terrain")(np.arange(256))[:, :3].astype(np.float64)
    for sigma in (6.0, 1.2, 3.0, 0.8):
        r = int(4.0 * sigma + 0.5)
        imp = np.zeros(2 * r + 1, np.float64)
        imp[r] = 1.0
        data[f"impulse_{sigma}"] = gaussian_filter(imp, sigma, mode="constant")   # the 1-D weights, read back through scipy
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(index)} cases")


if __name__ == "__main__":
    main()
