"""Generates tests/golden/dataset.npz: what SciPy, NumPy and the reference's own calculate_stats_welford (terrain_diffusion/data/preprocessing/
calculate_stds.py) give on the committed cases of tests/_dataset_twin.py.

Needs a checkout of the reference, numpy and scipy; the fixture needs neither.  calculate_stds.py imports click, h5py, matplotlib and tqdm at the
top, which are not required here: only the function's FunctionDef is executed (make_golden.extract_functions), with a pass-through tqdm, over a
dict-shaped group.  Only inputs' identities, outputs and library versions are stored, never source text:

    python tests/golden/make_dataset_golden.py --reference PATH_TO_REFERENCE_CHECKOUT      (or TD_REFERENCE=PATH)

Arrays:
  void_names json [name]; void_mask_<name> uint8 (H, W) (1 = void) and void_edt_<name> float64 (H, W) = scipy.ndimage.distance_transform_edt of the
      mask, for every case of _dataset_twin.void_cases() that holds a valid pixel (the inputs themselves are made by that function);
  median_in float32 (96, 192) and median_r<r> float32 (96 / r, 192 / r) = np.median of every r x r block on its own, r in 1, 2, 3, 8, 16, 32;
  stats json {"crc": CRC-32 of the group's arrays (made by _dataset_twin.stats_group from the project's portable generator), "n": values per 2-D
      chunk, "chunks": their number}; stats_<dataset>_<feed>_<pct>_means / _stds float64: the reference's outputs for dataset residual (2-D) /
      climate (3-D), the arrays fed as float32 (f32) or cast to float64 (f64), min_stat_landcover_pct 0.0 (p0) or 0.4 (p4);
  versions json.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "dataset.npz")
F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"), help="root of a terrain-diffusion checkout")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set TD_REFERENCE")
    import scipy
    from scipy.ndimage import distance_transform_edt
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from make_golden import extract_functions
    import _dataset_twin as twin
    data = {}

    names = []
    for name, (dem, _) in twin.void_cases().items():
        mask = np.isnan(dem)
        if mask.all():
            continue                                        # no valid pixel: the reference takes the base, there is no distance to record
        names.append(name)
        data["void_mask_" + name] = mask.astype(np.uint8)
        data["void_edt_" + name] = distance_transform_edt(mask).astype(np.float64)
    data["void_names"] = np.array(json.dumps(names))

    x = twin.median_input()
    data["median_in"] = x
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for r in twin.MEDIAN_RS:
            blocks = twin.blocks_of(x, r)
            data[f"median_r{r}"] = np.array([[np.median(blocks[i, j]) for j in range(blocks.shape[1])] for i in range(blocks.shape[0])], F)

    stds_py = os.path.join(args.reference, "terrain_diffusion", "data", "preprocessing", "calculate_stds.py")
    ns = extract_functions(stds_py, {"calculate_stats_welford"}, {"np": np, "tqdm": lambda it, **kw: it})
    group = twin.stats_group()
    n_chunks = len(group)
    data["stats"] = np.array(json.dumps({"crc": twin.group_crc(group), "n": int(group["0"]["chunk_0_0"]["residual"].array.size), "chunks": n_chunks}))
    for feed, g in (("f32", group), ("f64", twin.cast_group(group, np.float64))):
        for tag, pct in (("p0", 0.0), ("p4", 0.4)):
            for name in ("residual", "climate"):
                with contextlib.redirect_stdout(io.StringIO()):
                    means, stds = ns["calculate_stats_welford"](g, name, pct)
                data[f"stats_{name}_{feed}_{tag}_means"] = np.asarray(means, np.float64)
                data[f"stats_{name}_{feed}_{tag}_stds"] = np.asarray(stds, np.float64)

    data["versions"] = np.array(json.dumps({"numpy": np.__version__, "scipy": scipy.__version__}))
    # a fixed member order and timestamp: regenerating gives the same bytes
    import zipfile
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(data):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(data[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; {len(names)} void masks, {len(twin.MEDIAN_RS)} block sizes, {n_chunks} chunks of statistics")


if __name__ == "__main__":
    main()
