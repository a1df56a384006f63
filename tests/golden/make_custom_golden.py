"""Generates tests/golden/custom.npz by RUNNING THE REFERENCE'S OWN fill_nodata and h_to_meters (terrain_diffusion/inference/utils/
azgaar_to_tiff.py) and by reading its two tables as data: BIOME_VARIABILITY of that file and CHANNEL_FILES of inference/tiff_export.py.

Needs a checkout of the reference, numpy and scipy; the fixture does not.  Both modules import rasterio at the top, which is not required
here: the two functions are taken out with make_golden.extract_functions (only their FunctionDefs are executed) and the tables are read
from the syntax tree with ast.literal_eval (float("nan") entries through their string argument).  rasterize_layer and _load_and_pad need
rasterio itself and are not recorded; tests/test_custom_cpu.py holds them to independent checks.  Only inputs, outputs and library versions
are stored, never source text:

    python tests/golden/make_custom_golden.py --reference PATH_TO_REFERENCE_CHECKOUT      (or TD_REFERENCE=PATH)

Arrays: "cases" json [{"name", "nodata" (null = NaN), "out"}]; fill_in_<name> / fill_out_<out> float32 (H, W): an input of fill_nodata and what
the reference returned (valid pixels hold distinct integers, so an output pixel names its source; equal outputs are stored once); h_in (n, 4)
float64 rows of (h, exponent, ocean_max_depth, ocean_power) and h_out (n,) float64; biome_variability (13, 2) float64; channel_names,
channel_index, channel_scale, channel_default (NaN = None); constants json {"PADDING", "PIXELS_PER_CELL"}.
"""
import argparse
import ast
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "custom.npz")
F = np.float32


def literal(node):
    """ast.literal_eval, with float("...") calls evaluated through their literal argument."""
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "float" and len(node.args) == 1:
        return float(ast.literal_eval(node.args[0]))
    if isinstance(node, (ast.Tuple, ast.List)):
        return [literal(e) for e in node.elts]
    if isinstance(node, ast.Dict):
        return {literal(k): literal(v) for k, v in zip(node.keys, node.values)}
    return ast.literal_eval(node)


def assigned(path, name):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            return literal(node.value)
    raise KeyError(name)


def distinct(shape):
    """Distinct integer-valued float32 pixels (exact below 2^24)."""
    return np.arange(shape[0] * shape[1], dtype=F).reshape(shape) + F(1)


def fill_inputs():
    rng = np.random.default_rng(20240)
    cases = []
    big = rng.random((96, 160)) < 0.35
    big[30:70, 50:110] = True
    cases.append(("scattered_nan", big, None))
    cases.append(("scattered_sentinel", big, -9999.0))
    cases.append(("s7x5", rng.random((7, 5)) < 0.5, None))
    cases.append(("s1x9", np.array([[1, 1, 0, 1, 1, 1, 0, 1, 1]], bool), -9999.0))
    col = rng.random((33, 1)) < 0.6
    col[0], col[16] = True, False
    cases.append(("s33x1", col, None))
    lines = rng.random((40, 48)) < 0.3
    lines[:, 17] = True
    lines[23, :] = True
    cases.append(("lines", lines, -9999.0))
    single = np.ones((20, 20), bool)
    single[13, 6] = False
    cases.append(("single", single, None))
    cases.append(("no_hole", np.zeros((9, 11), bool), None))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"), help="root of a terrain-diffusion checkout")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set TD_REFERENCE")
    import scipy
    from scipy.ndimage import distance_transform_edt
    sys.path.insert(0, HERE)
    from make_golden import extract_functions
    azgaar = os.path.join(args.reference, "terrain_diffusion", "inference", "utils", "azgaar_to_tiff.py")
    export = os.path.join(args.reference, "terrain_diffusion", "inference", "tiff_export.py")
    ns = extract_functions(azgaar, {"fill_nodata", "h_to_meters"}, {"np": np, "distance_transform_edt": distance_transform_edt})
    data, index = {}, []

    for name, holes, nodata in fill_inputs():
        a = distinct(holes.shape)
        a[holes] = np.nan if nodata is None else nodata
        out = ns["fill_nodata"](a.copy(), float("nan") if nodata is None else nodata)
        assert out.dtype == F and out.shape == a.shape
        same = [c["out"] for c in index if np.array_equal(data["fill_out_" + c["out"]], out)]     # the sentinel twin of a NaN input: stored once
        data["fill_in_" + name] = a
        if not same:
            data["fill_out_" + name] = out
        index.append({"name": name, "nodata": nodata, "out": same[0] if same else name})
    assert [c["out"] for c in index if c["name"] == "scattered_sentinel"] == ["scattered_nan"]

    rows = [(h, e, d, p) for h in (0, 1, 5, 19, 19.5, 20, 21, 35, 50.25, 99, 100) for e, d, p in ((1.8, 4000.0, 1.5), (2.0, 6000.0, 1.0), (1.5, 2500.0, 2.2))]
    data["h_in"] = np.array(rows, np.float64)
    data["h_out"] = np.array([ns["h_to_meters"](*r) for r in rows], np.float64)

    table = assigned(azgaar, "BIOME_VARIABILITY")
    assert sorted(table) == list(range(13))
    data["biome_variability"] = np.array([table[k] for k in range(13)], np.float64)
    files = assigned(export, "CHANNEL_FILES")
    data["channel_names"] = np.array([f[0] for f in files])
    data["channel_index"] = np.array([f[1] for f in files], np.int64)
    data["channel_scale"] = np.array([f[2] for f in files], np.float64)
    data["channel_default"] = np.array([np.nan if f[3] is None else f[3] for f in files], np.float64)
    data["constants"] = np.array(json.dumps({"PADDING": assigned(export, "PADDING"), "PIXELS_PER_CELL": assigned(export, "PIXELS_PER_CELL")}))

    data["cases"] = np.array(json.dumps(index))
    data["versions"] = np.array(json.dumps({"numpy": np.__version__, "scipy": scipy.__version__}))
    # a fixed member order and timestamp: regenerating gives the same bytes
    import zipfile
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(data):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(data[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; {len(index)} fill cases, {len(rows)} heights")


if __name__ == "__main__":
    main()
