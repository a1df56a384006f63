"""Generates tests/golden/coarse.npz: what the reference's own fill_oceans (terrain_diffusion/training/datasets/coarse_dataset.py:17-220), torch
and NumPy give on the committed cases of tests/_coarse_twin.py.

Needs a checkout of the reference, numpy, scipy and torch; the fixture needs none of them.  coarse_dataset.py imports rasterio, h5py, skimage and
tqdm at the top, which are not required here: only fill_oceans' FunctionDef is executed (make_golden.extract_functions) with np, sparse, zoom and a
cg wrapper that counts scipy's callbacks.  Only outputs, counts and library versions are stored, never source text:

    python tests/golden/make_coarse_golden.py --reference PATH_TO_REFERENCE_CHECKOUT      (or TD_REFERENCE=PATH)

Arrays:
  fill_names json [name]; fill_out_<name> float64 (H, W): the reference's output; fill_info_<name> int32[4]: scipy's callback count and info of the
      coarse and the fine solve (zeros where the reference returns before it solves); fill_raises json {name: exception type} for the cases
      on which the reference raises (no output is stored for them);
  fill_ratio float64 (cases, orders): max|twin - reference| / (2^-52 max|land| (coarse + fine iterations)) per case and summation order of the
      twin (_coarse_twin.ORDERS), 0 where no iteration ran; fill_ratio_max its maximum: CG_MEASURED_RATIO of the twin is this, rounded up;
  resize_w<W_out> float32 (H, W_out): F.interpolate(mode='area') of _coarse_twin.resize_input();
  tile_<stat>_t<t> float32: np.mean / np.nanmean / np.quantile(0.05) over the tiles of _coarse_twin.tile_input(), stat in mean, nanmean, quantile;
  crop_c<c> float32 (N,): torch's score (:396-403) of the crops of _coarse_twin.crop_input();
  versions json.

The generator refuses a fill case whose residual norm at one of the last two stop tests lies within a relative 1e-6 of the threshold (in any of
the twin's summation orders): its iteration count would be a coin toss.  Pick another seed in _coarse_twin.FILL_SEEDS then.
"""
import argparse
import io
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "coarse.npz")
F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"), help="root of a terrain-diffusion checkout")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set TD_REFERENCE")
    import scipy
    import torch
    from scipy import sparse
    from scipy.ndimage import zoom
    from scipy.sparse.linalg import cg as scipy_cg
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from make_golden import extract_functions
    import _coarse_twin as twin
    data = {}

    calls = []

    def cg(A, b, **kw):
        count = [0]

        def callback(xk):
            count[0] += 1
        x, info = scipy_cg(A, b, callback=callback, **kw)
        calls.append((count[0], int(info)))
        return x, info
    path = os.path.join(args.reference, "terrain_diffusion", "training", "datasets", "coarse_dataset.py")
    ns = extract_functions(path, {"fill_oceans"}, {"np": np, "sparse": sparse, "zoom": zoom, "cg": cg, "print": lambda *a, **k: None})

    names, raises, ratios = [], {}, []
    for name, (a, kw) in twin.fill_cases().items():
        assert a.shape[0] <= 64 and a.shape[1] <= 160, name
        del calls[:]
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ref = ns["fill_oceans"](a, tol=twin.FILL_TOL, **kw)
        except Exception as e:                              # recorded: the library refuses such an input
            raises[name] = type(e).__name__
            print(f"{name}: the reference raises {type(e).__name__}: {e}")
            continue
        info = np.zeros(4, np.int32)
        if calls:
            assert len(calls) == 2, (name, calls)
            info[:] = (calls[0][0], calls[0][1], calls[1][0], calls[1][1])
        names.append(name)
        data["fill_out_" + name] = np.asarray(ref, np.float64)
        data["fill_info_" + name] = info
        land = a[~np.isnan(a)]
        iters = int(info[0] + info[2])
        row = []
        for order in twin.ORDERS:
            traces = ([], [])
            got, tinfo = twin.fill_oceans(a, tol=twin.FILL_TOL, order=order, traces=traces, **kw)
            assert np.array_equal(tinfo, info), (name, order, tinfo, info)
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            for level, trace in enumerate(traces):
                thr = None
                if trace:
                    ocean = np.isnan(a) if level else np.isnan(twin.block_nanmean(a, int(kw.get("multires_factor", 8))))
                    src = a if level else twin.block_nanmean(a, int(kw.get("multires_factor", 8)))
                    _, b = twin.system(src, ocean)
                    thr = max(twin.FILL_TOL, 1e-5 * float(np.sqrt(np.sum(b[ocean] ** 2))))
                for rn in trace[-2:]:
                    if abs(rn - thr) <= 1e-6 * thr:
                        raise SystemExit(f"{name} ({order}, level {level}): |r| = {rn!r} within 1e-6 of the threshold {thr!r}: pick another seed")
            err = float(np.nanmax(np.abs(got - ref))) if np.isnan(a).any() and not np.isnan(ref).all() else 0.0
            row.append(err / (2.0 ** -52 * float(np.abs(land).max()) * iters) if iters and land.size else 0.0)
            if not iters:
                assert err <= 2.0 ** -52 * (float(np.abs(land).max()) if land.size else 1.0), (name, order, err)
        ratios.append(row)
        print(f"{name}: {a.shape}, {int(np.isnan(a).sum())} unknowns, info {info.tolist()}, ratio per order {[round(r, 3) for r in row]}")
    data["fill_names"] = np.array(json.dumps(names))
    data["fill_raises"] = np.array(json.dumps(raises))
    data["fill_ratio"] = np.array(ratios, np.float64)
    data["fill_ratio_max"] = np.float64(np.max(ratios))
    print(f"largest ratio {np.max(ratios):.4f}; the twin states CG_MEASURED_RATIO = {twin.CG_MEASURED_RATIO}")
    assert np.max(ratios) <= twin.CG_MEASURED_RATIO <= 1.3 * np.max(ratios) + 0.01, "update CG_MEASURED_RATIO in tests/_coarse_twin.py"

    x = twin.resize_input()
    for w_out in twin.RESIZE_W_OUT:
        got = torch.nn.functional.interpolate(torch.from_numpy(x)[None, None], size=(x.shape[0], w_out), mode="area")[0, 0].numpy()
        d64, bound = twin.area_resize_w(x, w_out)
        assert np.array_equal(np.isnan(got), np.isnan(d64)) and np.all(np.abs(got - d64)[~np.isnan(d64)] <= bound[~np.isnan(d64)]), w_out
        data[f"resize_w{w_out}"] = got.astype(F)

    x = twin.tile_input()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for t in twin.TILE_TS:
            tl = twin.tiles_of(x, t)
            data[f"tile_mean_t{t}"] = tl.mean(-1).astype(F)
            data[f"tile_nanmean_t{t}"] = np.nanmean(tl, -1).astype(F)
            data[f"tile_quantile_t{t}"] = np.quantile(tl, q=twin.TILE_Q, axis=-1).astype(F)
            assert data[f"tile_mean_t{t}"].dtype == F and tl.dtype == F

    plane, mean0, std0, offsets = twin.crop_input()
    tp = torch.from_numpy(plane)
    for c in twin.CROP_CS:
        out = []
        for i, j in offsets[c]:
            crop0 = tp[i:i + c, j:j + c]
            elev_sqrt = crop0 * float(std0) + float(mean0)
            elev = torch.sign(elev_sqrt) * torch.square(elev_sqrt)
            elev_zerod = torch.where(elev < 0, torch.zeros_like(elev), elev)
            img = elev_zerod.unsqueeze(0).unsqueeze(0)
            blurred = torch.nn.functional.avg_pool2d(img, kernel_size=3, stride=1, padding=1)
            out.append(float(torch.quantile((img - blurred) ** 2, q=twin.CROP_Q)))
        want, bound = twin.crop_scores(plane, mean0, std0, offsets[c], c)
        worst = float(np.max(np.abs(np.array(out) - want) / bound))
        print(f"crop scores c = {c}: torch within {worst:.3f} of the bound")
        assert worst <= 1.0, (c, worst)
        data[f"crop_c{c}"] = np.array(out, F)

    data["versions"] = np.array(json.dumps({"numpy": np.__version__, "scipy": scipy.__version__, "torch": torch.__version__.split("+")[0]}))
    import zipfile
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(data):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(data[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; {len(names)} fill cases ({len(raises)} more raise)")


if __name__ == "__main__":
    main()
