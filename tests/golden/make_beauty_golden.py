"""Generates tests/golden/beauty.npz by RUNNING THE REFERENCE'S OWN beauty_score.py (analyze_terrain_frequency, calculate_beauty_score) and
laplacian_encoder.py (laplacian_decode) on the committed cases of tests/_beauty_twin.py.

Needs a checkout of the reference, torch and click; the fixture needs none of them.  Both modules are loaded by path.  Their imports of h5py,
matplotlib, tqdm and torchvision are replaced by stub modules in sys.modules: names only, except torchvision.transforms.functional.resize, which
is F.interpolate(mode="bilinear", align_corners=False, antialias=True) -- the project's stated PARITY-UNPINNED equivalence
(terrain_diffusion_amd/composition.py).  Only inputs, outputs and library versions are stored, never source text:

    python tests/golden/make_beauty_golden.py --reference PATH_TO_REFERENCE_CHECKOUT      (or TD_REFERENCE=PATH)

Arrays:
  cases json {"spectrum": [{"name", "kind", "H", "W", "seed", "crc", "rho"}], "score": [{"name", "S", "ratio", "seed", "land", "crc", "rho",
      "share", "score", "std"}], "bins": [4, 7]}: crc = CRC-32 of the fp32 inputs _beauty_twin regenerates, rho = the relative L2 error of the
      reference's own fp32 torch.fft.fft2 against numpy's float64 fft2 of the same fp32 plane (for a score case: of the decoded plane);
  in_<name> fp32: the input plane of every spectrum case of 4096 values at most; low_<name>, res_<name> fp32 for every score case of 64 x 64;
  powers<bins>_<name> float64 (bins,): the reference's bin_powers; counts<bins>_<name> int64 (bins,): the members of every ring;
  features_<name> float64 (5,): the four bin_powers and the std the reference's calculate_beauty_score works from (score cases above the ocean rule);
  versions json.

The generator asserts what the tests lean on: min |F64_k| >= 64 rho ||x||_2 in every case but the flat plane; no share of pixels <= 0 between
0.98 and 0.995; every decoded value an exact zero or farther from zero than the decode's bound; no reference score within the score's bound of
a rounding edge.
"""
import argparse
import importlib.util
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _beauty_twin as twin  # noqa: E402

OUT = os.path.join(HERE, "beauty.npz")
F = np.float32


def install_stubs():
    import torch
    import torch.nn.functional as nnf

    def resize(img, size, interpolation=None, antialias=True):
        lead = img.shape[:-2]
        out = nnf.interpolate(img.reshape(-1, 1, *img.shape[-2:]).float(), size=tuple(int(s) for s in size), mode="bilinear", align_corners=False,
                              antialias=True)
        return out.reshape(*lead, *out.shape[-2:])

    tf = types.ModuleType("torchvision.transforms.functional")
    tf.resize = resize
    tf.InterpolationMode = types.SimpleNamespace(BILINEAR="bilinear")
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda it, **kw: it
    h5py = types.ModuleType("h5py")
    h5py.File, h5py.Group = object, object
    for name in ("torchvision", "torchvision.transforms", "matplotlib", "matplotlib.pyplot", "terrain_diffusion", "terrain_diffusion.data"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision.transforms.functional"] = tf
    sys.modules["torchvision.transforms"].functional = tf
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["tqdm"] = tqdm
    sys.modules["h5py"] = h5py


def load(reference, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(reference, "terrain_diffusion", *rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def rho_of(x32):
    import torch
    ref = torch.fft.fft2(torch.from_numpy(np.ascontiguousarray(x32, F))).numpy().astype(np.complex128)
    f64 = twin.spectrum(x32)
    return float(np.sqrt((np.abs(ref - f64) ** 2).sum() / (np.abs(f64) ** 2).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"), help="root of a terrain-diffusion checkout")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set TD_REFERENCE")
    import torch
    install_stubs()
    enc = load(args.reference, ("data", "laplacian_encoder.py"), "terrain_diffusion.data.laplacian_encoder")
    bs = load(args.reference, ("data", "preprocessing", "beauty_score.py"), "reference_beauty_score")
    data, spec_index, score_index = {}, [], []

    def record_bins(name, x32):
        for bins in twin.BINS:
            centres, powers = bs.analyze_terrain_frequency(torch.from_numpy(np.ascontiguousarray(x32)), bins)
            data[f"powers{bins}_{name}"] = np.array(powers, np.float64)
            data[f"counts{bins}_{name}"] = np.array([int(m.sum()) for m in twin.bin_masks(*x32.shape, bins)], np.int64)
            assert len(centres) == bins

    planes = twin.spectrum_planes()
    for name, kind, H, W, seed in twin.SPECTRUM_CASES:
        x = planes[name]
        rho = rho_of(x)
        if kind != "flat":
            least, norm = twin.min_magnitude(x)
            assert least >= twin.FLOOR_FACTOR * rho * norm, (name, least, rho, norm)
        if x.size <= 4096:
            data["in_" + name] = x
        record_bins(name, x)
        spec_index.append({"name": name, "kind": kind, "H": H, "W": W, "seed": seed, "crc": twin.crc(x), "rho": rho})

    for name, S, ratio, seed, land in twin.SCORE_CASES:
        low, res = twin.score_inputs(name)
        decoded = enc.laplacian_decode(torch.from_numpy(res), torch.from_numpy(low))
        squared = np.sign(decoded) * decoded**2                                        # beauty_score.py:63
        squared = torch.as_tensor(squared)
        share = torch.mean((squared <= 0).float()).item()
        assert not 0.98 <= share <= 0.995, (name, share)
        d, E, v, Ev, out = twin.decode_ref(low, res)
        assert ((d == 0) | (np.abs(d) > E)).all(), name                                # the count of pixels <= 0 does not hinge on a rounding
        assert int((v <= 0).sum()) == int((squared <= 0).sum()), name
        score = bs.calculate_beauty_score(torch.from_numpy(low), torch.from_numpy(res))
        clamped = torch.where(squared < 0, torch.zeros_like(squared), squared)
        rho = rho_of(clamped.numpy())
        entry = {"name": name, "S": S, "ratio": ratio, "seed": seed, "land": land, "crc": twin.crc(low, res), "rho": rho, "share": share,
                 "score": score, "std": torch.std(clamped).item()}
        if share > 0.99:
            assert score == 1.0
        else:
            least, norm = twin.min_magnitude(clamped.numpy())
            assert least >= twin.FLOOR_FACTOR * rho * norm, (name, least, rho, norm)
            _, powers = bs.analyze_terrain_frequency(clamped, bins=4)
            data["features_" + name] = np.array(powers + [entry["std"]], np.float64)
            ref = twin.score_ref(low, res, rho)
            edge = abs(score - (np.floor(score) + 0.5))
            assert edge > ref["score_bound"] and abs(score - ref["score"]) <= ref["score_bound"], (name, score, ref["score"], ref["score_bound"])
        if S <= 64:
            data["low_" + name], data["res_" + name] = low, res
        score_index.append(entry)

    data["cases"] = np.array(json.dumps({"spectrum": spec_index, "score": score_index, "bins": list(twin.BINS)}))
    data["versions"] = np.array(json.dumps({"numpy": np.__version__, "torch": torch.__version__}))
    # a fixed member order and timestamp: regenerating gives the same bytes
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(data):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(data[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; {len(spec_index)} spectrum cases, {len(score_index)} score cases")
    for e in spec_index:
        print(f"  {e['name']:16s} rho_ref {e['rho']:.3e}")
    for e in score_index:
        print(f"  {e['name']:16s} rho_ref {e['rho']:.3e} share {e['share']:.4f} score {e['score']:.6f}")


if __name__ == "__main__":
    main()
