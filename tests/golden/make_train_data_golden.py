"""Generates tests/golden/train_data.npz by RUNNING THE REFERENCE'S OWN three dataset classes -- H5LatentsDataset, H5DecoderTerrainDataset,
H5AutoencoderDataset (terrain_diffusion/training/datasets/) -- on the committed tree of tests/_train_data_twin.py.

Needs a checkout of the reference and torch; the fixture needs neither.  The three modules and models/mp_layers.py are loaded by path.  Their
imports of h5py, torchvision and tqdm are replaced by stub modules in sys.modules, as make_beauty_golden.py does; h5py.File(path) returns the
in-memory tree (tests/_train_data_twin.py TREE(): dicts of NumPy arrays with .attrs).  torch.randn / rand / randint / multinomial are wrapped
while an item is built so that every draw made with a generator is recorded in order; a FORCED item replaces chosen randint results (the key
index, i, j, transform_idx) and records the replacement.  The autoencoder class keeps its keys in set order, which changes from one
interpreter to the next: the generator sorts them after construction, as train_data.H5AutoencoderDataset does.  Only inputs' checksums,
draws, outputs and library versions are stored, never source text:

    python tests/golden/make_train_data_golden.py --reference PATH_TO_REFERENCE_CHECKOUT      (or TD_REFERENCE=PATH)

Arrays:
  cases json {"configs": {name: constructor arguments}, "items": [...], "runs": {name: {"config", "seed", "items": [...]}}, "tree_crc",
      "keys": {config: key lists}}.  An item: {"name", "cls", "config", "path", "i", "j", "t", "forced", "full", "draws": [[fn, shape, key or
      null, crc]]}; a draw of more than 1024 values is stored only for a `full` item;
  <item>_<key>: image (`full` items) / its lowfreq channel (forced items) / cond_img / cond_inputs / cond_inputs_img / histogram_raw / noise_level / lowfreq / lowfreq_padded;
  <item>_raw (7, g, g): the reference's own _get_cond_image of the same window without dropout, noise or normalisation;
  <item>_m64 (5, g, g) float64: the correctly rounded float64 block means (math.fsum) of lowres_exact and the four climate planes;
  <item>_eref (5, g, g) float64: |raw - m64|, the reference's own error;
  versions json.

The generator asserts what the tests lean on: no exp argument within 2^-20 relative of a half rounding midpoint; no tie between a +0 and a
-0 at the selected ranks; no uniform within 1 ulp of the dropout threshold fl32(p) except in the one item whose uniforms are all forced ONTO it (torch compares in
fp32, so `>` and `>=` part there and nowhere else); every transform forced; a run of at least 12 items with and without NaN climate centres.
"""
import argparse
import importlib.util
import io
import json
import math
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _train_data_twin as twin  # noqa: E402

OUT = os.path.join(HERE, "train_data.npz")
F = np.float32
BIG = 1024

COND_MEAN = [13.36, 10.03, 16.17, 612.99, 869.73, 71.64, 0.674]
COND_STD = [22.22, 22.13, 10.23, 453.81, 797.71, 34.23, 0.460]
LAT = dict(h5_file="tree", pct_land_ranges=[[0, 0.01], [0.01, 1]], subset_resolutions=[90, 90], subset_weights=[0.1, 0.9],
           latents_mean=[0.1, -0.2, 0.05, 0.0], latents_std=[1.1, 0.9, 1.3, 0.7], sigma_data=0.5, split="train", beauty_dist=[False, True],
           residual_mean=0.0, residual_std=1.1678, cond_input_mean=COND_MEAN, cond_input_std=COND_STD)
DEC = dict(h5_file="tree", pct_land_ranges=[[0, 0.01], [0.01, 1]], subset_resolutions=[90, 90], subset_weights=[0.1, 0.9], split="train",
           residual_mean=0.05, residual_std=1.1678, sigma_data=0.5)
CONFIGS = {
    "LA": ("latents", dict(LAT, crop_size=64, clip_edges=True, cond_input_dropout=0.2, cond_input_max_noise=0.1)),
    "LB": ("latents", dict(LAT, crop_size=96, clip_edges=False, pct_land_ranges=[[0, 0.01], [0.7, 1]])),
    "LC": ("latents", dict(LAT, crop_size=64, clip_edges=True, eval_dataset=True, cond_input_max_noise=0.1)),
    "LD": ("latents", dict(LAT, crop_size=64, clip_edges=False, cond_input_dropout=0.2, pct_land_ranges=[None, [0.01, 1]],
                           subset_resolutions=[30, 90], subset_class_labels=[0, 1])),
    "DA": ("decoder", dict(DEC, crop_size=16, clip_edges=True)),
    "DB": ("decoder", dict(DEC, crop_size=24, clip_edges=True, subset_class_labels=[2, 3], sigma_data=1.0)),      # clip_edges=False: the reference fails
    "DC": ("decoder", dict(DEC, crop_size=64, clip_edges=True, eval_dataset=True)),
    "AA": ("autoencoder", dict(h5_file="tree", crop_size=32, pct_land_ranges=[[0, 0.01], [0.01, 1]], subset_resolutions=[90, 90],
                               subset_weights=[0.1, 0.9], split="train", residual_mean=0.05, residual_std=1.17)),
    "AB": ("autoencoder", dict(h5_file="tree", crop_size=24, pct_land_ranges=[None], subset_resolutions=[90], subset_class_labels=[4],
                               residual_mean=-0.1, residual_std=0.9)),
}
# seeded runs of successive items: (config, seed, count)
RUNS = {"runLA": ("LA", 1234, 14), "runLB": ("LB", 77, 4), "runLC": ("LC", 5, 3), "runLD": ("LD", 99, 4), "runDA": ("DA", 31, 4), "runDB": ("DB", 32, 3),
        "runDC": ("DC", 33, 2), "runAA": ("AA", 41, 4), "runAB": ("AB", 42, 3)}
# forced items: (config, seed, [key index, i, j, transform_idx], full); None leaves the draw, a float is a share of the draw's own range
# (0.0 its least value, 1.0 its largest: windows against every side and corner of whatever group is drawn), an int is the value itself
FORCED = (
    [("LA", 500 + t, [None, (0.0, 1.0, 0.5, 0.0, 1.0, 0.6, 0.15, 0.85)[t], (0.0, 1.0, 0.0, 1.0, 0.4, 0.05, 0.95, 0.2)[t], t], t == 6) for t in range(8)]
    + [("LB", 520, [None, 0.0, 1.0, 5], False), ("LB", 521, [None, 1.0, 0.0, 3], False),
       ("LD", 530, [None, 0.0, 1.0, 2], False), ("LD", 531, [None, 1.0, 0.0, 7], False),
       # every dropout uniform ON the threshold fl32(0.2): torch compares in fp32, `>` drops every block and `>=` would keep every one
       ("LA", 540, [None, 0.0, 0.0, 3, "u_drop_on_threshold"], False)]
    + [("DA", 600 + t, [None, (0.0, 1.0, 0.5, 0.0, 1.0, 0.3, 0.8, 0.6)[t], (0.0, 1.0, 0.0, 1.0, 0.6, 0.9, 0.4, 0.1)[t], t], False) for t in range(8)]
    + [("DB", 620, [None, 0.0, 0.0, 1], False), ("DB", 621, [None, 1.0, 1.0, 4], False)]
    + [("AA", 700 + t, [None, (0.0, 1.0, 0.3, 0.6, 0.0, 1.0, 0.7, 0.2)[t], (0.0, 1.0, 0.6, 0.3, 1.0, 0.0, 0.1, 0.5)[t], t], False) for t in range(8)]
)


# ------------------------------------------------------------------------------------------------------------------------------ the reference
def install_stubs():
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda it, **kw: it
    h5py = types.ModuleType("h5py")
    h5py.File = lambda path, mode="r": twin.TREE()
    enc = types.ModuleType("terrain_diffusion.data.laplacian_encoder")
    enc.laplacian_decode = enc.laplacian_encode = None
    for name in ("torchvision", "terrain_diffusion", "terrain_diffusion.data", "terrain_diffusion.models"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["tqdm"], sys.modules["h5py"], sys.modules["terrain_diffusion.data.laplacian_encoder"] = tqdm, h5py, enc


def load(reference, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(reference, "terrain_diffusion", *rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class Recorder:
    """wraps torch's four draw functions: records every draw made with generator=, replaces randint results from `force`"""

    def __init__(self, torch):
        self.torch, self.draws, self.force, self.names = torch, [], [], ("randn", "rand", "randint", "multinomial")
        self.orig = {n: getattr(torch, n) for n in self.names}

    def __enter__(self):
        for n in self.names:
            setattr(self.torch, n, self.wrap(n))
        return self

    def __exit__(self, *exc):
        for n in self.names:
            setattr(self.torch, n, self.orig[n])
        return False

    def wrap(self, name):
        def fn(*a, **k):
            out = self.orig[name](*a, **k)
            if k.get("generator") is not None:
                if name == "randint" and self.force:
                    v = self.force.pop(0)
                    low, high = (0, a[0]) if not isinstance(a[1], int) else (a[0], a[1])
                    if isinstance(v, float):
                        v = low + int(round(v * (high - 1 - low)))
                    if v is not None:
                        assert low <= v < high, (v, low, high)
                        out = self.torch.full_like(out, v)
                if name == "rand" and out.dim() == 3 and "u_drop_on_threshold" in self.force:
                    out = self.torch.full_like(out, self.on_threshold)
                self.draws.append((name, out.clone()))
            return out
        return fn

    def item(self, ds, force):
        self.draws, self.force = [], list(force or [])
        self.on_threshold = getattr(ds, "cond_input_dropout", 0.0)
        out = ds[0]
        return out, self.draws


def name_draws(cls, cfg, draws):
    """the role of every draw of one item, from the order the classes make them in"""
    keys, k = [], 0
    seq = [d[0] for d in draws]
    if cls == "latents":
        keys = ["subset", "histogram_raw"]
        if seq[2] == "multinomial":
            keys.append("beauty")
        keys.append("index")
        if not cfg.get("eval_dataset"):
            keys += ["i", "j", "t"]
        keys.append("noise")
        if cfg.get("cond_input_dropout"):
            keys.append("u_drop")
        if cfg.get("cond_input_max_noise"):
            keys += ["u_noise", "z_mean", "z_p5"]
        keys.append("z_replace")                     # drawn even when no centre is NaN (an empty draw)
    elif cls == "decoder":
        keys = ["subset", "index"] + ([] if cfg.get("eval_dataset") else ["i", "j", "t"]) + ["noise"]
    else:
        keys = ["subset", "index", "i8", "j8", "t"]
    assert len(keys) == len(draws), (cls, keys, seq)
    return keys


def exact_block_means(v):
    b = twin.blocks_of(v.astype(np.float64))
    out = np.empty(b.shape[:-1])
    for idx in np.ndindex(*out.shape):
        out[idx] = math.fsum(b[idx]) / 1024.0 if not np.isnan(b[idx]).any() else np.nan
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"), help="root of a terrain-diffusion checkout")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set TD_REFERENCE")
    import torch
    install_stubs()
    load(args.reference, ("models", "mp_layers.py"), "terrain_diffusion.models.mp_layers")
    classes = {
        "latents": load(args.reference, ("training", "datasets", "h5_latents_dataset.py"), "reference_h5_latents").H5LatentsDataset,
        "decoder": load(args.reference, ("training", "datasets", "h5_decoder_terrain_dataset.py"), "reference_h5_decoder").H5DecoderTerrainDataset,
        "autoencoder": load(args.reference, ("training", "datasets", "h5_autoencoder_dataset.py"), "reference_h5_autoencoder").H5AutoencoderDataset,
    }
    tree = twin.TREE()
    data, items, runs, key_lists = {}, [], {}, {}
    sides = {f"{g[0]}/{g[1]}/{g[2]}": g[3] for g in twin.GROUPS}
    for path in sides:                                                       # what the latent tests lean on
        assert twin.exp_midpoint_distance(tree[path]["latent"].array[:, twin.LC:]) > 2.0 ** -20, path

    def build(name):
        cls, cfg = CONFIGS[name]
        ds = classes[cls](**cfg)
        if cls == "autoencoder":
            ds.keys = [sorted(k) for k in ds.keys]
        return ds

    raw_ds = build("LB")                    # no dropout, no noise; its means are taken away below: the reference's own unnormalised branch
    raw_ds.cond_input_mean = None
    seen_t = {"latents": set(), "decoder": set(), "autoencoder": set()}

    def record(rec, ds, name, cfg_name, force, full):
        cls, cfg = CONFIGS[cfg_name]
        out, draws = rec.item(ds, force)
        keys = name_draws(cls, cfg, draws)
        got = dict(zip(keys, (d[1] for d in draws)))
        index, subset = int(got["index"]), int(got["subset"])
        crop = cfg["crop_size"]
        if cls == "latents":
            path = out["path"]
            S = sides[path]
            t = int(got["t"]) if "t" in got else 0
            i, j = (int(got["i"]), int(got["j"])) if "i" in got else ((S - crop) // 2,) * 2
        elif cls == "decoder":
            path = out["path"]
            S = sides[path]
            t = int(got["t"]) if "t" in got else 0
            i, j = (int(got["i"]), int(got["j"])) if "i" in got else ((S - crop // 8) // 2,) * 2
        else:
            chunk, res, sub = ds.keys[subset][index]
            path = f"{res}/{chunk}/{sub}"
            t, i, j = int(got["t"]), int(got["i8"]) * 8, int(got["j8"]) * 8
        seen_t[cls].add(t)
        entry = {"name": name, "cls": cls, "config": cfg_name, "path": path, "i": i, "j": j, "t": t, "subset": subset, "forced": force is not None,
                 "full": bool(full), "draws": []}
        for key, (fn, val) in zip(keys, draws):
            arr = val.numpy()
            stored = arr.size <= BIG or full
            if stored:
                data[f"{name}_d_{key}"] = arr
            entry["draws"].append([fn, list(arr.shape), key if stored else None, twin.crc(arr)])
        if cls == "latents":
            img = out["image"].numpy()
            if full:
                data[f"{name}_image"] = img
            elif force is not None:
                data[f"{name}_lowfreq"] = img[-1]
            entry["image_crc"] = twin.crc(img)
            data[f"{name}_cond_inputs"] = out["cond_inputs"][0].numpy()
            data[f"{name}_cond_inputs_img"] = out["cond_inputs_img"].numpy()
            data[f"{name}_histogram_raw"] = out["histogram_raw"].numpy()
            data[f"{name}_noise_level"] = out["noise_level"].numpy().reshape(1)
            entry["label"] = int(out["cond_inputs"][1]) if len(out["cond_inputs"]) > 1 else None
            assert out["image"].dtype == torch.float32 and out["cond_inputs"][0].dtype == torch.float32
            # the reference's own raw block statistics of the same window, and the float64 means
            li, lj = twin.inverse_offsets(i, j, crop, crop, t, S)
            raw, _ = raw_ds._get_cond_image(tree, path, li, lj, crop, crop, t // 4 == 1, t % 4)
            raw = raw.numpy()
            V = crop + 64
            lo = twin.view(twin.window(tree[path]["lowres_exact"].array, li - 32, lj - 32, V, V), t)
            cl = twin.view(twin.window(tree[path]["climate"].array[list(twin.CLIMATE_CHANNELS)], li - 32, lj - 32, V, V), t)
            m64 = np.concatenate([exact_block_means(lo)[None], exact_block_means(cl)])
            assert np.array_equal(np.isnan(m64), np.isnan(raw[[0, 2, 3, 4, 5]])), name
            assert not twin.zero_ties(lo), name
            if "u_drop" in got:
                u = got["u_drop"].numpy()
                p = F(cfg["cond_input_dropout"])
                assert ((np.abs(u - p) > np.spacing(p)) | (u == p)).all() and ((u == p).all() if "u_drop_on_threshold" in (force or []) else (u != p).all()), name
            data[f"{name}_raw"], data[f"{name}_m64"] = raw, m64
            data[f"{name}_eref"] = np.abs(raw[[0, 2, 3, 4, 5]].astype(np.float64) - m64)
            entry["nan_centres"] = int(got["z_replace"].numel()) if "z_replace" in got else 0
        elif cls == "decoder":
            for key in ("image", "cond_img", "lowfreq", "lowfreq_padded"):
                data[f"{name}_{key}"] = out[key].numpy()
            assert out["cond_img"].dtype == torch.float16 and out["image"].dtype == torch.float32
            entry["label"] = int(out["cond_inputs"][0]) if out["cond_inputs"] else None
        else:
            data[f"{name}_image"] = out["image"].numpy()
            entry["label"] = int(out["cond_inputs"][0]) if "cond_inputs" in out else None
        items.append(entry)
        return entry

    with Recorder(torch) as rec:
        for run, (cfg_name, seed, count) in RUNS.items():
            ds = build(cfg_name)
            key_lists[cfg_name] = json.loads(json.dumps(ds.keys))
            ds.set_seed(seed)
            names = []
            for n in range(count):
                # the first item of the longest run carries its whole image and noise
                names.append(record(rec, ds, f"{run}_{n}", cfg_name, None, full=(run == "runLA" and n == 0))["name"])
            runs[run] = {"config": cfg_name, "seed": seed, "items": names}
        for cfg_name, seed, force, full in FORCED:
            ds = build(cfg_name)
            ds.set_seed(seed)
            record(rec, ds, f"f{seed}", cfg_name, force, full)

    for cls, seen in seen_t.items():
        assert seen == set(range(8)), (cls, seen)
    la = [e for e in items if e["name"].startswith("runLA_")]
    assert len(la) >= 12 and any(e["nan_centres"] for e in la) and any(not e["nan_centres"] for e in la), [e["nan_centres"] for e in la]

    data["cases"] = np.array(json.dumps({"configs": {k: {"cls": c, "args": a} for k, (c, a) in CONFIGS.items()}, "items": items, "runs": runs,
                                         "tree_crc": twin.tree_crc(), "keys": key_lists}))
    data["versions"] = np.array(json.dumps({"numpy": np.__version__, "torch": torch.__version__}))
    # a fixed member order and timestamp: regenerating gives the same bytes
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(data):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(data[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; {len(items)} items")
    for e in items:
        if e["cls"] == "latents":
            print(f"  {e['name']:10s} {e['config']} {e['path']:10s} i {e['i']:3d} j {e['j']:3d} t {e['t']} nan centres {e['nan_centres']} "
                  f"max e_ref {np.nanmax(data[e['name'] + '_eref'][0]):.3e}")


if __name__ == "__main__":
    main()
