"""Generates tests/golden/explorer.npz by RUNNING THE REFERENCE'S OWN explorer routes (terrain_diffusion/inference/explorer/server.py, through
Flask's app.test_client()) and its sampler's sample_land_tiles / get_coarse_climate_info (inference/random_sampler.py) on a stub world.

Needs a checkout of the reference and the torch, flask, click, matplotlib, scipy and PIL its modules import; the fixture does not.  The three
modules (relief_map, explorer/server, random_sampler) are loaded by path; terrain_diffusion.inference.world_pipeline and
terrain_diffusion.common.cli_helpers are replaced by stub modules (names only, plus normalize_tensor's one-line definition as the sampler
uses it: numerator planes over the last plane).  The stub world is deterministic in the absolute index and logs every block it hands out.
Only inputs, outputs and library versions are stored, never source text:

    python tests/golden/make_explorer_golden.py --reference PATH_TO_REFERENCE_CHECKOUT      (or TD_REFERENCE=PATH)

Index (json in "cases"): coarse cases {"name", "kind", "box" [ci0, ci1, cj0, cj1], "views" [{"key", "channel", "filters" {ch: [lo, hi]}}]},
detail cases {"name", "kind", "args" {ci, cj, detail_size, pan_i, pan_j}, "native_resolution", "modes", "has_climate"}, land cases {"name",
"window", "detail_size", "min_land_frac", "n_samples"}, info cases {"name", "ci", "cj"}.  Arrays: coarse_<case> (7, H, W) the block every
request of the case read; img_<key> decoded RGBA; hdr_<key> json; stats_<case> / data_<case> the json bodies as bytes (no data_default); elev_<case> / climate_<case> the
world.get window; png_<case>_<mode>; raw_<case> bytes + rawhdr_<case> (the two 64 x 64 cases); land_coarse the sampler's block; full_<name> / picks_<name> (n, 2);
info_<name> (4,) float64; lut_viridis / lut_terrain / lut_RdBu_r (256, 3) fp32.
"""
import argparse
import importlib.util
import io
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _explorer_twin as twin  # noqa: E402

OUT = os.path.join(HERE, "explorer.npz")
F = np.float32
SEED = 1234
NAN_COARSE = [(0, 0), (3, 36), (40, 0), (17, 20), (18, 20)]   # offsets inside the "nan" coarse region
NAN_DETAIL = [(0, 0), (5, 90), (95, 95), (40, 41), (40, 42)]


def coarse_fields(kind, ii, jj):
    """(7, H, W) fp32 weighted sums at absolute coarse rows ii, columns jj: six channels times a weight plane, the weight plane last."""
    fi, fj = ii.astype(np.float64), jj.astype(np.float64)
    a = np.sin(0.131 * fi + 0.217 * fj) + 0.6 * np.cos(0.093 * fi - 0.171 * fj)
    b = np.sin(0.071 * fi - 0.113 * fj + 1.0)
    if kind == "const":
        a, b = np.full_like(fi, 0.25), np.full_like(fi, -0.5)
    if kind == "land":
        # rows above 0: 7 land cells in every 10 consecutive columns (each 10 x 10 window holds exactly 70); below: a hashed ~55 % land
        h = (((ii * 73856093) ^ (jj * 19349663)) & 0xFFFF) / 65536.0
        land = np.where(ii < 0, np.mod(ii * 7 + jj * 3, 10) < 7, h < 0.55)
        a = np.where(land, 0.2 + np.abs(a), -0.2 - np.abs(a))
    vals = np.stack([38.0 * a, 30.0 * a - 6.0, 11.0 + 17.0 * b, 600.0 + 450.0 * a * b, 900.0 * (a + 0.4), 55.0 + 40.0 * b])
    w = 1.0 + 0.45 * np.sin(0.31 * fi + 0.23 * fj) if kind != "const" else np.full_like(fi, 1.5)
    return np.concatenate([vals * w, w[None]]).astype(F)


class Coarse:
    def __init__(self, world):
        self.world = world

    def __getitem__(self, idx):
        import torch
        ch, si, sj = idx
        assert ch == slice(None)
        ii, jj = np.meshgrid(np.arange(si.start, si.stop), np.arange(sj.start, sj.stop), indexing="ij")
        block = coarse_fields(self.world.kind, ii, jj)
        if self.world.kind == "nan":
            for (a, b) in NAN_COARSE:
                if a < block.shape[1] and b < block.shape[2]:
                    block[:, a, b] = np.nan
            block[2, 7, 7] = np.nan      # one channel only
        self.world.coarse_log.append(((si.start, si.stop, sj.start, sj.stop), block))
        return torch.from_numpy(block.copy())


def detail_fields(kind, ii, jj):
    fi, fj = ii.astype(np.float64), jj.astype(np.float64)
    e = 900.0 * np.sin(fi / 23.0) * np.cos(fj / 31.0) + 500.0 * np.sin((fi + 2 * fj) / 17.0) + 150.0
    if kind == "ocean":
        e = -np.abs(e) - 25.0
    if kind == "raw":
        e = e * 40.0   # beyond the int16 range on both sides
    clim = np.stack([14.0 + 12.0 * np.sin(fi / 41.0) + 5.0 * np.cos(fj / 29.0), 700 + 300 * np.sin(fj / 37.0), 900 + 500 * np.cos(fi / 19.0),
                     50 + 30 * np.sin(fi / 13.0 + fj / 11.0), 0.0065 + 0 * fi]).astype(F)
    return e.astype(F), clim


class StubWorld:
    seed = 4242

    def __init__(self, kind, native_resolution=90.0, climate=True):
        self.kind, self.native_resolution, self.climate = kind, native_resolution, climate
        self.coarse, self.coarse_log, self.get_log = Coarse(self), [], []

    def get(self, i1, j1, i2, j2, with_climate=True):
        import torch
        ii, jj = np.meshgrid(np.arange(i1, i2), np.arange(j1, j2), indexing="ij")
        elev, clim = detail_fields(self.kind, ii, jj)
        if self.kind == "nan":
            for (a, b) in NAN_DETAIL:
                elev[a, b] = np.nan
        if self.kind == "raw":
            elev[0, :8] = [32768.7, -32768.7, 32767.0, -32768.0, -0.25, -1.0, 7.0, 0.999]
            elev[1, :4] = [32767.5, -32769.0, -3.75, 40000.0]
        clim = clim if (with_climate and self.climate) else None
        self.get_log.append(((int(i1), int(j1), int(i2), int(j2)), elev, clim))
        return {"elev": torch.from_numpy(elev.copy()), "climate": None if clim is None else torch.from_numpy(clim.copy())}


def install_stubs(reference):
    wp = types.ModuleType("terrain_diffusion.inference.world_pipeline")
    wp.WorldPipeline = StubWorld
    wp.resolve_hdf5_path = lambda p: p
    wp.normalize_tensor = lambda tensor, dim=0: tensor[:-1] / tensor[-1:]   # world_pipeline.normalize_tensor for dim = 0
    cli = types.ModuleType("terrain_diffusion.common.cli_helpers")
    cli.parse_kwargs = lambda kw: {}
    cli.parse_cache_size = lambda s: s
    for name in ("terrain_diffusion", "terrain_diffusion.inference", "terrain_diffusion.common"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["terrain_diffusion.inference.world_pipeline"] = wp
    sys.modules["terrain_diffusion.common.cli_helpers"] = cli
    sys.modules["terrain_diffusion.inference.relief_map"] = load(reference, "relief_map", "terrain_diffusion.inference.relief_map")


def load(reference, rel, name=None):
    path = os.path.join(reference, "terrain_diffusion", "inference", *rel.split("/")) + ".py"
    spec = importlib.util.spec_from_file_location(name or "reference_" + rel.replace("/", "_"), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def coarse_cases():
    six = [{"key": f"odd_ch{c}", "channel": c, "filters": {}} for c in range(6)]
    filt = [("f_none", {}), ("f_one", {2: [9.0, None]}), ("f_both", {0: [-200.0, 1500.0], 3: [300.0, 900.0], 5: [None, 70.0]}),
            ("f_all", {4: [1e9, None]}), ("f_p5_ignored", {1: [1e9, None]})]
    return [
        ("odd", "plain", (-20, 21, 5, 42), six + [{"key": f"odd_{n}", "channel": 4, "filters": f} for n, f in filt]),
        ("nan", "nan", (-7, 34, -30, 7), [{"key": f"nan_ch{c}", "channel": c, "filters": {}} for c in (0, 2, 4)]
         + [{"key": "nan_filtered", "channel": 2, "filters": {2: [0.0, None]}}]),
        ("one", "plain", (3, 4, -9, -8), [{"key": f"one_ch{c}", "channel": c, "filters": {}} for c in (0, 4)]),
        ("const", "const", (0, 9, 0, 11), [{"key": f"const_ch{c}", "channel": c, "filters": {}} for c in (0, 3, 4)]),
        ("default", "plain", (-50, 50, -50, 50), [{"key": "default_ch0", "channel": 0, "filters": {}},
                                                   {"key": "default_ch4", "channel": 4, "filters": {0: [0.0, None], 2: [None, 20.0]}}]),
    ]


def detail_cases():
    a96 = {"ci": 1, "cj": -2, "detail_size": 96, "pan_i": 7, "pan_j": -13}
    modes = ["elevation", "temperature", "relief"]
    return [("clim", "plain", a96, 90.0, True, modes), ("noclim", "plain", a96, 90.0, False, modes),
            ("nan", "nan", {"ci": 0, "cj": 0, "detail_size": 96, "pan_i": 48, "pan_j": 48}, 90.0, True, ["elevation"]),
            ("ocean", "ocean", a96, 30.0, True, modes),
            ("raw", "raw", {"ci": 0, "cj": 0, "detail_size": 64, "pan_i": 32, "pan_j": 32}, 90.0, True, []),
            ("raw_noclim", "raw", {"ci": 0, "cj": 0, "detail_size": 64, "pan_i": 32, "pan_j": 32}, 90.0, False, [])]


def land_cases():
    c = []
    for ds in (256, 512, 768, 1024, 2560):
        for frac in (0.0, 0.5, 1.0, 0.7):
            c.append((f"d{ds}_f{str(frac).replace('.', '')}", 12, ds, frac, 10))
    return c


def query(view, box):
    q = {"channel": view["channel"], "ci0": box[0], "ci1": box[1], "cj0": box[2], "cj1": box[3]}
    for ch, (lo, hi) in view["filters"].items():
        if lo is not None:
            q[f"ch{ch}_min"] = repr(float(lo))
        if hi is not None:
            q[f"ch{ch}_max"] = repr(float(hi))
    return q


def decode(png):
    from PIL import Image
    img = np.array(Image.open(io.BytesIO(png)))
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 4
    return img


def same_block(log, box):
    blocks = [b for k, b in log if k == tuple(box)]
    assert blocks and all(np.array_equal(b, blocks[0], equal_nan=True) for b in blocks)
    return blocks[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"), help="root of a terrain-diffusion checkout")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set TD_REFERENCE")
    import warnings
    import matplotlib
    import torch
    warnings.simplefilter("ignore", RuntimeWarning)
    install_stubs(args.reference)
    server = load(args.reference, "explorer/server")
    sampler = load(args.reference, "random_sampler")
    import matplotlib.pyplot as plt
    client = server.app.test_client()
    data, index = {}, {"coarse": [], "detail": [], "land": [], "info": []}
    luts = {n: plt.get_cmap(n)(np.arange(256))[:, :3].astype(F) for n in ("viridis", "terrain", "RdBu_r")}
    for n, lut in luts.items():
        data["lut_" + n] = lut

    for name, kind, box, views in coarse_cases():
        world = StubWorld(kind)
        server._PIPELINE = world
        for v in views:
            r = client.get("/api/coarse.png", query_string=query(v, box))
            assert r.status_code == 200, (v, r.get_data()[:300])
            data["img_" + v["key"]] = decode(r.get_data())
            data["hdr_" + v["key"]] = np.array(json.dumps({k: r.headers[k] for k in ("X-Vmin", "X-Vmax")}))
        q = {"ci0": box[0], "ci1": box[1], "cj0": box[2], "cj1": box[3]}
        for route, key in (("/api/coarse_stats", "stats_"), ("/api/coarse_data.json", "data_")):
            r = client.get(route, query_string=q)
            assert r.status_code == 200, r.get_data()[:300]
            if key == "data_" and name == "default":
                continue   # 60 000 numbers of text: the smaller regions cover the route
            data[key + name] = np.frombuffer(r.get_data(), np.uint8).copy()
        block = same_block(world.coarse_log, box)
        data["coarse_" + name] = block
        # the channel-4 (log1p) views: the share of pixels within 4 ulp of a table boundary stays under the tests' cap for the reference
        # alone, and the rounded headers do not move when the range moves by 2 ulp
        for v in views:
            if v["channel"] == 4:
                _, hdr, margin = twin.coarse_image(block, 4, luts["viridis"], {int(k): tuple(b) for k, b in v["filters"].items()})
                assert (margin <= 4).sum() <= 1e-3 * margin.size, (v["key"], int((margin <= 4).sum()))
                d = twin.display(twin.channels(block)[4], True)
                for val in twin.view_range(d):
                    for k in (-2, 2):
                        moved = float(F(val) + k * np.spacing(F(val))) if np.isfinite(val) else val
                        assert round(moved, 3) == round(val, 3) or not np.isfinite(val), (v["key"], val)
        index["coarse"].append({"name": name, "kind": kind, "box": list(box), "views": views})

    for name, kind, a, nr, has_climate, modes in detail_cases():
        world = StubWorld(kind, nr, has_climate)
        server._PIPELINE = world
        for mode in modes:
            r = client.get("/api/detail.png", query_string={**a, "mode": mode})
            assert r.status_code == 200, (name, mode, r.get_data()[:300])
            data[f"png_{name}_{mode}"] = decode(r.get_data())
        if kind == "raw":
            r = client.get("/api/detail_raw", query_string=a)
            assert r.status_code == 200
            data["raw_" + name] = np.frombuffer(r.get_data(), np.uint8).copy()
            data["rawhdr_" + name] = np.array(json.dumps({k: r.headers[k] for k in ("X-Height", "X-Width", "X-Has-Temp")}))
        boxes = {k for k, _, _ in world.get_log}
        assert len(boxes) == 1
        _, elev, clim = world.get_log[0]
        data["elev_" + name] = elev
        if clim is not None:
            data["climate_" + name] = clim
        index["detail"].append({"name": name, "kind": kind, "args": a, "native_resolution": nr, "modes": modes, "has_climate": has_climate,
                                "box": list(world.get_log[0][0])})

    world = StubWorld("land")
    for name, window, ds, frac, n in land_cases():
        random.seed(SEED)
        picks = sampler.sample_land_tiles(world, window, ds, frac, n)
        random.seed(SEED)
        full = sampler.sample_land_tiles(world, window, ds, frac, 10 ** 9)     # more than exist: the whole list, in order
        data["picks_" + name] = np.array(picks, np.int64).reshape(-1, 2)
        data["full_" + name] = np.array(full, np.int64).reshape(-1, 2)
        index["land"].append({"name": name, "window": window, "detail_size": ds, "min_land_frac": frac, "n_samples": n})
    block = same_block(world.coarse_log, (-12, 12, -12, 12))
    data["land_coarse"] = block
    # at least one half = 5 window holds exactly 70 land cells, and the reference leaves that position out at 0.7
    land = twin.channels(block, eps=0.0)[0] > 0
    seventy = [(i, j) for i in range(5, 19) for j in range(5, 19) if land[i - 5:i + 5, j - 5:j + 5].sum() == 70]
    assert seventy
    full07 = {tuple(t) for t in data["full_d2560_f07"].tolist()}
    assert all((i - 12, j - 12) not in full07 for i, j in seventy)
    assert len(full07) > 0 and len(data["full_d256_f00"]) == 0
    for name, ci, cj in (("a", 3, -4), ("b", -11, 7)):
        info = sampler.get_coarse_climate_info(world, ci, cj)
        data["info_" + name] = np.array([info[k] for k in ("temp", "temp_std", "precip", "precip_cv")], np.float64)
        data["info_coarse_" + name] = same_block(world.coarse_log, (ci, ci + 1, cj, cj + 1))
        index["info"].append({"name": name, "ci": ci, "cj": cj})

    data["cases"] = np.array(json.dumps(index))
    data["seed"] = np.array(SEED)
    data["versions"] = np.array(json.dumps({"torch": torch.__version__, "numpy": np.__version__, "matplotlib": matplotlib.__version__}))
    # a fixed member order and timestamp: regenerating gives the same bytes
    import zipfile
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(data):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(data[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; {len(index['coarse'])} coarse, {len(index['detail'])} detail, {len(index['land'])} land cases")


if __name__ == "__main__":
    main()
