"""Generates tests/golden/mc.npz by RUNNING THE REFERENCE'S OWN minecraft_api.py (_get_upsampled, _classify_biome, _binary_response) and
api.py (_get_terrain), from terrain_diffusion/inference/.

Needs a checkout of the reference and the torch, flask and click its modules import; the fixture does not.  Both modules are loaded by path.
Three of their imports are replaced by stub modules in sys.modules:
  * pyfastnoiselite.pyfastnoiselite: FastNoiseLite.gen_from_coords returns this package's own FBm noise (tests/_mc_twin.py) for the
    generator's seed, frequency, octaves and gain -- pyfastnoiselite itself is not needed;
  * terrain_diffusion.inference.world_pipeline and terrain_diffusion.common.cli_helpers: names only (the requests below pass a stub world).
The reference's classifier and noise step squeeze their Sobel output, so a box one pixel wide (W = 1, H > 1) gets a wrongly broadcast
(H, H) result there; that shape is recorded through api.py only.  The stub world returns deterministic, crop-consistent fields of the absolute
native pixel (a 6 x 6 pattern of 8 x 8-pixel climate cells, each with a ramp of its own steepness) and logs every window it hands out.  Only inputs, outputs and the torch version are stored, never source
text:

    python tests/golden/make_mc_golden.py --reference PATH_TO_REFERENCE_CHECKOUT      (or TD_REFERENCE=PATH)

Each case is {"name", "fn" (mc | api), "box" [i1, j1, i2, j2], "scale", "noise", "kind", "native_resolution", "gets" [[i1, j1, i2, j2,
with_climate], ...]}.  Arrays, for case <n>: win<k>_elev_<n> / win<k>_climate_<n> (the k-th window world.get returned; climate absent when
None), noise_<n> (7, H, W) in the reference's generator order; mc: elev_, elev_smooth_, climate_, elev_padded_ (scale > 1), biome_ (int16),
payload_ (uint8 bytes); api: elev_, climate_.
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _mc_twin as twin  # noqa: E402

OUT = os.path.join(HERE, "mc.npz")
CELL = 8
# one row per climate cell: (elevation base m, ramp m per native pixel along j, temp C, t_season, precip mm, p_cv %) -- aimed at every id
CELLS = [
    (-200, 2, -10, 300, 300, 20), (-300, 2, 0, 300, 300, 20), (-100, 2, 24, 300, 800, 20), (-50, 2, 12, 300, 600, 20),
    (3000, 66.6, -3, 2000, 200, 100), (3000, 117, 10, 500, 300, 20), (3000, 5, -10, 300, 300, 20), (3000, 5, -2, 1500, 300, 20),
    (3000, 5, -2, 1500, 500, 20), (3000, 5, -10, 300, 100, 20), (3000, 5, 10, 500, 100, 20), (3000, 5, 3, 172, 500, 10),
    (3000, 5, 8, 500, 400, 20), (3000, 5, 8, 500, 1000, 20), (500, 5, -10, 300, 300, 20), (500, 5, -2, 1500, 300, 20),
    (500, 5, -2, 1500, 500, 20), (300, 5, 28, 300, 10, 20), (800, 5, -3, 100, 100, 20), (500, 5, 3, 172, 500, 10),
    (300, 5, 28, 300, 1000, 20), (300, 5, 22, 300, 600, 50), (300, 5, 15, 300, 700, 20), (50, 2, 22, 300, 1500, 20),
    (300, 5, 15, 300, 1000, 20), (300, 5, 8, 500, 600, 20), (300, 117, 15, 300, 300, 20), (800, 66.6, -3, 2000, 200, 100),
    (300, 5, 8, 500, 400, 20), (300, 5, 22, 300, 3000, 20), (50, 2, 15, 300, 3000, 20), (500, 5, 8, 500, 2000, 20),
    (500, 5, 15, 300, 2500, 20), (300, 58.5, 15, 300, 1000, 20), (300, 5, 30, 300, 1500, 20), (-500, 2, 28, 300, 500, 20),
]
NAN_PIXELS = [(3, 4), (17, 30), (-2, -5), (20, 9)]


def fields(kind, ii, jj):
    """(elev (H, W), climate (5, H, W) or None) fp32 at absolute native rows ii, columns jj."""
    t = CELLS_ARR[(np.mod(ii // CELL, 6) * 6 + np.mod(jj // CELL, 6))]
    fi, fj = ii.astype(np.float64), jj.astype(np.float64)
    wave = np.sin(0.23 * fi + 0.41 * fj) + 0.5 * np.cos(0.37 * fi - 0.19 * fj)
    elev = t[..., 0] + t[..., 1] * (np.mod(jj, CELL) - 3.5) + 3.0 * wave
    if kind == "ocean":
        elev = -np.abs(elev) - 40.0
    clim = np.stack([t[..., 2] + 0.6 * wave, t[..., 3] * (1.0 + 0.05 * wave), t[..., 4] * (1.0 + 0.04 * wave), t[..., 5] + 2.0 * wave,
                     0.0065 + 0.001 * wave]).astype(np.float32)
    elev = elev.astype(np.float32)
    if kind == "nan":
        for (a, b) in NAN_PIXELS:
            elev[(ii == a) & (jj == b)] = np.nan
    if kind == "noclim":
        return elev, None
    if kind == "clim3":
        return elev, clim[:3].copy()
    return elev, clim


CELLS_ARR = np.array(CELLS, np.float64)


class StubWorld:
    def __init__(self, kind, native_resolution):
        self.kind, self.native_resolution, self.log = kind, native_resolution, []

    def get(self, i1, j1, i2, j2, with_climate=True):
        import torch
        ii, jj = np.meshgrid(np.arange(i1, i2), np.arange(j1, j2), indexing="ij")
        elev, clim = fields(self.kind, ii, jj)
        clim = clim if with_climate else None
        self.log.append(([int(i1), int(j1), int(i2), int(j2), bool(with_climate)], elev, clim))
        return {"elev": torch.from_numpy(elev.copy()), "climate": None if clim is None else torch.from_numpy(clim.copy())}


class StubNoise:
    calls = []

    def __init__(self, seed=1337):
        self.seed, self.frequency, self.fractal_octaves, self.fractal_gain, self.fractal_lacunarity = seed, 0.01, 3, 0.5, 2.0

    def gen_from_coords(self, coords):
        assert self.fractal_lacunarity == 2.0
        v = twin.fbm(self.seed, self.frequency, self.fractal_octaves, self.fractal_gain, coords)
        StubNoise.calls.append(((self.seed, self.frequency, self.fractal_octaves, self.fractal_gain), v))
        return v


def install_stubs():
    ns = types.SimpleNamespace
    fnl = types.ModuleType("pyfastnoiselite.pyfastnoiselite")
    fnl.FastNoiseLite = StubNoise
    fnl.NoiseType = ns(NoiseType_Perlin="perlin")
    fnl.FractalType = ns(FractalType_FBm="fbm")
    wp = types.ModuleType("terrain_diffusion.inference.world_pipeline")
    wp.WorldPipeline = StubWorld
    wp.resolve_hdf5_path = lambda p: p
    cli = types.ModuleType("terrain_diffusion.common.cli_helpers")
    cli.parse_kwargs = lambda kw: {}
    cli.parse_cache_size = lambda s: s
    for name in ("pyfastnoiselite", "terrain_diffusion", "terrain_diffusion.inference", "terrain_diffusion.common"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["pyfastnoiselite.pyfastnoiselite"] = fnl
    sys.modules["terrain_diffusion.inference.world_pipeline"] = wp
    sys.modules["terrain_diffusion.common.cli_helpers"] = cli


def load(reference, name):
    path = os.path.join(reference, "terrain_diffusion", "inference", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    c = [("x1_cover", "mc", (0, 0, 48, 48), 1, 1.0, "plain", 90.0), ("x1_neg", "mc", (-13, -7, 5, 9), 1, 1.0, "plain", 90.0)]
    for s, box in ((2, (-6, 10, 20, 34)), (4, (37, -23, 61, 5)), (8, (-45, 77, -21, 101))):
        for n in (0.0, 1.0, 2.5):
            c.append((f"x{s}_n{str(n).replace('.', '')}", "mc", box, s, n, "plain", 90.0))
    c += [("x8_cells", "mc", (120, 250, 152, 278), 8, 1.0, "plain", 90.0), ("x4_cliffs", "mc", (130, 120, 158, 148), 4, 1.0, "plain", 90.0),
          ("x3_odd", "mc", (5, -4, 21, 12), 3, 1.0, "plain", 90.0),
          ("t1x9", "mc", (3, 5, 4, 14), 4, 1.0, "plain", 90.0), ("t9x1", "api", (3, 5, 12, 6), 2, 0.0, "plain", 90.0),
          ("t7x5", "mc", (-3, -2, 4, 3), 8, 1.0, "plain", 90.0), ("t7x5_x1", "mc", (-3, -2, 4, 3), 1, 1.0, "plain", 90.0),
          ("clim_none", "mc", (9, 9, 25, 29), 4, 1.0, "noclim", 90.0), ("clim3", "mc", (9, 9, 25, 29), 2, 1.0, "clim3", 90.0),
          ("clim3_x1", "mc", (9, 9, 25, 29), 1, 1.0, "clim3", 90.0),
          ("ocean", "mc", (-20, 30, 4, 58), 4, 1.0, "ocean", 90.0), ("nan_x1", "mc", (0, -8, 24, 36), 1, 1.0, "nan", 90.0),
          ("nan_x2", "mc", (0, -12, 44, 24), 2, 1.0, "nan", 90.0), ("nr30", "mc", (-11, 13, 13, 41), 2, 1.0, "plain", 30.0),
          ("api_x1", "api", (-5, 3, 17, 23), 1, 0.0, "plain", 90.0), ("api_x2", "api", (-5, 3, 17, 23), 2, 0.0, "plain", 90.0),
          ("api_x3", "api", (-7, 2, 10, 22), 3, 0.0, "plain", 90.0), ("api_x8", "api", (-30, 41, -9, 66), 8, 0.0, "plain", 90.0),
          ("api_noclim", "api", (4, 4, 20, 12), 4, 0.0, "noclim", 90.0)]
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"), help="root of a terrain-diffusion checkout")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set TD_REFERENCE")
    import torch
    install_stubs()
    mc = load(args.reference, "minecraft_api")
    api = load(args.reference, "api")
    data, index = {}, []
    for name, fn, (i1, j1, i2, j2), s, noise, kind, nr in cases():
        world = StubWorld(kind, nr)
        StubNoise.calls.clear()
        H, W = i2 - i1, j2 - j1
        planes = twin.noise_planes(i1, j1, H, W)
        if fn == "mc":
            if s == 1:
                pad = world.get(i1 - 1, j1 - 1, i2 + 1, j2 + 1, with_climate=False)
                out = world.get(i1, j1, i2, j2, with_climate=True)
                elev = out["elev"]
                biome = mc._classify_biome(elev, out.get("climate"), i1, j1, elev_padded=pad["elev"], pixel_size_m=nr)
            else:
                pix = nr / s
                up = mc._get_upsampled(world, i1, j1, i2, j2, scale=s, noise_scale=noise, pixel_size_m=pix)
                elev = up["elev"]
                biome = mc._classify_biome(up["elev_smooth"], up.get("climate"), i1, j1, elev_padded=up["elev_padded"], pixel_size_m=pix)
                data[f"elev_smooth_{name}"] = up["elev_smooth"].numpy().copy()
                data[f"elev_padded_{name}"] = up["elev_padded"].numpy().copy()
                if up["climate"] is not None:
                    data[f"climate_{name}"] = up["climate"].numpy().copy()
            resp = mc._binary_response(elev, biome=biome)
            assert resp.headers["X-Height"] == str(H) and resp.headers["X-Width"] == str(W) and resp.headers["X-Dtype"] == "int16-le"
            data[f"elev_{name}"] = elev.numpy().copy()
            data[f"biome_{name}"] = biome.numpy().copy()
            data[f"payload_{name}"] = np.frombuffer(resp.get_data(), np.uint8).copy()
            assert biome.dtype == torch.int16 and tuple(biome.shape) == (H, W)
        else:
            out = api._get_terrain(world, i1, j1, i2, j2, s)
            data[f"elev_{name}"] = out["elev"].numpy().copy()
            if out["climate"] is not None:
                data[f"climate_{name}"] = out["climate"].numpy().copy()
        # what the noise stub handed the reference is what the recorded planes hold
        for (seed, freq, octs, gain), v in StubNoise.calls:
            k = [g[1:] for g in twin.GENERATORS].index((seed, freq, octs, gain))
            if octs == 3 and seed == 12345:
                k = 0
            assert np.array_equal(v.reshape(H, W), planes[k]), name
        data[f"noise_{name}"] = planes
        for k, (_, e, c) in enumerate(world.log):
            data[f"win{k}_elev_{name}"] = e
            if c is not None:
                data[f"win{k}_climate_{name}"] = c
        index.append({"name": name, "fn": fn, "box": [i1, j1, i2, j2], "scale": s, "noise": noise, "kind": kind, "native_resolution": nr,
                      "gets": [g for g, _, _ in world.log]})
    data["cases"] = np.array(json.dumps(index))
    data["torch_version"] = np.array(torch.__version__)
    data["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(OUT, **data)
    ids = sorted({int(v) for k, a in data.items() if k.startswith("biome_") for v in np.unique(a)})
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(index)} cases, biome ids {ids}")


if __name__ == "__main__":
    main()
