"""Device time of the training-batch library (terrain_diffusion_amd.train_data, libtd_batch.so): one batch of 256 H5LatentsDataset items at crop
96 over resident 512 x 512 groups, per entry point, and the same items composed from plain torch operations on the GPU in the same process.
Prints one JSON line per measurement; every line carries the hash of the library's sources.

    python tools/train_data_bench.py [--items 256] [--crop 96] [--side 512] [--groups 4] [--reps 10] [--warmup 2] [--rounds 3]

Each measurement is --reps back-to-back enqueue-only calls between two events on the engine's stream (tables and draws are on the device before
the timing starts, so a host enqueue gap would be included), repeated --rounds times: the median per call with the least and the largest
round.  Beside each time stand the bytes per item the kernel must move as it is built, the GB/s that gives and its share of the HBM rate:
  views          8 c^2: the fp32 window in, the view out (c = crop);
  latents        48 c^2 for four latent channels: per element the two halves in (4), the fp32 noise in (4), the fp32 draw out (4);
  cond_image     20 (c + 64)^2: the haloed window of lowres_exact and of four climate planes in; the 7 g^2 outputs are nothing beside it;
  cond_vector    reads 7 g^2 and writes 58 values: launch-bound.
`get_batch` is the whole call with its host half -- the torch.Generator draws of 256 items and their upload -- timed by the host clock.
The yardstick `torch_compose` builds the same items with torch operations on the same resident planes (NaN-padded once, outside the timing):
slice, flip, rot90, block means, torch.quantile, the reparameterisation, the normalisation -- an item at a time, as the reference's loop does.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBPS = 8000.0           # the MI355X's HBM3E rate, 8 TB/s
COND_MEAN = [13.36, 10.03, 16.17, 612.99, 869.73, 71.64, 0.674]
COND_STD = [22.22, 22.13, 10.23, 453.81, 797.71, 34.23, 0.460]


class _Data:
    def __init__(self, array, **attrs):
        self.array, self.attrs, self.shape, self.dtype = array, attrs, array.shape, array.dtype

    def __getitem__(self, idx):
        return self.array[idx]


class _Group(dict):
    attrs = None


def make_tree(n_groups, side, seed=3):
    import numpy as np
    rng = np.random.default_rng(seed)
    chunks = _Group()
    for n in range(n_groups):
        f = lambda *s: rng.standard_normal(s, dtype=np.float32)
        g = _Group(latent=_Data(f(8, 8, side, side).astype(np.float16), pct_land=0.5, split="train"), lowfreq=_Data(f(side, side) * 30, pct_land=0.5),
                   lowres_exact=_Data(f(side, side) * 30), climate=_Data(f(15, side, side) * 10))
        g.attrs = {"beauty_score": 1.0 + n % 5}
        chunks[f"c{n}"] = _Group(s0=g)
    return _Group({"90": chunks})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--crop", type=int, default=96)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    from terrain_diffusion_amd import train_data as td
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "train_data_bench measures on the GPU; there is no CPU fallback"
    row = ge.BATCH_LIBS[0]
    sha = ge._sha16(ge.side_deps(row[0], row[1], row[3]))
    eng = get_engine("cuda")
    dev = torch.device("cuda", eng.device_id)
    N, crop, g = args.items, args.crop, (args.crop + 64) // 32
    ds = td.H5LatentsDataset(make_tree(args.groups, args.side), crop, [[0, 1]], [90], [1.0], latents_mean=[0.0] * 4, latents_std=[1.0] * 4, clip_edges=True,
                             beauty_dist=[True], cond_input_mean=COND_MEAN, cond_input_std=COND_STD, cond_input_dropout=0.2, cond_input_max_noise=0.1,
                             engine=eng)
    ds.set_seed(1)
    G = ds.groups
    G.table()                                               # the planes are resident before anything is timed

    with eng.on_stream(torch.cuda.Stream(), asynchronous=True):
        st = torch.cuda.current_stream()

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            rounds = []
            for _ in range(args.rounds):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                for _ in range(args.reps):
                    fn()
                b.record(st)
                b.synchronize()
                rounds.append(a.elapsed_time(b) / args.reps)
            rounds.sort()
            return rounds[len(rounds) // 2], rounds[0], rounds[-1]

        def emit(what, t, bytes_per_item=None, **line):
            ms, lo, hi = t
            if bytes_per_item is not None:
                gbps = bytes_per_item * N / (ms * 1e-3) / 1e9
                line.update(bytes_per_item=bytes_per_item, GBps=round(gbps, 1), hbm_share=round(gbps / HBM_GBPS, 4))
            print(json.dumps({"tool": "train_data_bench", "what": what, "source_sha16": sha, "items": N, "crop": crop, "side": args.side, "reps": args.reps,
                              "rounds": args.rounds, "device_ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), **line}), flush=True)

        plans = []
        for _ in range(N):
            p = ds.plan_item()
            p["z_replace"] = torch.randn(4, generator=ds.rng)
            plans.append(p)
        up = lambda k: torch.stack([p[k] for p in plans]).to(dev)
        items = ds._table(plans).to(dev)
        noise, hist, zr = up("noise"), up("histogram_raw"), up("z_replace")
        u_drop, u_noise, z_mean, z_p5 = up("u_drop")[:, 0].contiguous(), up("u_noise")[:, 0].contiguous(), up("z_mean")[:, 0].contiguous(), up("z_p5")[:, 0].contiguous()
        mean, std = torch.zeros(4, device=dev), torch.ones(4, device=dev)
        cm, cs = torch.tensor(COND_MEAN, device=dev), torch.tensor(COND_STD, device=dev)
        kw = dict(u_drop=u_drop, dropout=0.2, u_noise=u_noise, max_noise=0.1, z_mean=z_mean, z_p5=z_p5, mean=cm, std=cs)
        t = timed(lambda: td.views(G, items, "lowfreq", crop, affine=(td.LOWFREQ_MEAN, td.LOWFREQ_STD, 0.5)))
        emit("views", t, 8 * crop * crop)
        t = timed(lambda: td.sample_latents(G, items, noise, mode=0, mean=mean, std=std))
        emit("latents", t, 48 * crop * crop)
        t = timed(lambda: td.cond_image(G, items, crop, **kw))
        emit("cond_image", t, 20 * (crop + 64) ** 2, blocks=N * g * g)
        img = td.cond_image(G, items, crop, **kw)
        t = timed(lambda: td.cond_vector(img, hist, u_noise, zr, engine=eng))
        emit("cond_vector", t)

        def batch():
            td.views(G, items, "lowfreq", crop, affine=(td.LOWFREQ_MEAN, td.LOWFREQ_STD, 0.5))
            td.sample_latents(G, items, noise, mode=0, mean=mean, std=std)
            td.cond_vector(td.cond_image(G, items, crop, **kw), hist, u_noise, zr, engine=eng)
        emit("batch_device_half", timed(batch), 8 * crop * crop + 48 * crop * crop + 20 * (crop + 64) ** 2)

        # the yardstick: the same items from torch operations on the same planes
        pad = torch.nn.functional.pad
        padded = {}
        for path in G.index:
            lo, cl = G.plane(path, "lowres_exact"), G.plane(path, "climate")
            padded[path] = torch.cat([pad(lo[None], (32, 32, 32, 32), value=float("nan")), pad(cl, (32, 32, 32, 32), value=float("nan"))])
        f_mean, f_std = torch.tensor(td.LOWFREQ_MEAN, device=dev), torch.tensor(td.LOWFREQ_STD, device=dev)

        def torch_compose():
            images, conds = [], []
            for n, p in enumerate(plans):
                flip, k = p["t"] // 4 == 1, p["t"] % 4
                view = lambda x: torch.rot90(torch.flip(x, dims=[-1]) if flip else x, k, dims=[-2, -1])
                lat = G.plane(p["path"], "latent")[p["t"], :, p["i"]:p["i"] + crop, p["j"]:p["j"] + crop]
                sampled = (noise[n] * (lat[4:] * 0.5).exp() + lat[:4] - mean.view(-1, 1, 1)) / std.view(-1, 1, 1) * 0.5
                low = view(G.plane(p["path"], "lowfreq")[None, p["li"]:p["li"] + crop, p["lj"]:p["lj"] + crop])
                images.append(torch.cat([sampled, (low - f_mean) / f_std * 0.5]))
                blocks = view(padded[p["path"]][:, p["li"]:p["li"] + crop + 64, p["lj"]:p["lj"] + crop + 64]).reshape(5, g, 32, g, 32)
                means = blocks.mean(dim=(2, 4))
                p5 = torch.quantile(blocks[0].permute(0, 2, 1, 3).reshape(g * g, 1024), 0.05, dim=1).reshape(g, g)
                mask = (1 - torch.isnan(means[0]).float()) * (u_drop[n] > 0.2)
                s = u_noise[n] * 0.1
                m0 = torch.where(mask == 0, torch.nan, means[0]) + z_mean[n] * s
                q = torch.where(mask == 0, torch.nan, p5) + z_p5[n] * s
                stack = torch.cat([m0.nan_to_num(COND_MEAN[0])[None], q.nan_to_num(COND_MEAN[1])[None], means[1:], mask[None]])
                conds.append((stack - cm.view(-1, 1, 1)) / cs.view(-1, 1, 1))
            return torch.stack(images), torch.stack(conds)
        emit("torch_compose", timed(torch_compose))

    # the whole call, host half included, by the host clock
    walls = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds.get_batch(N)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    walls.sort()
    print(json.dumps({"tool": "train_data_bench", "what": "get_batch_wall", "source_sha16": sha, "items": N, "crop": crop, "side": args.side,
                      "rounds": args.rounds, "wall_ms": round(walls[len(walls) // 2], 3), "min_ms": round(walls[0], 3), "max_ms": round(walls[-1], 3)}), flush=True)


if __name__ == "__main__":
    main()
