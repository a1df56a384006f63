"""Device time of the autoencoder (terrain_diffusion_amd.EDMAutoencoder, the released autoencoder_x8 config on synthetic weights) beside a
yardstick of the same process: a batch-8 512 x 512 forward of the decoder U-Net, whose 64-channel 512 x 512 level is the closest existing
workload.  Prints one JSON line per measurement.

    python tools/autoencoder_bench.py [--reps 10] [--warmup 2] [--rounds 3] [--dtypes bf16 fp16] [--size 512]

Method (that of tools/rivers_bench.py): the mean of --reps back-to-back calls between two events on the engine's stream, inputs on the device
before the window opens; the median of --rounds rounds with their min .. max, the legs of one dtype alternating.  The autoencoder calls are
enqueue-only (option "async"); EDMUnet2D's forward ends with a stream synchronisation of its own, which its figure therefore includes.
  encode_dihedral   one 1 x size x size chunk -> the 8 dihedral views -> preencode -> fp16 latent stack (batch 8 at size^2)
  decode            8 latents 4 x size/8 x size/8 -> 8 x 1 x size x size
  unet_decoder_b8   the yardstick
After the timing, one call of each autoencoder leg runs with option "profile" = 1: the per-kernel event times, split into convs, the other
kernels of the graph and the kernels of ae_kernels.hip, each as a share of their sum.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp16"])
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    import torch
    import _ae_twin as T
    import terrain_diffusion_amd as td
    from oracle import rng
    from oracle.unet import DECODER_CONFIG, synth_state_dict
    from terrain_diffusion_amd._lib import lib
    from terrain_diffusion_amd.engine import get_engine
    assert torch.cuda.is_available(), "autoencoder_bench measures on the GPU; there is no CPU fallback"
    eng = get_engine("cuda")
    dev = torch.device("cuda", eng.device_id)
    S = args.size
    common = dict(tool="autoencoder_bench", size=S, reps=args.reps, rounds=args.rounds, device=torch.cuda.get_device_name(dev),
                  build_id=lib().td_build_id().decode(), method="mean of back-to-back calls between two stream events; median of rounds")
    chunk = torch.from_numpy(rng.standard_normal(1, (1, S, S))).to(dev)
    z = torch.from_numpy(rng.standard_normal(2, (8, 4, S // 8, S // 8))).to(dev)
    xu = torch.from_numpy(rng.standard_normal(3, (8, 5, S, S))).to(dev)
    tu = torch.full((8,), 0.8)
    ae_sd = T.synth_ae_state_dict(T.RELEASED, seed=78)
    un_sd = synth_state_dict(DECODER_CONFIG, seed=5)
    for dtype in args.dtypes:
        ae = td.EDMAutoencoder(**T.RELEASED, dtype=dtype).load_state_dict(ae_sd)
        un = td.EDMUnet2D(**DECODER_CONFIG, dtype=dtype).load_state_dict(un_sd)
        legs = {"encode_dihedral": lambda: ae.encode_dihedral(chunk), "decode": lambda: ae.decode(z), "unet_decoder_b8": lambda: un(xu, tu, [])}
        with eng.on_stream(torch.cuda.Stream(), asynchronous=True):
            st = torch.cuda.current_stream()

            def timed(fn):
                for _ in range(args.warmup):
                    fn()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                for _ in range(args.reps):
                    fn()
                b.record(st)
                b.synchronize()
                return a.elapsed_time(b) / args.reps
            ms = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    ms[k].append(timed(fn))
        for k, v in ms.items():
            med = statistics.median(v)
            line = dict(common, what=k, dtype=dtype, device_ms=round(med, 4), device_ms_min=round(min(v), 4), device_ms_max=round(max(v), 4))
            if k != "unet_decoder_b8":
                line["chunks_per_s"] = round(1e3 / med, 2)
            print(json.dumps(line), flush=True)
        # the profile option's split, one eager call per leg (events around every kernel; not part of the timing above)
        eng.set_option("profile", 1)
        try:
            for k in ("encode_dihedral", "decode"):
                eng.profile_read(reset=True)
                legs[k]()
                eng.synchronize()
                ops = eng.profile_ops()
                conv_ms, conv_n, other_ms, other_n = eng.profile_read(reset=True)
                ae_ops = {lab: round(t, 4) for lab, t, _n in ops if lab.startswith("ae_")}
                tot = conv_ms + other_ms
                print(json.dumps(dict(common, what=k + "_profile", dtype=dtype, conv_ms=round(conv_ms, 4), conv_launches=conv_n, other_ms=round(other_ms, 4),
                                      other_launches=other_n, ae_kernels_ms=ae_ops, ae_kernels_share=round(sum(ae_ops.values()) / tot, 4) if tot else None)), flush=True)
        finally:
            eng.set_option("profile", 0)
        ae.close()
        un.close()


if __name__ == "__main__":
    main()
