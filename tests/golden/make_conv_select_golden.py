"""Generates tests/golden/conv_select.npz: the conv kernel / tile / split-K choices of the plan builder AS THE COMMIT BEFORE csrc/conv_select.h MADE
THEM (32b0b2a, where the choice was part of build_plan's `conv` lambda in csrc/engine.hip), recorded from that commit's own library on an MI355X.
tests/test_conv_select_cpu.py replays every row through conv_select() on the CPU.

    python tests/golden/make_conv_select_golden.py <checkout of 32b0b2a, instrumented and built> [out.npz]

The checkout's engine.hip gets these lines in front of `pl.ops.push_back(op);` at the end of the `conv` lambda (nothing else changes; without the
environment variable they do nothing).  They append two lines per conv op of every plan that is built: the inputs of the decision (tests/
conv_select_harness.cpp --fields, first two lists) and the decision in the columns of the harness's third list, then the label tag as run_unet prints it.
Fields the old encoding left over from a branch that was overridden later carry no meaning and are recorded as 0: glds_variant outside flavour 2
(and for its wide tile, which is a kernel of its own now), sb_mt / sb_nt outside flavour 4, sb_order outside flavours 4 and 5.

    if (const char* log_ = getenv("TD_CONV_SELECT_LOG")) {
        static const struct { const char* k; long long d; } ko[] = {{"batch_invariant", 0}, {"attn_mfma", 1}, {"bn128_min_wgs", 128}, {"glds", 1}, {"glds_bn", 0},
            {"glds_bn64", 1}, {"glds_dma1x1", 1}, {"glds_min_wgs", 8}, {"glds_round_aware", 1}, {"glds_small_max_groups", 6}, {"glds_splitk", 1},
            {"glds_splitk_from_groups", 2}, {"glds_splitk_max", 32}, {"glds_splitk_min_groups", 1}, {"glds_tiny", 0}, {"glds_variant", -1}, {"glds_wide", 1},
            {"glds_wide_min_wgs", 384}, {"glds_wide_tail", 1}, {"glds_wide_persist", 0}, {"glds_wide_mfma16", 1}, {"fewcout", 1}, {"producer_act", 1}, {"s16", 1},
            {"s16_min_wgs", 128}, {"sb", 1}, {"sb_m4", 0}, {"sb_max_glds_wgs", 1 << 30}, {"sb_mt", 0}, {"sb_nt", 0}, {"sb_order", -1}, {"sb_splitk", 1},
            {"sb_splitk_max", 16}, {"sb_splitk_wgs", 224}, {"sb_target_wgs", 160}, {"splitk", 1}, {"splitk_target_wgs", 512}, {"splitk_weighted", 1},
            {"walk_alternate", 1}};   // (each with the default of its read sites in that file)
        FILE* f = fopen(log_, "a");
        fprintf(f, "%d %d %d %d %d %d %d", N, h, w, cw.cout, cw.cout_pad, kgroups, p.nseg);
        for (int i = 0; i < 3; ++i) fprintf(f, " %d %d %d %d %d %d", p.seg[i].C, p.seg[i].taps, p.seg[i].xform, p.seg[i].resample, p.seg[i].Hs, p.seg[i].Ws);
        fprintf(f, " %d %d %d %d %d %d %d %d %d %d", chunk, u->dt, (int)u->bf16, cw.sb_n3, (int)out_f32, epi, res ? 1 : 0, clip > 0.f ? 1 : 0, u->eng->n_cus, (int)pl.ops.size());
        for (auto& o : ko) fprintf(f, " %lld", (long long)u->eng->option(o.k, o.d));
        const int fl = op.flavor; const bool wide = fl == 2 && op.glds_variant == 3, sbk = fl == 4 || fl == 5;
        fprintf(f, "\\n%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d ", fl == 2 ? (wide ? (op.wide16 ? 3 : 2) : 1) : fl, (int)op.narrow, op.bn, fl == 2 && !wide ? op.glds_variant : 0,
                fl == 4 ? op.sb_mt : 0, fl == 4 ? op.sb_nt : 0, p.tiles_x, p.tiles_y, p.img_groups, p.n_ntiles, p.ksplit, p.persist, sbk ? p.sb_order : 0, p.reverse, p.dma1x1, out_parts,
                fl == 4 ? 1 : fl == 5 ? 2 : 0);
        fprintf(f, "f%d%s bn%d%s\\n", <the flavour, shape, bn and " x16" arguments of run_unet's snprintf, copied verbatim>);
        fclose(f);
    }

The driver builds plans only: one forward per (model, dtype, shape, option set) with weights of no consequence (the choice reads shapes alone).  Identical
(inputs, options) rows are stored once, and the driver refuses a log in which the same inputs gave two different decisions (the recorded inputs would
then not be everything the decision reads).
"""
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.dont_write_bytecode = True

# one change at a time against the shipped defaults
ARMS = [{}] + [{k: v} for k, vs in dict(
    batch_invariant=[1], glds=[0], splitk=[0], sb=[0], s16=[0, 2], sb_m4=[1], sb_splitk=[0], sb_mt=[1, 2, 4], sb_nt=[1, 2], sb_order=[0, 1],
    glds_variant=[0, 1], glds_bn=[64, 96, 128], glds_bn64=[0], glds_round_aware=[0], glds_tiny=[1], glds_min_wgs=[192], glds_dma1x1=[0],
    glds_wide=[0, 2], glds_wide_tail=[0, 2], glds_wide_persist=[1], glds_wide_mfma16=[0], fewcout=[0], walk_alternate=[0], bn128_min_wgs=[1]).items() for v in vs]
ARMS.append(dict(glds_tiny=1, sb=0))   # the one pair: with the small-batch flavour on, it takes every launch the tiny tile would get
WIDE_ARMS = [a for a in ARMS if not a or next(iter(a)).startswith("glds_wide") or "fewcout" in a]   # the 512 x 512 plans: these only (run time)


def main():
    parent = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "conv_select.npz")
    log = os.environ.get("TD_CONV_SELECT_LOG") or tempfile.NamedTemporaryFile(prefix="conv_select_", suffix=".log", delete=False).name   # (a caller's log is kept)
    keep_log = "TD_CONV_SELECT_LOG" in os.environ
    os.environ["TD_CONV_SELECT_LOG"] = log
    if sys.argv[1] != "-":   # "-": only convert the caller's log
        record(parent)
    convert(log, out, keep_log)


def record(parent):
    sys.path[:0] = [parent, os.path.join(parent, "tests"), TESTS]
    import torch
    import terrain_diffusion_amd as td
    assert os.path.abspath(td.__file__).startswith(parent), td.__file__
    import _ae_twin as T
    from _engine_opts import pinned
    from oracle.unet import BASE_CONFIG, COARSE_CONFIG, DECODER_CONFIG, synth_state_dict, tiny_config
    eng = td.engine.get_engine("cuda")
    t0 = time.time()

    def unet(cfg, dtypes, shapes, seed=5):
        """shapes: {dtype: [(n, size, arms), ...]}"""
        sd = synth_state_dict(cfg, seed=seed)
        for dt in dtypes:
            m = td.EDMUnet2D(**cfg, dtype=dt).load_state_dict(sd)
            for n, s, arms in shapes[dt]:
                x = torch.zeros(n, cfg["in_channels"], s, s, device="cuda")
                conds = [torch.zeros(n, d, device="cuda") if typ == "tensor" else torch.zeros(n, device="cuda") for typ, d, _ in cfg["conditional_inputs"]]
                for arm in arms:
                    with pinned(eng, **arm):
                        m(x, torch.full((n,), 1.1), conds)
            m.close()
            print(f"{cfg['model_channels']}ch x {cfg['image_size']} {dt}: {time.time() - t0:.0f} s", flush=True)

    tiny = [(n, s, ARMS) for s in (24, 40, 72) for n in (1, 2, 3)]
    tiny16 = [(n, s, ARMS) for s in (24, 40, 64) for n in (1, 64)]   # (72: 81 midblock tokens, more than the scalar attention kernel of fp16 / fp32 holds)
    unet(tiny_config(64, 1), ("bf16", "fp16", "fp32"), {"bf16": tiny + [(64, s, ARMS) for s in (24, 40, 72)], "fp16": tiny16, "fp32": tiny16})
    unet(COARSE_CONFIG, ("bf16",), {"bf16": [(n, 16, ARMS) for n in (1, 8, 64)]})
    unet(dict(BASE_CONFIG), ("bf16", "fp16", "fp32"), {"bf16": [(n, 64, ARMS) for n in (1, 2, 3, 5, 8, 16, 32, 64)], "fp16": [(n, 64, ARMS) for n in (1, 64)],
                                                       "fp32": [(n, 64, ARMS) for n in (1, 64)]})
    unet(DECODER_CONFIG, ("bf16",), {"bf16": [(1, 512, WIDE_ARMS), (4, 512, WIDE_ARMS), (1, 256, ARMS)]})
    # the two autoencoder graph kinds (encoder only / skip-less decoder) at the shapes of tests/test_autoencoder_gpu.py
    g = np.load(os.path.join(TESTS, "golden", "autoencoder.npz"))
    for dt in ("bf16", "fp16", "fp32"):
        m = td.EDMAutoencoder(**T.TINY, dtype=dt).load_state_dict(T.synth_ae_state_dict(T.TINY, seed=77))
        for arm in (ARMS if dt == "bf16" else [{}]):
            with pinned(eng, **arm):
                xa = torch.from_numpy(g["tiny_x_a"]).cuda()
                m.preencode(xa); m.preencode(torch.cat([xa, xa[:1]])); m.preencode(torch.from_numpy(g["tiny_x_b"]).cuda())
                m.decode(torch.from_numpy(g["tiny_means_a"]).cuda()); m.decode(torch.from_numpy(g["tiny_means_b"]).cuda())
                m.decode(torch.zeros(2, 3, 5, 7, device="cuda")); m.preencode_dihedral(torch.zeros(2, 48, 48, device="cuda"), 0.3, 1.7)
        m.close()
    m = td.EDMAutoencoder(**T.RELEASED, dtype="bf16").load_state_dict(T.synth_ae_state_dict(T.RELEASED, seed=78))
    for arm in WIDE_ARMS:
        with pinned(eng, **arm):
            m.encode_dihedral(torch.from_numpy(g["rel_chunk"]).cuda()); m.decode(torch.from_numpy(g["rel_means"]).cuda())
    m.close()
    print(f"autoencoders: {time.time() - t0:.0f} s", flush=True)


def convert(log, out, keep_log):
    import subprocess
    lines = open(log).read().split("\n")
    if not keep_log:
        os.unlink(log)
    seen, order = {}, []
    for case, res in zip(lines[0::2], lines[1::2]):
        key = tuple(int(v) for v in case.split())
        f = res.split(" ", 17)
        val = (tuple(int(v) for v in f[:17]), f[17])
        assert seen.setdefault(key, val) == val, ("one input row, two decisions", key, seen[key], val)
        if seen[key] is val:
            order.append(key)
    exe = os.path.join(tempfile.mkdtemp(), "csel")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(os.path.dirname(TESTS), "terrain_diffusion_amd", "csrc"), os.path.join(TESTS, "conv_select_harness.cpp"), "-o", exe])
    fin, fopt, fout = (l.split() for l in subprocess.check_output([exe, "--fields"]).decode().splitlines())
    order.sort()   # (sorted rows in column-major arrays: long constant runs, a tenth of the compressed size)
    rows = np.array(order, dtype=np.int32)
    assert rows.shape[1] == len(fin) + len(fopt)
    tags = sorted({seen[k][1] for k in order})
    col = np.asfortranarray
    np.savez_compressed(out, inputs=col(rows[:, :len(fin)]), options=col(rows[:, len(fin):]), results=col(np.array([seen[k][0] for k in order], dtype=np.int32)),
                        tag_index=np.array([tags.index(seen[k][1]) for k in order], dtype=np.int16), tags=np.array(tags),
                        input_names=np.array(fin), option_names=np.array(fopt), result_names=np.array(fout))
    print(f"{len(lines) // 2} decisions, {len(order)} distinct rows, {len(tags)} tags -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
