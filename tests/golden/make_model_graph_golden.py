"""Generates tests/golden/model_graph.npz: the parameters and fused ops of every model kind AS THE COMMIT BEFORE csrc/model_graph.h STATED THEM (5d97d5d,
where build_blocks / build_blocks_ae listed the parameters, finalize's do_block the weight K-segments and build_plan's loops the activation K-segments),
recorded from that commit's own library on an MI355X.  tests/test_model_graph_cpu.py compares the graph with it on the CPU.

    python tests/golden/make_model_graph_golden.py <checkout of 5d97d5d, instrumented and built> [out.npz]

The checkout's csrc/engine.hip gets the lines below (nothing else changes; without the environment variable they do nothing).  Pointers are printed as they
are; convert() turns them into tensor indices in order of first appearance as an output (0: the model input).  Floats are printed as fp32 bit patterns.

finalize(), in front of the `mk` lambda, in `mk` in front of `return pack_conv(u, cw);`, and in the `seg` lambda in front of its `return s;`:

    std::map<const void*, std::pair<std::string, float>> wn_;
    auto fb_ = [](float v) { unsigned b; memcpy(&b, &v, 4); return b; };

        if (const char* log_ = getenv("TD_MODEL_GRAPH_LOG")) {
            FILE* f = fopen(log_, "a");
            fprintf(f, "weights %s %d %d\\n", label.c_str(), cout_, (int)cw.segs.size());
            for (auto& s : cw.segs) fprintf(f, "wseg %s %u %d %d %d %d %d %u\\n", wn_[s.w].first.c_str(), fb_(wn_[s.w].second), s.cin_tot, s.cin_off, s.c_real, s.c_pad, s.taps, fb_(s.mul));
            fclose(f);
        }

        wn_[s.w] = {wname, gain};

build_plan(), at the end of the `conv` lambda in front of `pl.ops.push_back(op);`:

        if (const char* log_ = getenv("TD_MODEL_GRAPH_LOG")) {
            FILE* f = fopen(log_, "a");
            auto fb_ = [](float v) { unsigned b; memcpy(&b, &v, 4); return b; };
            fprintf(f, "conv %s %d %d %d %d %d %p %d %d %u %d %d %p %d\\n", label.c_str(), h, w, cw.cout, epi, cvec_off, res ? res->ptr : nullptr, res ? res_resample : 0, (int)(res && res_norm),
                    fb_(clip), (int)want_sumsq, (int)out_f32, outT->ptr, p.nseg);
            for (int i = 0; i < p.nseg; ++i) fprintf(f, "aseg %p %d %d %d %d %u\\n", p.seg[i].src, p.seg[i].C, p.seg[i].taps, p.seg[i].resample, p.seg[i].xform, fb_(p.seg[i].scale));
            fclose(f);
        }

and in front of each of the two `pl.ops.push_back(a);` of the attention sub-blocks:

            if (const char* log_ = getenv("TD_MODEL_GRAPH_LOG")) { FILE* f = fopen(log_, "a"); fprintf(f, "attn %s %d %d %d %p %p\\n", a.label.c_str(), h, w, a.C, a.qkv, a.att); fclose(f); }

A K-segment's gain is logged by value; the driver loads every model with distinct non-unit output gains and convert() names the scalar parameter that holds
the value ("-" for 1).  Every model is built in fp32 (K chunk 32) and bf16 (K chunk 64) and runs one batch-1 forward at a small shape (the graph does not
depend on the shape); the parameter list comes from td_unet_param_info / td_ae_param_info.  A golden line has the form tests/model_graph_harness.cpp prints,
with the map (h w) the op ran on in place of its level.
"""
import json
import os
import struct
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def unet_config(cfg, chunk):
    """td_unet_config as terrain_diffusion_amd/unet.py fills it from EDMUnet2D.config (kind 0)"""
    conds = cfg["conditional_inputs"]
    return dict(kind=0, chunk=chunk, image_size=cfg["image_size"], in_channels=cfg["in_channels"], out_channels=cfg["out_channels"], model_channels=cfg["model_channels"],
                n_levels=len(cfg["model_channel_mults"]), channel_mults=list(cfg["model_channel_mults"]), layers_per_block=list(cfg["layers_per_block"]),
                layers_per_block_decoder=[], n_attn_resolutions=len(cfg["attn_resolutions"]), attn_resolutions=list(cfg["attn_resolutions"]),
                midblock_attention=int(bool(cfg["midblock_attention"])), concat_balance_bits=f32_bits(cfg["concat_balance"]), noise_emb_dims=int(cfg["noise_emb_dims"] or 0),
                emb_channels=int(cfg["emb_channels"] or 0), n_cond=len(conds), cond_type=[0 if c[0] == "tensor" else 1 for c in conds], cond_dims=[int(c[1]) for c in conds])


def ae_configs(cfg, chunk):
    """the td_unet_config of the two stacks as td_ae_create (csrc/engine.hip) fills them from EDMAutoencoder.config: kind 1, kind 2"""
    L, D = cfg["latent_channels"], len(cfg["direct_skips"])
    out = []
    for kind in (1, 2):
        out.append(dict(kind=kind, chunk=chunk, image_size=cfg["image_size"], in_channels=cfg["in_channels"] if kind == 1 else L + D,
                        out_channels=2 * L if kind == 1 else cfg["out_channels"], model_channels=cfg["model_channels"], n_levels=len(cfg["model_channel_mults"]),
                        channel_mults=list(cfg["model_channel_mults"]), layers_per_block=list(cfg["layers_per_block"]), layers_per_block_decoder=list(cfg["layers_per_block_decoder"]),
                        n_attn_resolutions=len(cfg["attn_resolutions"]), attn_resolutions=list(cfg["attn_resolutions"]), midblock_attention=int(cfg["midblock_attention"]) if kind == 2 else 0,
                        concat_balance_bits=f32_bits(0.5), noise_emb_dims=0, emb_channels=0, n_cond=0, cond_type=[], cond_dims=[]))
    return out


def convert(log_lines, params, scalars):
    """one graph's log -> golden lines.  params: [(name, shape)] in order; scalars: {fp32 bits: name} of the scalar parameters a gain may be"""
    lines = ["param %s %d %s" % (n, len(s), " ".join(str(int(v)) for v in (list(s) + [0] * 4)[:4])) for n, s in params]
    rec = [l.split(" ") for l in log_lines if l]
    weights, i = [], 0
    while i < len(rec) and rec[i][0] in ("weights", "wseg"):
        if rec[i][0] == "weights":
            n = int(rec[i][3])
            weights.append((rec[i][1], int(rec[i][2]), [r[1:] for r in rec[i + 1:i + 1 + n]]))
            assert all(r[0] == "wseg" for r in rec[i + 1:i + 1 + n])
            i += 1 + n
    ids = {"(nil)": -1}
    xin = []

    def tensor(ptr, define=False):
        if define:
            assert ptr not in ids, "an output buffer written twice"
            ids[ptr] = len(ids)   # 1, 2, ... ("(nil)" occupies one slot; 0 is the input)
        elif ptr not in ids:
            xin.append(ptr)
            assert len(set(xin)) == 1, "more than one tensor that no op wrote"
            return 0
        return ids[ptr]
    wi = 0
    while i < len(rec):
        r = rec[i]
        if r[0] == "attn":
            qkv = tensor(r[5])
            lines.append("attn %s %s %s %s %d %d" % (r[1], r[2], r[3], r[4], qkv, tensor(r[6], True)))
            i += 1
            continue
        assert r[0] == "conv", r
        label, h, w, cout, epi, cvec_off, res, res_resample, res_norm, clip, want_sumsq, out_f32, out, nseg = r[1:]
        nseg = int(nseg)
        wl, wc, wsegs = weights[wi]
        wi += 1
        assert wl == label and wc == int(cout) and len(wsegs) == nseg, ("finalize and build_plan disagree", wl, label)
        segs = []
        for ws, a in zip(wsegs, rec[i + 1:i + 1 + nseg]):
            assert a[0] == "aseg"
            wname, gain, cin_tot, cin_off, c_real, c_pad, taps, mul = ws
            src, C, ataps, resample, xform, scale = a[1:]
            assert C == c_pad and ataps == taps, ("segment/weight mismatch", label)
            gain = "-" if int(gain) == f32_bits(1.0) else scalars[int(gain)]
            segs.append("seg %s %s %s %s %s %s %s %s %d %s %s %s" % (wname, gain, cin_tot, cin_off, c_real, c_pad, taps, mul, tensor(src), resample, xform, scale))
        lines.append("conv %s %s %s %s %s %s %d %s %s %s %s %s %d %d" % (label, h, w, cout, epi, cvec_off, tensor(res), res_resample, res_norm, clip, want_sumsq, out_f32, tensor(out, True), nseg))
        lines += segs
        i += 1 + nseg
    assert wi == len(weights)
    return lines


def main():
    parent = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "model_graph.npz")
    log = tempfile.NamedTemporaryFile(prefix="model_graph_", suffix=".log", delete=False).name
    os.environ["TD_MODEL_GRAPH_LOG"] = log
    sys.path[:0] = [parent, os.path.join(parent, "tests")]
    import torch
    import terrain_diffusion_amd as td
    assert os.path.abspath(td.__file__).startswith(parent), td.__file__
    import _ae_twin as T
    from oracle.unet import BASE_CONFIG, COARSE_CONFIG, DECODER_CONFIG, synth_state_dict, tiny_config
    models = {}

    def take_log():
        with open(log) as f:
            lines = f.read().split("\n")
        open(log, "w").close()
        return lines

    def scalars_of(sd):
        s = {f32_bits(float(v)): k for k, v in sd.items() if torch.as_tensor(v).ndim == 0 and not k.endswith(".emb_gain")}
        assert f32_bits(1.0) not in s
        return s

    for name, cfg, size in (("coarse", COARSE_CONFIG, 16), ("base", dict(BASE_CONFIG), 16), ("decoder", DECODER_CONFIG, 16), ("tiny", tiny_config(64, 1), 16),
                            ("tiny_attn", tiny_config(64, 2, image_size=32), 16)):
        sd = synth_state_dict(cfg, seed=5, out_gain=1.75)
        for dt, chunk in (("fp32", 32), ("bf16", 64)):
            take_log()
            m = td.EDMUnet2D(**cfg, dtype=dt).load_state_dict(sd)
            x = torch.zeros(1, cfg["in_channels"], size, size, device="cuda")
            conds = [torch.zeros(1, d, device="cuda") if typ == "tensor" else torch.zeros(1, device="cuda") for typ, d, _ in cfg["conditional_inputs"]]
            m(x, torch.full((1,), 1.1), conds)
            models[f"{name}_{dt}"] = dict(config=unet_config(m.config, chunk), shape=[1, size, size], lines=convert(take_log(), list(m.expected_parameters().items()), scalars_of(sd)))
            m.close()
            print(name, dt, len(models[f"{name}_{dt}"]["lines"]), "lines", flush=True)
    for name, cfg, seed in (("ae_tiny", T.TINY, 77), ("ae_released", T.RELEASED, 78)):
        sd = T.synth_ae_state_dict(cfg, seed=seed)
        for dt, chunk in (("fp32", 32), ("bf16", 64)):
            take_log()
            m = td.EDMAutoencoder(**cfg, dtype=dt).load_state_dict(sd)
            L, D, down = m.config["latent_channels"], len(m.config["direct_skips"]), m.down
            m.preencode(torch.zeros(1, cfg["in_channels"], 16, 16, device="cuda"))
            m.decode(torch.zeros(1, L + D, 16 // down, 16 // down, device="cuda"))
            lines = take_log()
            params = list(m.expected_parameters().items())
            # both stacks finalize before either runs: the encoder's records are the ones whose label starts with "encoder."
            labels, mine = [], []
            for l in lines:
                if l.startswith(("weights ", "conv ", "attn ")):
                    labels.append(l.split(" ")[1].startswith("encoder."))
                mine.append(labels[-1] if labels else None)
            for stack, c, shape in zip(("enc", "dec"), ae_configs(m.config, chunk), ([1, 16, 16], [1, 16 // down, 16 // down])):
                enc = stack == "enc"
                models[f"{name}_{stack}_{dt}"] = dict(config=c, shape=shape, lines=convert([l for l, e in zip(lines, mine) if e == enc],
                                                                                              [(n, s) for n, s in params if n.startswith("encoder.") == enc], scalars_of(sd)))
                print(name, stack, dt, len(models[f"{name}_{stack}_{dt}"]["lines"]), "lines", flush=True)
            m.close()
    os.unlink(log)
    save(models, out)


def save(models, out):
    """{name: dict(config, shape, lines)} -> npz: `names`, per model its config as JSON text and its shape, and every model's lines in one array cut at `offsets`"""
    import numpy as np
    names = sorted(models)
    counts = [len(models[n]["lines"]) for n in names]
    np.savez_compressed(out, names=np.array(names), configs=np.array([json.dumps(models[n]["config"], sort_keys=True) for n in names]),
                        shapes=np.array([models[n]["shape"] for n in names], dtype=np.int32), lines=np.array([l for n in names for l in models[n]["lines"]]),
                        offsets=np.cumsum([0] + counts).astype(np.int32))
    print(f"{len(models)} graphs, {sum(counts)} lines -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
