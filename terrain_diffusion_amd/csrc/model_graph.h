// What a model consists of, stated once: the block lists, the parameters it owns and the fused ops it runs, for the EDMUnet2D and the two stacks of the
// EDMAutoencoder.  Host only (no HIP include, no pointers, no map sizes; plain g++ -std=c++17 compiles it): tests/model_graph_harness.cpp prints a graph
// and tests/test_model_graph_cpu.py compares it with tests/golden/model_graph.npz on the CPU.  engine.hip reads the list twice: finalize() folds and
// packs the weight side of every K-segment, build_plan() wires the activation side of the same segments at a shape (N, H, W).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/td_engine.h"
#include "conv_select.h"

namespace td {

static const float kMixRes = 0.7f / 0.76157731058639082f;   // (1-0.3)/sqrt(0.7^2+0.3^2)
static const float kMixNew = 0.3f / 0.76157731058639082f;

struct GraphBlock {
    std::string name;
    bool is_conv = false;      // the plain first conv
    bool enc = true;
    int cin = 0, cout = 0;
    int resample = 0;          // 0 keep 1 down 2 up
    bool attn = false;
    bool concat = false;
    int skip_c = 0;
    int cvec_off = 0;          // offset into the concatenated per-block c vectors
};

struct GraphParam {
    std::string name;
    int ndim = 0;
    int64_t shape[4] = {0, 0, 0, 0};
};

// An activation tensor: `level` halvings of the model input's map (negative: doublings, the autoencoder's decoder grows its latent).  Tensor 0 is the input.
struct GraphTensor { int C = 0, level = 0; };

// One K-segment of a fused conv, both sides: a slice of a (folded) reference weight tensor, and the activations it multiplies
struct GraphSeg {
    std::string wname;         // weight parameter [cout][cin_tot][k][k]
    std::string gain;          // scalar parameter folded into it ("": 1)
    int cin_tot = 0, cin_off = 0, c_real = 0, c_pad = 0, taps = 9;
    float mul = 1.f;           // constant folded into the packed weights
    int src = 0;               // tensor id
    int resample = 0, xform = 0;   // ConvSeg::resample / xform
    float scale = 1.f;
    GraphSeg& from(int src_, int resample_ = 0, int xform_ = 0, float scale_ = 1.f) { src = src_; resample = resample_; xform = xform_; scale = scale_; return *this; }
};

struct GraphOp {
    bool attn = false;         // self-attention over the map: reads tensor `qkv`, writes `out` (C = cout channels); everything below `out` is a conv's
    std::string label;
    std::string block;         // ATTN: the block it belongs to (error texts)
    int level = 0, cout = 0;
    int out = 0;               // tensor id
    int qkv = -1;
    std::vector<GraphSeg> segs;   // 1 to 3
    int epi = EPI_PLAIN;
    int cvec_off = -1;         // EPI_EMB_SILU: offset of this block's c vector
    int res = -1, res_resample = 0;   // EPI_RESIDUAL: residual tensor or -1
    bool res_norm = false;     // ... pixel-normalised
    float clip = 0.f;
    bool want_sumsq = false;   // the consumer pixel-normalises the output
    bool out_f32 = false;      // the model output F
};

struct ModelGraph {
    std::vector<GraphBlock> enc, dec;
    int emb_ch = 0, noise_dims = 0, c_total = 0, final_c = 0;
    int max_cout = 64;         // over the blocks, at least 64
    bool cout16 = true;        // every block's cout is a multiple of 16
    std::string out_label, out_gain_name;
    std::vector<GraphParam> params;
    std::vector<GraphTensor> tensors;
    std::vector<GraphOp> ops;
    std::string err;           // text of the error build_model_graph returned
};

// kind 0: the EDMUnet2D (edm_unet.py:105-139; encoder + skip-concat decoder, modulated by an embedding).  The two stacks of the EDMAutoencoder
// (edm_autoencoder.py:66-103) have no embedding parameters (the reference's unused `emb_gain` scalars are not expected) and `c` carries the stack's own
// channels: kind 1 the encoder alone, out_conv on the bottleneck (in_channels -> 2 * latent_channels); kind 2 the skip-less decoder behind a 1x1
// decoder_conv (latent + direct channels -> out_channels), `lpb_dec` its layers_per_block_decoder.  Block and parameter names are the reference's
// state-dict keys.  chunk: channels per 128-byte K chunk (32 fp32, 64 16-bit).  Returns TD_OK, or the error code with its text in g.err.
inline int build_model_graph(const td_unet_config& c, int kind, const int32_t* lpb_dec, int chunk, ModelGraph& g) {
    g = ModelGraph();
    auto fail = [&](int code, const std::string& msg) { g.err = msg; return code; };
    auto param = [&](const std::string& name, std::initializer_list<int64_t> shape) {
        GraphParam p;
        p.name = name;
        for (auto s : shape) p.shape[p.ndim++] = s;
        g.params.push_back(std::move(p));
    };
    if (c.n_levels < 1 || c.n_levels > 8) return fail(TD_ERR_ARG, "n_levels out of range");
    auto has_attn = [&](int res) { for (int i = 0; i < c.n_attn_resolutions; ++i) if (c.attn_resolutions[i] == res) return true; return false; };
    const std::string pre = kind == 1 ? "encoder." : "";
    g.out_label = pre + "out_conv"; g.out_gain_name = pre + "out_gain";

    // ---- blocks
    int cout = c.in_channels + 1;
    if (kind != 2)   // edm_unet.py:107-121
        for (int l = 0; l < c.n_levels; ++l) {
            const int ch = c.model_channels * c.channel_mults[l], res = c.image_size >> l;
            const std::string r = pre + "enc." + std::to_string(res) + "x" + std::to_string(res);
            GraphBlock b;
            if (l == 0) { b.name = r + "_conv"; b.is_conv = true; b.cin = cout; b.cout = ch; cout = ch; }
            else { b.name = r + "_down"; b.cin = cout; b.cout = cout; b.resample = 1; }
            g.enc.push_back(b);
            for (int i = 0; i < c.layers_per_block[l]; ++i) {
                GraphBlock k;
                k.name = r + "_block" + std::to_string(i);
                k.cin = cout; k.cout = ch; k.attn = has_attn(res); cout = ch;
                g.enc.push_back(k);
            }
        }
    auto dec_block = [&](const std::string& name, int cout_, int resample, bool attn, int skip_c) {
        GraphBlock k;
        k.name = name; k.enc = false; k.concat = skip_c > 0; k.skip_c = skip_c;
        k.cin = cout + skip_c; k.cout = cout_; k.resample = resample; k.attn = attn; cout = cout_;
        g.dec.push_back(k);
    };
    if (kind == 2) cout = c.model_channels * c.channel_mults[c.n_levels - 1];   // behind decoder_conv
    if (kind != 1) {   // edm_unet.py:122-139; edm_autoencoder.py:87-101 (blocks "decoder.<index>", no skips)
        std::vector<int> skips;
        for (auto& b : g.enc) skips.push_back(b.cout);
        for (int l = c.n_levels - 1; l >= 0; --l) {
            const int ch = c.model_channels * c.channel_mults[l], res = c.image_size >> l;
            const std::string r = "dec." + std::to_string(res) + "x" + std::to_string(res);
            auto name = [&](const std::string& unet_name) { return kind == 0 ? r + unet_name : "decoder." + std::to_string(g.dec.size()); };
            if (l == c.n_levels - 1) { dec_block(name("_in0"), cout, 0, c.midblock_attention != 0, 0); dec_block(name("_in1"), cout, 0, false, 0); }
            else dec_block(name("_up"), cout, 2, false, 0);
            const int n = (kind == 0 ? c.layers_per_block[l] : lpb_dec[l]) + 1;
            for (int i = 0; i < n; ++i) {
                int skip_c = 0;
                if (kind == 0) { skip_c = skips.back(); skips.pop_back(); }
                dec_block(name("_block" + std::to_string(i)), ch, 0, has_attn(res), skip_c);
            }
        }
    }
    g.final_c = cout;
    for (auto* list : {&g.enc, &g.dec})
        for (auto& b : *list) { g.max_cout = std::max(g.max_cout, b.cout); g.cout16 = g.cout16 && b.cout % 16 == 0; }

    // ---- parameters in front of the blocks', and what a config is refused for
    if (kind == 0) {
        int maxm = 0;
        for (int l = 0; l < c.n_levels; ++l) maxm = std::max(maxm, c.channel_mults[l]);
        g.emb_ch = c.emb_channels ? c.emb_channels : c.model_channels * maxm;
        g.noise_dims = c.noise_emb_dims ? c.noise_emb_dims : c.model_channels;
        param(g.out_gain_name, {});
        param("noise_fourier.freqs", {g.noise_dims / 2});
        param("noise_linear.weight", {g.emb_ch, g.noise_dims});
        if (c.n_cond < 0 || c.n_cond > 8) return fail(TD_ERR_ARG, "n_cond out of range");
        for (int i = 0; i < c.n_cond; ++i) {
            const std::string cl = "conditional_layers." + std::to_string(i);
            if (c.cond_type[i] == 0) param(cl + ".weight", {g.emb_ch, c.cond_dims[i]});
            else if (c.cond_type[i] == 1) {
                param(cl + ".0.freqs", {c.cond_dims[i]});
                param(cl + ".0.phases", {c.cond_dims[i]});
                param(cl + ".1.weight", {g.emb_ch, c.cond_dims[i]});
            } else return fail(TD_ERR_UNSUPPORTED, "conditional input type (embedding tables are not on the accelerated path)");
        }
    }
    for (auto& b : g.enc) if (!b.is_conv && (b.cout % 64 || b.cin % 64)) return fail(TD_ERR_UNSUPPORTED, "block channels must be multiples of 64: " + b.name);
    for (auto& b : g.dec) if (b.cout % 64 || b.cin % 64) return fail(TD_ERR_UNSUPPORTED, "block channels must be multiples of 64: " + b.name);
    if (kind == 0 && c.in_channels + 1 > 32) return fail(TD_ERR_UNSUPPORTED, "in_channels+1 must fit one K chunk (<=32)");
    if (kind == 0 && c.out_channels > 8) return fail(TD_ERR_UNSUPPORTED, "out_channels must be <= 8");

    // ---- ops
    int level = 0, cur = 0;
    g.tensors.push_back({chunk, 0});   // the input: ones channel appended, zero padded to one K chunk
    auto wseg = [&](const std::string& wname, int cin_tot, int cin_off, int c_real, int taps, float mul) {
        GraphSeg s;
        s.wname = wname; s.cin_tot = cin_tot; s.cin_off = cin_off; s.c_real = c_real; s.c_pad = (c_real + chunk - 1) / chunk * chunk; s.taps = taps; s.mul = mul;
        return s;
    };
    auto conv = [&](const std::string& label, int cout_, std::vector<GraphSeg> segs) {
        GraphOp o;
        o.label = label; o.cout = cout_; o.level = level; o.segs = std::move(segs);
        return o;
    };
    auto emit = [&](GraphOp o) {   // allocates its output
        o.out = (int)g.tensors.size();
        g.tensors.push_back({o.cout, o.level});
        g.ops.push_back(std::move(o));
        return g.ops.back().out;
    };
    auto weight_param = [&](const GraphOp& o) { const GraphSeg& s = o.segs[0]; const int k = s.taps == 9 ? 3 : 1; param(s.wname, {o.cout, s.cin_tot, k, k}); };

    std::vector<int> skips;
    // next_norms: the consumer of this block's output pixel-normalises it directly (an encoder block without skip conv)
    auto block = [&](GraphBlock& b, bool next_norms) {
        const std::string& n = b.name;
        if (b.is_conv) {
            GraphOp o = conv(n, b.cout, {wseg(n + ".weight", b.cin, 0, b.cin, 9, 1.f).from(cur)});
            o.want_sumsq = next_norms;
            weight_param(o);
            cur = emit(o);
            return;
        }
        const std::string res0 = n + ".conv_res0", res1 = n + ".conv_res1", skip = n + ".conv_skip", qkv = n + ".attn_qkv", proj = n + ".attn_proj";
        const bool change = b.cin != b.cout;
        if (kind == 0) { b.cvec_off = g.c_total; g.c_total += b.cout; param(n + ".emb_gain", {}); }
        param(res0 + ".weight", {b.cout, b.enc ? b.cout : b.cin, 3, 3});
        if (kind == 0) param(n + ".emb_linear.weight", {b.cout, g.emb_ch});
        param(res1 + ".weight", {b.cout, b.cout, 3, 3});
        if (change) param(skip + ".weight", {b.cout, b.cin, 1, 1});
        if (b.attn) {
            param(qkv + ".weight", {3 * b.cout, b.cout, 1, 1});
            param(proj + ".weight", {b.cout, b.cout, 1, 1});
        }
        if (b.resample == 1) ++level;
        if (b.resample == 2) --level;
        GraphOp o0, o1;   // conv_res0: EPI_EMB_SILU; conv_res1 on its output: mixes the new branch into the block's input
        if (b.enc) {
            int xs = cur, rs = b.resample;
            if (change) {
                GraphOp s = conv(skip, b.cout, {wseg(skip + ".weight", b.cin, 0, b.cin, 1, 1.f).from(cur, rs)});
                s.want_sumsq = true;
                xs = emit(s); rs = 0;
            }
            o0 = conv(res0, b.cout, {wseg(res0 + ".weight", b.cout, 0, b.cout, 9, 1.f).from(xs, rs, 2)});
            o1 = conv(res1, b.cout, {wseg(res1 + ".weight", b.cout, 0, b.cout, 9, kMixNew)});
            o1.res = xs; o1.res_resample = rs; o1.res_norm = true; o1.want_sumsq = next_norms && !b.attn;
        } else {
            int sk = -1;
            if (b.concat) { sk = skips.back(); skips.pop_back(); }
            const int cx = b.cin - b.skip_c;
            float sa = 1.f, sb = 1.f;
            if (b.concat) {  // mp_concat([x, skip], w=[1-t, t]) — mp_layers.py:65-86
                double t = c.concat_balance, wa = 1.0 - t, wb = t, C = sqrt((double)b.cin / (wa * wa + wb * wb));
                sa = (float)(C / sqrt((double)cx) * wa); sb = (float)(C / sqrt((double)b.skip_c) * wb);
            }
            std::vector<GraphSeg> s0 = {wseg(res0 + ".weight", b.cin, 0, cx, 9, 1.f).from(cur, b.resample, 1, sa)};
            if (b.concat) s0.push_back(wseg(res0 + ".weight", b.cin, cx, b.skip_c, 9, 1.f).from(sk, 0, 1, sb));
            o0 = conv(res0, b.cout, s0);
            std::vector<GraphSeg> s1 = {wseg(res1 + ".weight", b.cout, 0, b.cout, 9, kMixNew)};
            if (change) {  // 1x1 skip conv over the mp_concat'ed input, fused as extra K segments
                s1.push_back(wseg(skip + ".weight", b.cin, 0, cx, 1, kMixRes * sa).from(cur, b.resample));
                if (b.concat) s1.push_back(wseg(skip + ".weight", b.cin, cx, b.skip_c, 1, kMixRes * sb).from(sk));
            }
            o1 = conv(res1, b.cout, s1);
            if (!change) { o1.res = cur; o1.res_resample = b.resample; }
        }
        o0.epi = EPI_EMB_SILU; o0.cvec_off = b.cvec_off;
        o1.segs[0].from(emit(o0));
        o1.epi = EPI_RESIDUAL; o1.clip = b.attn ? 0.f : 256.f;
        int o = emit(o1);
        if (b.attn) {
            const int q = emit(conv(qkv, 3 * b.cout, {wseg(qkv + ".weight", b.cout, 0, b.cout, 1, 1.f).from(o)}));
            GraphOp a;
            a.attn = true; a.label = n + ".attn"; a.block = n; a.cout = b.cout; a.level = level; a.qkv = q;
            const int att = emit(a);
            GraphOp p = conv(proj, b.cout, {wseg(proj + ".weight", b.cout, 0, b.cout, 1, kMixNew).from(att)});
            p.epi = EPI_RESIDUAL; p.res = o; p.clip = 256.f; p.want_sumsq = next_norms;
            o = emit(p);
        }
        cur = o;
    };
    if (kind == 2) {   // decoder_conv: 1x1 over latent + direct + ones channels (edm_autoencoder.py:89,137-138)
        const int cin = c.in_channels + 1;
        GraphOp o = conv("decoder_conv", g.dec.front().cin, {wseg("decoder_conv.weight", cin, 0, cin, 1, 1.f).from(cur)});
        weight_param(o);
        cur = emit(o);
    }
    for (size_t i = 0; i < g.enc.size(); ++i) {
        block(g.enc[i], i + 1 < g.enc.size() && g.enc[i + 1].cin == g.enc[i + 1].cout);
        skips.push_back(cur);
    }
    for (auto& b : g.dec) block(b, false);
    GraphOp out = conv(g.out_label, c.out_channels, {wseg(g.out_label + ".weight", g.final_c, 0, g.final_c, 9, 1.f).from(cur)});
    out.segs[0].gain = g.out_gain_name;
    out.out_f32 = true;
    weight_param(out);
    emit(out);
    if (kind != 0) param(g.out_gain_name, {});
    return TD_OK;
}

}  // namespace td
