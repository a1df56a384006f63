// Host-only harness for tests/test_model_graph_cpu.py: prints the model graph (csrc/model_graph.h) of a config read from stdin.
// Input, whitespace-separated integers: kind chunk image_size in_channels out_channels model_channels n_levels channel_mults[8] layers_per_block[8]
// layers_per_block_decoder[8] n_attn_resolutions attn_resolutions[8] midblock_attention concat_balance(fp32 bits) noise_emb_dims emb_channels n_cond
// cond_type[8] cond_dims[8].  Output, one record per line (floats as fp32 bit patterns):
//   error <code> <text>                                                     and nothing else, for a config the graph refuses
//   scalars emb_ch noise_dims c_total final_c max_cout cout16 out_label out_gain_name
//   block enc|dec name cvec_off
//   param name ndim shape[4]
//   tensor C level
//   conv label level cout epi cvec_off res res_resample res_norm clip want_sumsq out_f32 out nseg
//   seg wname gain|- cin_tot cin_off c_real c_pad taps mul src resample xform scale          (nseg of them behind their conv)
//   attn label level C qkv out
#include <cstdio>
#include <cstring>
#include <iostream>
#include "model_graph.h"
using namespace td;

static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

int main() {
    td_unet_config c;
    memset(&c, 0, sizeof c);
    int kind = 0, chunk = 0;
    int32_t lpb_dec[8];
    unsigned balance = 0;
    auto arr = [](int32_t* a) { for (int i = 0; i < 8; ++i) std::cin >> a[i]; };
    std::cin >> kind >> chunk >> c.image_size >> c.in_channels >> c.out_channels >> c.model_channels >> c.n_levels;
    arr(c.channel_mults); arr(c.layers_per_block); arr(lpb_dec);
    std::cin >> c.n_attn_resolutions; arr(c.attn_resolutions);
    std::cin >> c.midblock_attention >> balance >> c.noise_emb_dims >> c.emb_channels >> c.n_cond;
    arr(c.cond_type); arr(c.cond_dims);
    if (!std::cin || kind < 0 || kind > 2 || (chunk != 32 && chunk != 64)) { fprintf(stderr, "bad input\n"); return 2; }
    memcpy(&c.concat_balance, &balance, 4);
    ModelGraph g;
    if (int rc = build_model_graph(c, kind, lpb_dec, chunk, g)) { printf("error %d %s\n", rc, g.err.c_str()); return 0; }
    printf("scalars %d %d %d %d %d %d %s %s\n", g.emb_ch, g.noise_dims, g.c_total, g.final_c, g.max_cout, (int)g.cout16, g.out_label.c_str(), g.out_gain_name.c_str());
    for (auto& b : g.enc) printf("block enc %s %d\n", b.name.c_str(), b.cvec_off);
    for (auto& b : g.dec) printf("block dec %s %d\n", b.name.c_str(), b.cvec_off);
    for (auto& p : g.params) printf("param %s %d %lld %lld %lld %lld\n", p.name.c_str(), p.ndim, (long long)p.shape[0], (long long)p.shape[1], (long long)p.shape[2], (long long)p.shape[3]);
    for (auto& t : g.tensors) printf("tensor %d %d\n", t.C, t.level);
    for (auto& o : g.ops) {
        if (o.attn) { printf("attn %s %d %d %d %d\n", o.label.c_str(), o.level, o.cout, o.qkv, o.out); continue; }
        printf("conv %s %d %d %d %d %d %d %d %u %d %d %d %d\n", o.label.c_str(), o.level, o.cout, o.epi, o.cvec_off, o.res, o.res_resample, (int)o.res_norm, bits(o.clip),
               (int)o.want_sumsq, (int)o.out_f32, o.out, (int)o.segs.size());
        for (auto& s : o.segs)
            printf("seg %s %s %d %d %d %d %d %u %d %d %d %u\n", s.wname.c_str(), s.gain.empty() ? "-" : s.gain.c_str(), s.cin_tot, s.cin_off, s.c_real, s.c_pad, s.taps, bits(s.mul),
                   s.src, s.resample, s.xform, bits(s.scale));
    }
    return 0;
}
