// Which kernel and tile a fused conv op of the plan runs on: a pure function of the op's shape, its weights' geometry and the plan options.
// Host only (no HIP include, no pointers; plain g++ -std=c++17 compiles it): tests/conv_select_harness.cpp replays tests/golden/conv_select.npz
// through it on the CPU.  engine.hip's plan builder wires an op, fills a ConvSelIn, calls conv_select and copies the geometry into ConvParams.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>

namespace td {

enum { EPI_PLAIN = 0, EPI_EMB_SILU = 1, EPI_RESIDUAL = 2, EPI_DPM_STEP = 3 };   // ConvParams::epi (td_device.h), ConvSelIn::epi, GraphOp::epi (model_graph.h)

// Every engine option the plan builder reads, in the order of the harness's columns.  engine.hip's read_plan_options() reads each once (there the
// shipped defaults live) and build_plan() puts every member into the plan-cache key: an option the builder reads is in the key by construction.
#define TD_PLAN_OPTIONS(X)                                                                                                                          \
    X(batch_invariant) X(attn_mfma) X(bn128_min_wgs) X(glds) X(glds_bn) X(glds_bn64) X(glds_dma1x1) X(glds_min_wgs) X(glds_round_aware)              \
    X(glds_small_max_groups) X(glds_splitk) X(glds_splitk_from_groups) X(glds_splitk_max) X(glds_splitk_min_groups) X(glds_tiny) X(glds_variant)    \
    X(glds_wide) X(glds_wide_min_wgs) X(glds_wide_tail) X(glds_wide_persist) X(glds_wide_mfma16) X(fewcout) X(producer_act) X(s16) X(s16_min_wgs)   \
    X(sb) X(sb_m4) X(sb_max_glds_wgs) X(sb_mt) X(sb_nt) X(sb_order) X(sb_splitk) X(sb_splitk_max) X(sb_splitk_wgs) X(sb_target_wgs) X(splitk)       \
    X(splitk_target_wgs) X(splitk_weighted) X(walk_alternate)

struct PlanOptions {
#define TD_X(name) int64_t name;
    TD_PLAN_OPTIONS(TD_X)
#undef TD_X
    template <typename F> void for_each(F&& f) {
#define TD_X(name) f(#name, name);
        TD_PLAN_OPTIONS(TD_X)
#undef TD_X
    }
};

struct ConvSelSeg { int C = 0, taps = 0, xform = 0, resample = 0, Hs = 0, Ws = 0; };   // C: padded to the K chunk

struct ConvSelIn {
    int N = 0, h = 0, w = 0;           // batch, output map
    int cout = 0, cout_pad = 0;        // real couts, padded to 64
    int kgroups = 0, nseg = 0;         // K chunks over all segments
    ConvSelSeg seg[3];
    int chunk = 64;                    // channels per 128-byte K chunk
    int dt = 0;                        // TD_DTYPE_*: 0 fp32, 1 bf16, 2 fp16
    int bf16 = 0;                      // 16-bit storage (bf16 OR fp16)
    int sb_n3 = 0;                     // leading 3x3 K-groups of the weights; < 0: segment order the fragment-order flavours do not support
    int out_f32 = 0, epi = 0, has_res = 0, clip_pos = 0;
    int n_cus = 256;
    int op_index = 0;                  // position of the op in the plan (walk order)
};

enum class ConvKernel { PerTap = 0, Glds = 1, GldsWide = 2, GldsWide16 = 3, Sb = 4, S16 = 5, FewCout = 6 };
// PerTap: per-tap register-staged kernel (conv_igemm.hip); Glds: LDS-DMA throughput kernel (conv_glds.hip); GldsWide / GldsWide16: its wide tile on the
// 32x32x16 / 16x16x32 MFMA (conv_glds_wide.hip / conv_glds_wide16.hip); Sb: small-batch kernel, K split over the waves of a workgroup (conv_sb.hip);
// S16: deep-level latency kernel, 64 px x 16 couts (conv_s16.hip); FewCout: <= 4 couts on the VALU (conv_fewcout.hip)
enum class ConvWeightCopy { None = 0, Sb = 1, S16 = 2 };   // the fragment-order copy of the weights the kernel reads (made on first use)

struct ConvSel {
    ConvKernel kernel = ConvKernel::PerTap;
    bool narrow = false;               // 8-wide pixel tiles (maps narrower than 16)
    int bn = 64;                       // couts per tile of the PerTap / Glds* kernels (profile labels print it for every kernel)
    int glds_variant = 0;              // Glds: 0 big (8 waves x 256 pixels), 1 small (4 waves x 128 pixels), 2 tiny (64 px x 64 couts)
    int sb_mt = 0, sb_nt = 0;          // Sb: 32-pixel / 32-cout MFMA blocks per workgroup
    int tiles_x = 0, tiles_y = 0, img_groups = 0, n_ntiles = 0, ksplit = 1, persist = 0, sb_order = 0, reverse = 0, dma1x1 = 0;   // -> ConvParams
    int out_parts = 0;                 // pixel-norm partial planes the launch writes per output pixel
    ConvWeightCopy wcopy = ConvWeightCopy::None;
    bool glds_family() const { return kernel == ConvKernel::Glds || kernel == ConvKernel::GldsWide || kernel == ConvKernel::GldsWide16; }
};

// Number of persistent workgroups for a wide-tile launch of `tiles` workgroup tiles on `slots` resident workgroup slots (2 per CU): every workgroup walks
// ceil(tiles / slots) tiles (the last round may be short); a multiple of 8 when the launch's tile count is (XCD ranges).  0 = not worth it (one round).
inline int conv_wide_persist_grid(long long tiles, int slots) {
    if (tiles < 2LL * slots) return 0;
    const long long rounds = (tiles + slots - 1) / slots;
    long long g = (tiles + rounds - 1) / rounds;
    if ((tiles & 7) == 0) g = (g + 7) & ~7LL;
    return (int)std::min<long long>(g, tiles);
}

inline ConvSel conv_select(const ConvSelIn& in, const PlanOptions& o) {
    ConvSel s;
    const int N = in.N, h = in.h, w = in.w, kgroups = in.kgroups, cout_pad = in.cout_pad;
    const bool use_splitk = o.splitk != 0;
    // "batch_invariant": kernel flavour and K order do not depend on the batch size (no split-K, LDS-DMA flavour whenever it
    // applies), so a window's result is bit-identical whatever other windows share its batch / GPU.
    const bool inv = o.batch_invariant != 0;
    bool tail = false;   // any 1x1 K-segment
    for (int i = 0; i < in.nseg; ++i) if (in.seg[i].taps != 9) tail = true;
    s.narrow = w < 16;
    // throughput flavour (bf16, conv_glds.hip).  Two tile variants: "big" = 8 waves on 256 pixels (16x16, or 8x8 x 4 images),
    // one workgroup per CU; "small" = 4 waves on 128 pixels (8x16, or 8x8 x 2 images), two workgroups per CU.  Measured on
    // MI355X (tools/conv_bench.hip sweeps): equal when the grid is >= 4 workgroups per CU, "small" wins below that (8x8 / 16x16
    // levels of a 64-tile batch, everything at batch <= 8), and couts go in 128s unless that leaves < 2 workgroups per CU.
    // Every variant accumulates a given output in the same K order with the same MFMA, so they are bit-identical to each other.
    {
        const int TW2 = s.narrow ? 8 : 16;
        const bool c128 = cout_pad % 128 == 0, c96 = cout_pad % 96 == 0;
        auto tiles = [&](int TH, int NIMG) { return (int64_t)((w + TW2 - 1) / TW2) * ((h + TH - 1) / TH) * ((N + NIMG - 1) / NIMG); };
        // couts in 128s / 96s; 64s (cout_pad is always a multiple of 64) on 16-wide maps for the layers neither divides: the decoder's 64- and
        // 320-channel levels and the few-channel output convs, which would otherwise run on the per-tap flavour (option "glds_bn64")
        const bool c64 = !s.narrow && o.glds_bn64 != 0;
        auto pick_bn = [&](int64_t mt) { return (c128 && (mt * (cout_pad / 128) >= 512 || !c96)) ? 128 : (c96 ? 96 : (c64 ? 64 : 0)); };
        const int64_t mt_big = tiles(s.narrow ? 8 : 16, s.narrow ? 4 : 1), mt_small = tiles(8, s.narrow ? 2 : 1);
        int variant = 0, bn2 = pick_bn(mt_big);
        if (bn2 && mt_big * (cout_pad / bn2) < 1024) { variant = 1; bn2 = pick_bn(mt_small); }
        // short K loops (<= "glds_small_max_groups" K-groups): prologue and epilogue dominate a workgroup's life, two independent small
        // workgroups per CU overlap them (decoder 512x512 / 256x256 levels: 64- and 128-channel convs)
        if (bn2 && !s.narrow && kgroups <= o.glds_small_max_groups) { variant = 1; bn2 = pick_bn(mt_small); }
        // test hooks: "glds_variant" = 0 (big) / 1 (small) and "glds_bn" = 96 / 128 force the tile shape wherever it is legal
        // (tests assert that every legal shape gives bit-identical results: same K order, same MFMA)
        const int64_t fv = o.glds_variant, fbn = o.glds_bn;
        if (bn2 && (fv == 0 || fv == 1)) { variant = (int)fv; bn2 = pick_bn(variant ? mt_small : mt_big); }
        if (bn2 && ((fbn == 128 && c128) || (fbn == 96 && c96) || (fbn == 64 && c64))) bn2 = (int)fbn;
        const int64_t mt2 = variant ? mt_small : mt_big;
        // round quantisation: when both cout tilings are legal, 96s win if they turn a partial last round of the CU slots into full rounds
        // (768-cout layers at 16x16, batch 64: 768 workgroups of 128 couts = 1.5 rounds of 512 slots, 1024 of 96 couts = 2.0 rounds of
        // workgroups that are 3/4 as long); the tile shape never changes the bits
        if (bn2 == 128 && c96 && fbn == 0 && o.glds_round_aware != 0) {
            const int64_t slots_ = variant ? 512 : 256, w128 = mt2 * (cout_pad / 128), w96 = mt2 * (cout_pad / 96);
            const double t128 = (double)((w128 + slots_ - 1) / slots_) * 128.0, t96 = (double)((w96 + slots_ - 1) / slots_) * 96.0 * 1.03;
            if (t96 < 0.9 * t128) bn2 = 96;
        }
        // (grids below "glds_min_wgs" used to fall to the per-tap flavour; with the small-batch flavour available they enter here and take it)
        // The small-batch flavour's own conditions are evaluated HERE: a grid below "glds_min_wgs" may only enter the branch when that flavour
        // will really take it -- otherwise it falls to the per-tap flavour as before (it used to stay on conv_glds with a tiny grid)
        bool sb_avail = in.bf16 && !inv && o.sb != 0 && in.sb_n3 >= 0;
        for (int i = 0; i < in.nseg; ++i) if (in.seg[i].taps != 9 && in.seg[i].xform != 0) sb_avail = false;   // its 1x1 K-groups go straight from global memory to the MFMA
        const bool sb_takes = sb_avail && bn2 && mt2 * (cout_pad / bn2) * 2 <= (variant ? 512 : 256) && mt2 * (cout_pad / bn2) <= o.sb_max_glds_wgs;
        if (in.bf16 && bn2 && o.glds && (inv || sb_takes || mt2 * (cout_pad / bn2) >= o.glds_min_wgs)) {
            s.kernel = ConvKernel::Glds; s.bn = bn2; s.glds_variant = variant;
            int TH2 = variant ? 8 : (s.narrow ? 8 : 16);
            const int NIMG2 = s.narrow ? (variant ? 2 : 4) : 1;
            s.tiles_x = (w + TW2 - 1) / TW2; s.tiles_y = (h + TH2 - 1) / TH2; s.img_groups = (N + NIMG2 - 1) / NIMG2;
            s.n_ntiles = cout_pad / bn2; s.ksplit = 1;
            // too few workgroups to give every SIMD two waves (8x8 level of a 64-tile batch, small batches): split K, the fp32
            // partials are summed in fixed order by conv_splitk_reduce_kernel (not in batch_invariant mode: the K order changes)
            const int64_t wgs = mt2 * s.n_ntiles, slots = variant ? 512 : 256;
            const bool may_split = !inv && use_splitk && o.glds_splitk && wgs * 2 <= slots;
            if (may_split && kgroups >= o.glds_splitk_from_groups)
                s.ksplit = (int)std::min<int64_t>(std::min<int64_t>(o.glds_splitk_max, kgroups / std::max<int64_t>(1, o.glds_splitk_min_groups)), slots / wgs);
            // Latency regime, 16-wide maps (round 3, option "glds_tiny"): in the split-K regime the fp32 partial slabs dominate the traffic -- at
            // batch 1 a forward wrote 0.95 GB and read 1.7 GB against 0.5 GB of weights (profiles/r03_batch1_hbm_traffic.json).  A "tiny" tile
            // (64 px x 64 couts, 4 waves) fills the chip with (pixel tile, cout tile) workgroups instead of K slices: K is split only as far as
            // it takes to reach ~1.5 workgroups per CU (64x64 level of one tile: no split at all).  tools/b1_tiny.sh: 18 -> 12 us (192->192 at
            // 64x64), 31 -> 21 us (384->384), 25 -> 19.5 us (768->384 at 32x32) incl. the reduce launch.  Same K order and MFMA per output as
            // every other shape (bit-identical when neither splits K).
            if (may_split && !s.narrow && variant == 1 && o.glds_tiny != 0) {
                const int64_t wgs_tiny = tiles(4, 1) * (cout_pad / 64);
                if (wgs_tiny <= 384) {
                    s.glds_variant = 2; s.bn = 64; TH2 = 4;
                    s.tiles_y = (h + TH2 - 1) / TH2; s.n_ntiles = cout_pad / 64;
                    s.ksplit = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kgroups, o.glds_splitk_max), 384 / wgs_tiny));
                }
            }
            // Wide tile (conv_glds_wide.hip, round 6): 256 px x 96 / 64 couts on 4 waves, two workgroups per CU, 32-channel K-groups with a double-buffered
            // patch -- half the weight bytes per MFMA through the CU's L2 -> LDS path, 0.6x the LDS fragment reads, half as many workgroup
            // prologues / epilogue drains, no restage barrier.  Taken where its grid still gives every CU slot >= "glds_wide_min_wgs" / 512 workgroups
            // (the 64x64, 32x32 and 16x16 levels of a 64-window batch -- 384 workgroups of 256 pixels there are one round on 3/4 of the slots where 768 of 128 pixels
            // are one and a half rounds: +0.9 % on the bench line, tools/r06_exp3.sh --, the decoder's 512x512 / 256x256 levels) for launches it serves at full speed: 3x3
            // K-segments, optionally followed by untransformed 1x1 segments (streamed by LDS-DMA), 16-bit output in 16-byte runs.  Another K order than the other tiles (channel half outside the
            // taps): never in batch_invariant mode, where the choice must not depend on the batch.  Option "glds_wide": 0 never, 1 this rule, 2 wherever legal.
            {
                const int64_t wmode = o.glds_wide;
                const int bnw = cout_pad % 96 == 0 ? 96 : (cout_pad % 64 == 0 ? 64 : 0);
                // A 1x1 tail (the decoder blocks' fused skip conv) is streamed by LDS-DMA on the wide tile as well, when its sources need no transform at staging.
                // Measured (tools/r06_exp7.sh): level with conv_glds's stream on the base model's 192 / 384-cout layers (360.7 vs 360.8, 320.1 vs 320.5, 267.8 vs
                // 266.9 us), a loss at the 16x16 level (134 -> 145 us) and -1.4 % on the bench line with two lanes; +10 % on the decoder model's 64-cout layers
                // (268 -> 242 us) and +1.7 % on the cascade.  Hence: tails on the wide tile for the 64-cout tile only.  "glds_wide_tail": 0 never, 1 this rule, 2 always.
                const int64_t tmode = o.glds_wide_tail;
                bool pure3 = true;
                for (int i = 0; i < in.nseg; ++i) if (in.seg[i].taps != 9 && (in.seg[i].xform != 0 || tmode == 0 || (tmode == 1 && bnw != 64))) pure3 = false;
                const int64_t wgs_w = bnw ? tiles(16, 1) * (cout_pad / bnw) : 0;
                if (wmode != 0 && !inv && fv < 0 && fbn == 0 && !s.narrow && s.ksplit == 1 && bnw && !in.out_f32 && (in.cout & 7) == 0 && in.nseg <= 3 && (pure3 || wmode == 2) &&
                    (wmode == 2 || wgs_w >= o.glds_wide_min_wgs)) {
                    s.kernel = ConvKernel::GldsWide; s.bn = bnw; s.glds_variant = 0;
                    s.tiles_x = (w + 15) / 16; s.tiles_y = (h + 15) / 16; s.img_groups = N; s.n_ntiles = cout_pad / bnw;
                    // Persistent tile loop of the wide tile (option "glds_wide_persist", default 0): 2 x CUs workgroups walk the launch's tiles, the next tile's first
                    // patch, modulation row and weight half tiles requested under the current tile's taps, staging split by wave (two waves stream weights, two stage
                    // patches).  Exists for the 64-cout tile, pure 3x3 launches over whole 16 x 16 tiles.  Bit-identical to the one-tile-per-workgroup form and,
                    // measured, not faster (profiles/r06_wide_tile_persistent_loop.txt) -- which is why it is off.
                    if (o.glds_wide_persist != 0 && bnw == 64 && !tail && (h & 15) == 0 && (w & 15) == 0 && in.cout == cout_pad)
                        s.persist = conv_wide_persist_grid((long long)s.tiles_x * s.tiles_y * N * s.n_ntiles, 2 * std::max(1, in.n_cus));
                    // The 96-cout, pure-3x3, one-tile-per-workgroup launches -- two thirds of a grid forward's conv time -- exist a second time on the
                    // 16x16x32 MFMA shape (conv_glds_wide16.hip: same tile and pipeline, one 32-deep step per half K-step; another fp32 summation order).
                    // Option "glds_wide_mfma16": 0 the 32x32x16 kernel everywhere, 1 the 16x16x32 kernel for these launches (profiles/wide_mfma16_ab.txt).
                    if (o.glds_wide_mfma16 != 0 && bnw == 96 && !tail && s.persist == 0) s.kernel = ConvKernel::GldsWide16;
                }
            }
            // Small-batch flavour (conv_sb.hip, round 4) wherever the throughput tiles do not fill the chip (workgroups x 2 <= CU slots: the
            // launches that used to split K over WORKGROUPS).  K is split over the four waves of a workgroup and reduced through LDS: no fp32
            // partial planes in HBM, no reduce launch (BASELINE configs[1]: one tile x 20 steps; the 1-16-window batches of the cascade's latent
            // stage).  Tile: 64 px x 64 couts when that gives "sb_target_wgs" workgroups, else 64 x 32, else 32 x 32.  The weight-streaming-bound
            // deep levels (one tile: 8x8 and 16x16 maps, 6 - 21 MB of weights per conv against 24 - 144 workgroups that each ingest <= ~85 GB/s)
            // additionally split K over workgroups, 64 x 32 tiles, ~224 workgroups in all: the partial planes there are small (64 - 256 pixels)
            // and the reduce launch costs less than the weight stream gains (tools/sb_splitk.sh: 8x8 1536->768 39 -> 17 us cold).
            // Not in batch_invariant mode (conv_glds stays pinned): the K order differs, so the choice must not depend on the batch.
            if (sb_takes && s.kernel == ConvKernel::Glds) {
                const int TWs = s.narrow ? 8 : 16;
                auto th_of = [&](int mt) { return s.narrow ? (mt == 2 ? 8 : 4) : (mt == 4 ? 8 : mt == 2 ? 4 : 2); };
                auto sb_wgs = [&](int mt, int nt) { return (int64_t)((w + TWs - 1) / TWs) * ((h + th_of(mt) - 1) / th_of(mt)) * N * (cout_pad / (32 * nt)); };
                const int64_t target = o.sb_target_wgs;
                int mt = 1, nt = 1, ks = 1;
                // round 5: a 128 px x 32 cout tile exists for the launches where 64 x 64 would be chosen and it gives as many workgroups (31 % fewer
                // ingested bytes per workgroup and K-group).  OFF by default (option sb_m4 = 1 takes it): measured level -- -0.3 % / -1 % of a forward at
                // batch 1 / 2, +2.5 % at batch 8, +1 % at 16, -1 % at 32 (profiles/r05_conv_sb_128px_tile.txt)
                if (!s.narrow && o.sb_m4 != 0 && sb_wgs(2, 2) >= target && sb_wgs(4, 1) >= target) { mt = 4; nt = 1; }
                else if (sb_wgs(2, 2) >= target) { mt = 2; nt = 2; } else if (sb_wgs(2, 1) >= target) { mt = 2; nt = 1; }
                else if (use_splitk && o.sb_splitk != 0 && sb_wgs(2, 1) * 2 <= o.sb_splitk_wgs) {
                    mt = 2; nt = 1;
                    ks = (int)std::min<int64_t>(std::min<int64_t>(kgroups, o.sb_splitk_max), (o.sb_splitk_wgs + sb_wgs(2, 1) / 2) / sb_wgs(2, 1));
                }
                const int64_t fmt = o.sb_mt, fnt = o.sb_nt;   // test hooks
                if (fmt == 1 || fmt == 2 || (fmt == 4 && !s.narrow)) { mt = (int)fmt; ks = 1; }
                if (fnt == 1 || fnt == 2) { nt = (int)fnt; ks = 1; if (mt == 4 && fnt == 2 && fmt != 4) mt = 2; }
                if (mt == 4) nt = 1;   // (the 128-pixel tile exists with 32 couts only)
                // Round 5: the launches that would split K over workgroups on top (the weight-streaming-bound 8x8 / 16x16 levels of one or
                // two tiles) take the deep-level latency flavour instead (conv_s16.hip: 64 px x 16 couts, twice the workgroups per weight
                // byte, no partial planes, no reduce launch).  Option "s16": 1 = there (default), 0 = never, 2 = wherever conv_sb applies (test hook).
                // Measured (profiles/r05_conv_s16_deep_levels.txt): it wins where its own grid reaches about half the chip (16x16 level of one tile:
                // 144 workgroups, 8.9 against 10.1 us for 576 -> 576) and loses where it does not (8x8 level: 48 workgroups each streaming
                // 16 x K weights with 36 KB in flight per CU: 12.1 against 9.0 us) -- there split-K over workgroups stays.
                const int64_t wgs16 = sb_wgs(2, 1) * 2;
                const bool s16 = o.s16 == 2 || (o.s16 == 1 && fmt == 0 && fnt == 0 && sb_wgs(2, 2) < target && sb_wgs(2, 1) < target &&
                                                wgs16 <= o.sb_splitk_wgs && wgs16 >= o.s16_min_wgs);
                s.glds_variant = 0; s.img_groups = N; s.tiles_x = (w + TWs - 1) / TWs;
                if (s16) {
                    s.kernel = ConvKernel::S16; s.wcopy = ConvWeightCopy::S16; s.ksplit = 1;
                    s.tiles_y = (h + th_of(2) - 1) / th_of(2); s.n_ntiles = cout_pad / 16;
                } else {
                    s.kernel = ConvKernel::Sb; s.wcopy = ConvWeightCopy::Sb; s.sb_mt = mt; s.sb_nt = nt; s.ksplit = ks < 1 ? 1 : ks;
                    s.tiles_y = (h + th_of(mt) - 1) / th_of(mt); s.n_ntiles = cout_pad / (32 * nt);
                }
                // workgroup order (speed only): the operand that is larger decides which siblings share an XCD's L2.  Weights (every layer
                // of a single tile: 0.2 - 21 MB against <= 4.7 MB of activations): the pixel tiles of a cout tile are adjacent, so an XCD
                // fetches few cout tiles' weights instead of all of them (batch 1: 1636 -> 1121 MB fetched per forward, tools/r04_order.sh);
                // activations (larger batches): the cout tiles of a pixel tile are adjacent and share the halo patch.  Option sb_order forces.
                double wbytes = 0.0, abytes = 0.0;
                for (int i = 0; i < in.nseg; ++i) {
                    wbytes += (double)(in.seg[i].C / in.chunk) * in.seg[i].taps * cout_pad * 128.0;
                    abytes += (double)N * in.seg[i].Hs * in.seg[i].Ws * in.seg[i].C * 2.0;
                }
                s.sb_order = o.sb_order == 0 || o.sb_order == 1 ? (int)o.sb_order : (wbytes >= abytes ? 1 : 0);
            }
        }
    }
    if (s.kernel == ConvKernel::PerTap) {
        const int TH = 8, TW = s.narrow ? 8 : 16, NIMG = s.narrow ? 2 : 1;
        s.tiles_x = (w + TW - 1) / TW; s.tiles_y = (h + TH - 1) / TH; s.img_groups = (N + NIMG - 1) / NIMG;
        const int64_t mt = (int64_t)s.tiles_x * s.tiles_y * s.img_groups;
        s.bn = 64;
        // batch_invariant: the cout tile must not depend on the batch size either -- this flavour keeps its pixel-norm partials per
        // (cout tile, wave column), so a different bn would change the order in which the consumer adds the sums of squares
        if (cout_pad % 128 == 0 && (inv || mt * (cout_pad / 128) >= o.bn128_min_wgs)) s.bn = 128;
        else if (cout_pad % 96 == 0 && (inv || mt * (cout_pad / 96) >= o.bn128_min_wgs)) s.bn = 96;
        s.n_ntiles = cout_pad / s.bn;
        const int64_t base = mt * s.n_ntiles;
        s.ksplit = 1;
        if (use_splitk && !inv && base < o.splitk_target_wgs / 2 && kgroups > 1) s.ksplit = (int)std::min<int64_t>(kgroups, (o.splitk_target_wgs + base - 1) / base);
    }
    // Few-cout flavour (conv_fewcout.hip, round 6): an fp32-output 3x3 conv with <= 4 real couts (the decoder model's 64 -> 1 output conv) does its
    // multiply-adds on the VALU, one pixel per thread, instead of a 64-cout MFMA tile for one cout.  Maps of >= 128 x 128 pixels (a rule of the shape
    // only: also legal in batch_invariant mode); option "fewcout" = 0 keeps the MFMA tile.  If the sampler later fuses its solver step into this conv
    // (EPI_DPM_STEP), the same kernel runs the step in its epilogue: fused and unfused runs of the decoder model have the same bits.
    if (o.fewcout != 0 && (in.dt == 1 || in.dt == 2) && in.out_f32 && in.epi == 0 /* EPI_PLAIN */ && in.cout <= 4 && in.nseg == 1 && in.seg[0].taps == 9 &&
        in.seg[0].xform == 0 && in.seg[0].resample == 0 && in.seg[0].Hs == h && in.seg[0].Ws == w && !in.has_res && !in.clip_pos && (int64_t)h * w >= 128 * 128 && w >= 16) {
        s = ConvSel();
        s.kernel = ConvKernel::FewCout;
        s.tiles_x = (w + 15) / 16; s.tiles_y = (h + 15) / 16; s.img_groups = N; s.n_ntiles = 1;
    }
    if (s.ksplit > 64) s.ksplit = 64;
    // pixel-norm partials of the output: the LDS-DMA and small-batch flavours write one per 32-cout MFMA block, the 64 x 16 flavour one per 16 couts (independent of the tile shape),
    // the per-tap flavour one per (cout tile, wave column), the split-K reduce kernel one per 256 couts
    s.out_parts = s.ksplit > 1 ? (cout_pad + 255) / 256 : s.kernel == ConvKernel::S16 ? cout_pad / 16 : (s.kernel != ConvKernel::PerTap ? cout_pad / 32 : s.n_ntiles * 2);
    if (s.glds_family()) {
        // alternate the walk order of the workgroup grid from conv to conv (option "walk_alternate", speed only): a layer then starts with the
        // rows its producer wrote last, which are still in the 256 MB Infinity Cache (profiles/r03_conv_walk_order_and_stagger.txt)
        if (o.walk_alternate != 0) s.reverse = in.op_index & 1;
        // 1x1 segments by LDS-DMA where the launch qualifies (launch_glds_cfg).  Split-K slices of one or two K-groups (batch 1) do not amortise the
        // stream's start-up (a barrier and one exposed round trip): measured -0.5 % there, -19 % with 18 groups per slice (8x8 level at batch 64)
        s.dma1x1 = (o.glds_dma1x1 != 0 && (s.ksplit == 1 || kgroups >= 4 * s.ksplit)) ? 1 : 0;
    }
    return s;
}

// The part of a conv launch's profile label that depends on the choice: "f<digit><shape> bn<couts>", then `numbers` (the caller's, engine.hip: workgroups,
// split, GFLOP, MB), then " x16" for the 16x16x32 wide tile.  The digits are the kernel families' historical flavour numbers (3 was the persistent
// ping-pong kernel of rounds 2-4); tests and bench.py parse them.
inline std::string conv_sel_tag(const ConvSel& s, const std::string& numbers = "") {
    int digit = 0;
    const char* shape = "";
    switch (s.kernel) {
        case ConvKernel::PerTap: break;
        case ConvKernel::Glds: digit = 2; shape = s.glds_variant == 2 ? "t" : s.glds_variant ? "s" : "b"; break;
        case ConvKernel::GldsWide: case ConvKernel::GldsWide16: digit = 2; shape = s.persist > 0 ? "wp" : "w"; break;
        case ConvKernel::Sb: digit = 4; shape = s.sb_mt == 4 ? "m4n1" : s.sb_mt == 2 ? (s.sb_nt == 2 ? "m2n2" : "m2n1") : (s.sb_nt == 2 ? "m1n2" : "m1n1"); break;
        case ConvKernel::S16: digit = 5; shape = "c16"; break;
        case ConvKernel::FewCout: digit = 6; break;
    }
    char head[48];
    snprintf(head, sizeof head, "f%d%s bn%d", digit, shape, s.bn);
    return head + numbers + (s.kernel == ConvKernel::GldsWide16 ? " x16" : "");
}

}  // namespace td
