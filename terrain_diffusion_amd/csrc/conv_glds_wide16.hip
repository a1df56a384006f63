// The wide tile of conv_glds_wide.hip on the 16x16x32 MFMA shape, for the 96-cout pure-3x3 launches: 256 pixels (16 x 16) x 96 couts per 4-wave
// workgroup, two workgroups per CU, half-K-step weight ring of four slots fed by LDS-DMA, double-buffered 32-channel halo patch staged through
// registers -- the same tile, pipeline, parameter block, packed weight slab, fused prologues and epilogues as conv_glds_kernel_wide<T, 96, false, false>
// (read that file's header first; what is said there about the staging, the waits and the patch buffers holds here word for word).  What differs is
// the MFMA core: a wave owns 64 px x 96 couts as 4 x 6 blocks of 16 x 16 (96 accumulator registers, as there), one half K-step of 32 channels is ONE
// K = 32 MFMA per block -- 24 per barrier, the matrix time of the 12 32x32x16 MFMAs of the other file -- fed by ten 1-KB fragment reads (6 weight blocks,
// 4 pixel blocks).  On a clock-limited loop the chip holds a higher clock on this shape.  No TAIL, no PERS: those stay on 32x32x16.
//
// K ORDER: 64-channel chunk -> channel half -> tap -> one 32-deep step (two 16-deep steps in the other file): fp32 sums in another order, so results agree
// with the other tiles to fp32 rounding of the sums, not bit for bit.  The sum-of-squares planes add 4 x 8 couts (lane groups) where the other flavours add
// 2 x 16: compared against float64, like every plane.
//
// Operand roles: weights = A (rows = couts), pixels = B (columns).  Lane l holds piece g = l >> 4 (channels 8g .. 8g + 7 of the half) of row / column
// l & 15 on both sides, and on the output rows 4g .. 4g + 3 of column l & 15.  MFMA row m of cout block b stands for cout
//     32 (b >> 1) + 8 (m >> 2) + 4 (b & 1) + (m & 3)
// of the tile, so that the two blocks of a pair give lane group g the couts 32 (b >> 1) + 8g .. + 7 of its pixel: the 16-byte output run (and the
// residual run, and the two f32x4 of the modulation row) without v_permlane32_swap -- epi_unit8n.
//
// LDS layout, against the 16-lane service groups of ds_read_b128, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 (MI355X guide, LDS):
//   * A ring slot (6 KB) holds the six weight blocks in FRAGMENT order: the piece lane l reads for block b lies at b * 1024 + 16 l.  Any 16 distinct
//     lanes of a half-wave then fall on 16 different 16-byte columns of the 256-byte bank window: conflict-free.  The LDS-DMA writes wave-linear and each
//     lane's GLOBAL address is free, so the piece at position p = 64 b + l is fetched from row cout(b, l & 15), 16-byte slot
//     (4 h + (l >> 4)) ^ TD_SWZ(row) of the row's 128 bytes in the unchanged slab (the two channel halves differ by `offset ^ 64`, as there).
//   * The patch keeps its 80-byte pixel pitch (18 x 18 x 80 B, twice; 96 bytes would be conflict-free for 16 pixels of one tile row but costs 10 KB the
//     workgroup does not have).  Pixel (py, px) starts at 16-byte column 5 (18 py + px) = 10 py + 5 px (mod 16).  A service group holds 8 lanes of piece g
//     and 8 of piece g + 1: lanes n & 15 in S1 = {0-3, 12-15} with one, S2 = {4-11} with the other.  Writing A / B for the column sets of the S1 / S2
//     pixels, conflict-freedom of both groups of a half-wave asks A + (B + 1) = Z16 and B + (A + 1) = Z16, hence A = A + 2: A and B are both the even or
//     both the odd columns.  16 consecutive pixels of a row (columns 5 px) cannot do that; 8 pixels of ONE parity of px in one row can (10 k, k = 0 .. 7,
//     are the 8 residues of one parity), and the next row shifts them by 10: the same parity.  So a pixel block is 2 tile rows x the 8 pixels of one px
//     parity, S1 on the upper row and S2 on the lower; a wave (4 tile rows) owns the blocks (rows 0-1, even), (0-1, odd), (2-3, even), (2-3, odd), which
//     lie at COMPILE-TIME distances of one another: one lane base register, every fragment address is "lane base + compile-time (buffer, tap, block)
//     offset" -- no VALU in the tap loop.  A tap shifts every column of a group by the same amount and keeps the argument.
//
// Fragment registers: the pixel fragments are double-buffered by half-step parity (16 more registers than the other file's fragments: 256 in all, no
// spill), the weight fragments reloaded in two halves: behind the 12 MFMAs of cout blocks 0-2 the next half-step's four pixel fragments and weight
// blocks 0-2 are requested (7 reads), behind the 12 MFMAs of blocks 3-5 its blocks 3-5 (3 reads): every read has 12 MFMAs of cover, as in the other
// file.  (A finer interleave -- one weight and one pixel read behind every 4 MFMAs -- schedules as written but makes hipcc spill 34 registers.)
#include "conv_common.h"

namespace td {

#ifdef TD_TRACE
#define TDX_T(v) unsigned long long v = __builtin_amdgcn_s_memtime(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define TDX_TACC(acc, a, b) acc += (b) - (a)
#else
#define TDX_T(v)
#define TDX_TACC(acc, a, b)
#endif

// tile pixel of lane `lane` in pixel block `i` (0 .. 3) of wave `wave`: see the header
__device__ __forceinline__ void w16_pixel(int wave, int i, int lane, int& ty, int& tx) {
    const int n = lane & 15;
    const bool s2 = n >= 4 && n < 12;
    const int k = s2 ? n - 4 : (n < 4 ? n : n - 8);
    ty = wave * 4 + (i >> 1) * 2 + (s2 ? 1 : 0);
    tx = 2 * k + (i & 1);
}

template <typename T>
__global__ __launch_bounds__(256, 2) void conv_glds_kernel_x16(const ConvParams p) {
    typedef typename Half<T>::x8 hx8;
    constexpr int BN = 96;
    constexpr int NTHR = 256, TH = 16, TW = 16;
    constexpr int PW = 18, NPATCH = 18 * 18;
    constexpr int MB = 4, NB = BN / 16, NP = BN / 32;     // pixel blocks, cout blocks, cout-block pairs (= 32-cout groups) of a wave
    constexpr int CHUNK = 64, HALF = 32, PER16 = 8;
    constexpr int A_ITERS = (NPATCH * 4 + NTHR - 1) / NTHR;                 // 6 (four 16-byte pieces per patch pixel and channel half)
    constexpr int A_FULL = NPATCH * 4 / NTHR, A_REM = NPATCH * 4 - A_FULL * NTHR;
    // weight ring: four slots of BN x 64 bytes, half tiles requested three half-steps before their taps; a half tile is 384 pieces: every wave issues two
    // (the second one of waves 2 / 3 goes to the dump area, from the address of their first piece), so that the s_waitcnt immediates are compile-time
    constexpr int NBI = 2;
    constexpr int H_BYTES = BN * 64, RING = 4;
    constexpr int DUMP_BASE = RING * H_BYTES;
    constexpr int PITCH = 80;
    constexpr int A_BASE = DUMP_BASE + 2048, A_BYTES = NPATCH * PITCH;      // two patch buffers: A_BASE, A_BASE + A_BYTES
    constexpr int RN_BASE = A_BASE + 2 * A_BYTES, RN_BYTES = (NPATCH * 4 + 15) / 16 * 16;
    constexpr int CV_BASE = RN_BASE + RN_BYTES;
    constexpr int NUNIT = MB * NP;                                          // 16-byte output runs of a lane
    static_assert(2 * A_BYTES + 2 * PW * PITCH + 2 * PITCH + (2 * PW + 1) * PITCH + 64 < 65536, "ds_read offset field");
    static_assert(A_REM < NTHR && A_ITERS == A_FULL + 1, "patch pieces");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // the ONLY LDS object: its offset is 0
    float* s_rn = (float*)(smem + RN_BASE);
    float* s_cv = (float*)(smem + CV_BASE);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lg = lane >> 4;   // lane group: K piece of the operands, 4-row group of the outputs
#ifdef TD_TRACE
    unsigned long long tr_wait = 0, tr_stage = 0;
#endif
    TDX_T(tr_start);
#ifdef TD_TRACE
    const unsigned long long tr_rt0 = __builtin_amdgcn_s_memrealtime();
#endif

    // workgroup-id decode: conv_glds.hip's (XCD-aware sibling order, alternating walk direction, magic-number divisions).  Only what lives on is pinned to
    // scalar registers: pinning the decode's own operands as well costs eight scalar spills here.
    unsigned k_d1 = p.sb_d1, k_m1 = p.sb_m1, k_m2 = p.sb_m2, k_m3 = p.sb_m3, k_g8 = p.sb_grid8, k_grid = p.sb_grid;
    int k_tx = p.tiles_x, k_ty = p.tiles_y, k_rev = p.reverse, k_cpad = p.CoutPad, k_N = p.N, k_H = p.H, k_W = p.W;
    const unsigned char* k_wpack = (const unsigned char*)p.wpack;
    int k_epi = p.epi, k_Cout = p.Cout, k_cvs = p.cvec_stride;
    int k_c0 = p.seg[0].C, k_c1 = p.seg[1].C, k_c2 = p.seg[2].C, k_t0 = p.seg[0].taps, k_t1 = p.seg[1].taps, k_t2 = p.seg[2].taps;
    const bool k_hres = p.res != nullptr;
    asm volatile("" : "+s"(k_cpad), "+s"(k_N), "+s"(k_H), "+s"(k_W), "+s"(k_wpack), "+s"(k_epi), "+s"(k_Cout), "+s"(k_cvs));
    int n0, y0, x0, co0;
    {
        unsigned ubid = blockIdx.x;
        if (k_g8) ubid = (ubid & 7) * k_g8 + (ubid >> 3);
        if (k_rev) ubid = k_grid - 1 - ubid;
        const unsigned mtile = td_udiv(ubid, k_d1, k_m1);
        const int ntile = (int)(ubid - mtile * k_d1);
        const unsigned q2 = td_udiv(mtile, (unsigned)k_tx, k_m2);
        const int txi = (int)(mtile - q2 * (unsigned)k_tx), ig = (int)td_udiv(q2, (unsigned)k_ty, k_m3), tyi = (int)(q2 - (unsigned)ig * (unsigned)k_ty);
        n0 = ig; y0 = tyi * TH; x0 = txi * TW; co0 = ntile * BN;
    }
    // 64-channel units of the 3x3 segments (the launcher refuses anything else and zeroes the descriptors past nseg), per segment and in all
    const int u0 = k_t0 == 9 ? k_c0 / CHUNK : 0, u1 = (k_t0 == 9 && k_t1 == 9) ? k_c1 / CHUNK : 0, u2 = (u1 > 0 && k_t2 == 9) ? k_c2 / CHUNK : 0;
    const int n3 = u0 + u1 + u2;

    // ---- weight ring: half K-steps (conv_glds_wide.hip); the in-slot placement is the fragment order of the header
    const size_t wstep = (size_t)k_cpad * 128;
    const unsigned char* wchunk = k_wpack + (size_t)co0 * 128;
    const unsigned char* wnext = wchunk;
    unsigned wvoff[NBI];
#pragma unroll
    for (int i = 0; i < NBI; ++i) {
        const int pos = tid + i * NTHR, b = (pos >> 6) % NB, m = pos & 15, j = (pos >> 4) & 3;   // (% NB: the rowless positions of waves 2 / 3 are never fetched)
        const int r = (b >> 1) * 32 + (m >> 2) * 8 + (b & 1) * 4 + (m & 3), x = TD_SWZ(r);
        wvoff[i] = (unsigned)(r * 128 + ((((x & 4) | (j ^ (x & 3)))) << 4));
    }
    const unsigned ldsw = (unsigned)wave * 1024u;
    const bool dump1 = wave >= 2;
    const unsigned voff1 = dump1 ? wvoff[0] : wvoff[1];
    unsigned wslot = 0, rslot = 0;
#define TDX_SLOT_NEXT(X) { X += H_BYTES; if (X == RING * H_BYTES) X = 0; }
    // half tile T (0 .. 20; 18 .. 20 = taps 0 .. 2 of the NEXT unit) of the unit at wchunk
#define TDX_DMA(TILE)                                                                                        \
    {                                                                                                        \
        if ((TILE) == 9) wnext = wchunk;                                                                     \
        if ((TILE) == 18) { wnext += wstep; wchunk = wnext; }                                                \
        const unsigned x_ = ((TILE) >= 9 && (TILE) < 18) ? 64u : 0u;                                         \
        { const unsigned v_ = wvoff[0] ^ x_; const unsigned m_ = ldsw + wslot; TD_GLDS16(v_, wnext, m_, 0); } \
        { const unsigned v_ = voff1 ^ x_; const unsigned m_ = dump1 ? (unsigned)DUMP_BASE + ldsw - 2048u : ldsw + wslot + 4096u; TD_GLDS16(v_, wnext, m_, 0); } \
        TDX_SLOT_NEXT(wslot)                                                                                 \
        if ((TILE) != 8 && (TILE) != 17) wnext += wstep;                                                     \
    }
    TDX_DMA(0); TDX_DMA(1); TDX_DMA(2);
    const bool cv_stage = k_epi == EPI_EMB_SILU && tid < BN;
    float cv_val = 0.f;
    if (cv_stage) {
        if (n0 < k_N && co0 + tid < k_Cout) cv_val = p.cvec[(size_t)n0 * k_cvs + co0 + tid];
    }

    // ---- activation-patch staging (conv_glds_wide.hip): 16-byte pieces, one K-group ahead through registers, transformed on the way into LDS
    u32x4 av[A_ITERS];
    int aoff[A_ITERS];
    const T* seg_src = nullptr;
    int seg_xform = 0, seg_nchunks = 0;
    float seg_scale = 1.f;
#define TDX_SEG_BEGIN(SEG)                                                                                            \
    {                                                                                                                 \
        seg_src = (const T*)p.seg[SEG].src; seg_xform = p.seg[SEG].xform; seg_scale = p.seg[SEG].scale; seg_nchunks = p.seg[SEG].C / CHUNK; \
        const int Hs_ = p.seg[SEG].Hs, Ws_ = p.seg[SEG].Ws, rs_ = p.seg[SEG].resample, cs_ = p.seg[SEG].cstride;      \
        _Pragma("unroll") for (int it_ = 0; it_ < A_ITERS; ++it_) {                                                   \
            int e_ = tid + it_ * NTHR;                                                                                \
            asm volatile("" : "+v"(e_));   /* (the patch coordinates are re-derived per segment: nothing of them lives across the K loop) */ \
            const int pp_ = e_ >> 2, py_ = pp_ / PW, px_ = pp_ - py_ * PW;                                            \
            const int y_ = y0 + py_ - 1, x_ = x0 + px_ - 1;                                                           \
            const bool ok_ = pp_ < NPATCH && n0 < k_N && y_ >= 0 && y_ < k_H && x_ >= 0 && x_ < k_W;                  \
            aoff[it_] = -1;                                                                                           \
            if (ok_) aoff[it_] = src_pixel(n0, y_, x_, Hs_, Ws_, rs_) * cs_ + (e_ & 3) * PER16;                      \
        }                                                                                                             \
    }
    // always issued (offset 0 for zero-fill pieces), by inline asm: the loop's counted waits cover them, TDX_PIN_A -- behind such a wait -- is the point from
    // which the compiler may use the values
#define TDX_LOAD_A(CH, HF)                                                                             \
    {                                                                                                  \
        const T* src_ = seg_src + (CH) * CHUNK + (HF) * HALF;                                          \
        _Pragma("unroll") for (int it_ = 0; it_ < A_ITERS; ++it_) {                                    \
            const unsigned o_ = (unsigned)(aoff[it_] >= 0 ? aoff[it_] : 0) * (unsigned)sizeof(T);      \
            asm volatile(TD_SGPR_GUARD_LOAD "global_load_dwordx4 %0, %1, %2" : "=&v"(av[it_]) : "v"(o_), "s"(src_) : "memory"); \
        }                                                                                              \
    }
#define TDX_PIN_A() { _Pragma("unroll") for (int it_ = 0; it_ < A_ITERS; ++it_) asm volatile("" : "+v"(av[it_])); }
    const unsigned st_base = (unsigned)A_BASE + (unsigned)(tid >> 2) * PITCH + (unsigned)((tid & 3) << 4);
#define TDX_STORE_A(BUF)                                                                               \
    {                                                                                                  \
        _Pragma("unroll") for (int it_ = 0; it_ < A_ITERS; ++it_) {                                    \
            if (it_ < A_FULL || tid < A_REM) {                                                         \
                u32x4 v_ = aoff[it_] >= 0 ? av[it_] : u32x4{0u, 0u, 0u, 0u};                           \
                if (seg_xform != 0 && aoff[it_] >= 0) {                                                \
                    float s_ = seg_scale;                                                              \
                    if (seg_xform == 2) s_ *= s_rn[(tid >> 2) + it_ * (NTHR / 4)];                     \
                    v_ = xform_piece<T>(v_, s_);                                                       \
                }                                                                                      \
                *(u32x4*)(smem + st_base + ((BUF) * A_BYTES + it_ * (NTHR / 4) * PITCH)) = v_;         \
            }                                                                                          \
        }                                                                                              \
    }
    // residual runs of the epilogue: the first A_ITERS of the NUNIT units (unit q = pixel block q / NP, 32-cout group q % NP) are requested during the LAST
    // 3x3 unit into `av` (dead there), the rest at the top of the epilogue.  The run addresses are made where they are used: nothing of them lives across
    // the K loop.
    const bool r_want = k_epi == EPI_RESIDUAL && k_hres;
    bool r_pref = false;
#define TDX_R_PTR(I, DST)                                                                                             \
    {                                                                                                                 \
        int ty_, tx_; ln_ = tid;                                                                                      \
        asm volatile("" : "+v"(ln_));   /* (re-derived where it is used: left to itself hipcc hoists the addresses out of the K loop and spills them) */ \
        w16_pixel(ln_ >> 6, I, ln_, ty_, tx_);                                                                          \
        const int y_ = y0 + ty_, x_ = x0 + tx_;                                                                       \
        const int sp_ = (n0 < k_N && y_ < k_H && x_ < k_W) ? src_pixel(n0, y_, x_, p.res_Hs, p.res_Ws, p.res_resample) : 0; \
        DST = (const T*)p.res + ((size_t)sp_ * p.res_cstride + co0 + 8 * ((ln_ >> 4) & 3));                           \
    }
#define TDX_R_OFF(Q) ((co0 + ((Q) % NP) * 32 + 8 * ((ln_ >> 4) & 3) < k_Cout) ? ((Q) % NP) * 32 : 0)
#define TDX_LOAD_R()                                                                                                  \
    {                                                                                                                 \
        _Pragma("unroll") for (int i_ = 0; i_ < (A_ITERS + NP - 1) / NP; ++i_) {                                      \
            const T* rp_; int ln_; TDX_R_PTR(i_, rp_)                                                                 \
            _Pragma("unroll") for (int j_ = 0; j_ < NP; ++j_) if (i_ * NP + j_ < A_ITERS) av[i_ * NP + j_] = *(const u32x4*)(rp_ + TDX_R_OFF(i_ * NP + j_)); \
        }                                                                                                             \
        r_pref = true;                                                                                                \
    }
    TDX_SEG_BEGIN(0);
    TDX_LOAD_A(0, 0);

    // ---- MFMA operand addressing: ONE lane base per operand, everything else compile-time (made here: the last use of `wave`)
    unsigned xbase;
    {
        int ty, tx;
        w16_pixel(tid >> 6, 0, lane, ty, tx);   // (the wave index as a vector value: as a scalar it was spilled across the pixel-norm fill)
        xbase = (unsigned)A_BASE + (unsigned)(ty * PW + tx) * PITCH + (unsigned)lg * 16u;   // top-left tap of the lane's pixel of block 0
    }
    const unsigned wbase = (unsigned)lane * 16u;

    // ---- per-pixel 1/(eps + rms) of the pixel-normed source, for the patch pixels
    {
        const float* rn_sumsq = nullptr; int rn_parts = 0, rn_Hs = 0, rn_Ws = 0, rn_res = 0; float rn_invc = 0.f;
        if (p.seg[0].xform == 2) { rn_sumsq = p.seg[0].sumsq; rn_parts = p.seg[0].nparts; rn_Hs = p.seg[0].Hs; rn_Ws = p.seg[0].Ws; rn_res = p.seg[0].resample; rn_invc = p.seg[0].inv_c; }
        else if (p.res_sumsq) { rn_sumsq = p.res_sumsq; rn_parts = p.res_nparts; rn_Hs = p.res_Hs; rn_Ws = p.res_Ws; rn_res = p.res_resample; rn_invc = p.res_inv_c; }
        if (rn_sumsq) {
            const size_t npix = (size_t)k_N * rn_Hs * rn_Ws;
            for (int pp = tid; pp < NPATCH; pp += NTHR) {
                const int py = pp / PW, px = pp % PW;
                const int y = y0 + py - 1, x = x0 + px - 1;
                float rn = 0.f;
                if (n0 < k_N && y >= 0 && y < k_H && x >= 0 && x < k_W)
                    rn = pixel_rn(rn_sumsq, rn_parts, npix, src_pixel(n0, y, x, rn_Hs, rn_Ws, rn_res), rn_invc);
                s_rn[pp] = rn;
            }
        }
    }
    {
        int t_ = tid, e_ = k_epi;
        asm volatile("" : "+v"(t_), "+s"(e_));   // (the condition is made again: its masks would otherwise live in scalar registers across the pixel-norm fill)
        if (e_ == EPI_EMB_SILU && t_ < BN) s_cv[t_] = cv_val;
    }

    __syncthreads();  // s_rn visible
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the first patch (and the three half tiles requested in front of it)
    { TDX_PIN_A() TDX_STORE_A(0); }
    f32x4 acc[MB][NB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[i][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    TDX_T(tr_pro);

#define TDX_TOFF(TP) ((((TP) / 3) * PW + ((TP) % 3)) * PITCH)
#define TDX_XOFF(I) ((((I) >> 1) * 2 * PW + ((I) & 1)) * PITCH)
    u32x4 wf_[NB], xf_[2][MB];
#define TDX_READ_W(B0, B1, SLOT) { _Pragma("unroll") for (int b_ = (B0); b_ < (B1); ++b_) wf_[b_] = *(const u32x4*)(smem + (wbase + (SLOT)) + b_ * 1024); }
#define TDX_READ_X(XP, BUF, TOFF) { _Pragma("unroll") for (int i_ = 0; i_ < MB; ++i_) xf_[XP][i_] = *(const u32x4*)(smem + xbase + ((BUF) * A_BYTES + (TOFF) + TDX_XOFF(i_))); }
#define TDX_MFMA(B0, B1, XP)                                                                                \
    {                                                                                                        \
        _Pragma("unroll") for (int b_ = (B0); b_ < (B1); ++b_)                                               \
            _Pragma("unroll") for (int i_ = 0; i_ < MB; ++i_)                                                \
                acc[i_][b_] = Half<T>::mfma16(__builtin_bit_cast(hx8, wf_[b_]), __builtin_bit_cast(hx8, xf_[XP][i_]), acc[i_][b_]); \
    }
    // One half K-step S (0 .. 17) of a 64-channel unit: conv_glds_wide.hip's TDW_HS with the MFMA core of the header.  Pixel fragments of step S live in
    // xf_[S & 1] (18 steps per unit: the parity carries over).
#define TDX_HS(S)                                                                                            \
    {                                                                                                        \
        TDX_T(tA_);                                                                                          \
        /* in flight, oldest first: half tile S + 1 (needed now), [patch loads of S - 2], half tile S + 2, [patch loads of S - 1] */ \
        if ((S) == 1 || (S) == 2 || (((S) == 10 || (S) == 11) && nxt)) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_ITERS + NBI) : "memory"); \
        else if ((S) >= 16 && !nxt) { if (r_now) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_ITERS) : "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); } \
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NBI) : "memory");                                      \
        if ((S) == 6 || (S) == 15) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   /* this wave's patch writes of the previous half-step are out */ \
        TDX_T(tM_); TDX_TACC(tr_stage, tA_, tM_);                                                            \
        __builtin_amdgcn_s_barrier();                                                                        \
        asm volatile("" ::: "memory");                                                                       \
        TDX_T(tB_); TDX_TACC(tr_wait, tA_, tB_);                                                             \
        if ((S) == 3 || ((S) == 12 && nxt)) TDX_PIN_A()   /* (the wait above completed the patch loads) */ \
        if ((S) + 3 < 18 || nxt) TDX_DMA((S) + 3);   /* (nothing is requested past the end of the launch's 3x3 part) */ \
        if ((S) == 0) TDX_LOAD_A(chunk, 1);                                                                  \
        if ((S) == 9 && nxt) { if (newseg) TDX_SEG_BEGIN(seg + 1); TDX_LOAD_A(newseg ? 0 : chunk + 1, 0); }  \
        if ((S) == 15 && r_now) TDX_LOAD_R()                                                                 \
        if ((S) == 5) TDX_STORE_A(1);                                                                        \
        if ((S) == 14 && nxt) TDX_STORE_A(0);                                                                \
        TDX_MFMA(0, NB / 2, (S) & 1);                                                                        \
        if ((S) < 17 || nxt) { TDX_READ_X(((S) + 1) & 1, (((S) + 1) / 9) & 1, TDX_TOFF(((S) + 1) % 9)); TDX_READ_W(0, NB / 2, rslot); } \
        TDX_MFMA(NB / 2, NB, (S) & 1);                                                                       \
        if ((S) < 17 || nxt) { TDX_READ_W(NB / 2, NB, rslot); TDX_SLOT_NEXT(rslot) }                         \
        __builtin_amdgcn_sched_group_barrier(0x008, MB * NB / 2, 0);                                         \
        __builtin_amdgcn_sched_group_barrier(0x100, MB + NB / 2, 0);                                         \
        __builtin_amdgcn_sched_group_barrier(0x008, MB * NB / 2, 0);                                         \
        __builtin_amdgcn_sched_group_barrier(0x100, NB / 2, 0);                                              \
    }
    int seg = 0, chunk = 0;
    if (n3 > 0) {
        // entry of the pipeline: this wave's patch writes are out, half tiles 0 and 1 were issued a prologue ago
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NBI) : "memory");   // half tile 0 (1 and 2 stay in flight)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        TDX_READ_X(0, 0, TDX_TOFF(0));
        TDX_READ_W(0, NB, rslot);
        TDX_SLOT_NEXT(rslot)
    }
    for (int u = 0; u < n3; ++u) {
        const bool last = u + 1 == n3;
        const bool nxt = !last;
        const bool newseg = !last && chunk + 1 == seg_nchunks;
        const bool r_now = r_want && last;
        TDX_HS(0); TDX_HS(1); TDX_HS(2); TDX_HS(3); TDX_HS(4); TDX_HS(5); TDX_HS(6); TDX_HS(7); TDX_HS(8);
        TDX_HS(9); TDX_HS(10); TDX_HS(11); TDX_HS(12); TDX_HS(13); TDX_HS(14); TDX_HS(15); TDX_HS(16); TDX_HS(17);
        if (newseg) { ++seg; chunk = 0; } else ++chunk;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    TDX_T(tr_loop);

    // ---------------- epilogue (conv_glds_wide.hip's, on this kernel's ownership: lane group lg of pixel block i holds couts 32 jp + 8 lg .. + 7 of its pixel)
    int e_Cout = p.Cout, e_epi = p.epi, e_ocs = p.out_cstride;
    float e_rsc = p.res_scale, e_clip = p.clip, e_o2s = p.out2_scale;
    const bool e_hres = p.res != nullptr, e_hrss = p.res_sumsq != nullptr, e_hoss = p.out_sumsq != nullptr, e_ho2 = p.out2 != nullptr;
    asm volatile("" : "+s"(e_Cout), "+s"(e_epi), "+s"(e_ocs), "+s"(e_rsc), "+s"(e_clip), "+s"(e_o2s), "+s"(co0));
    const size_t M = (size_t)k_N * k_H * k_W;
    int elane = tid;
    asm volatile("" : "+v"(elane));   // (the epilogue's pixel coordinates are made here, not carried across the K loop)
    const int elg = (elane >> 4) & 3;
    const bool has_res = e_epi == EPI_RESIDUAL && e_hres;
    constexpr int NRX = NUNIT - A_ITERS;
    u32x4 rx[NRX];
#pragma unroll
    for (int q = 0; q < NRX; ++q) rx[q] = u32x4{0u, 0u, 0u, 0u};
    if (has_res) {
        if (!r_pref) TDX_LOAD_R()   // (a launch without 3x3 units: nothing was requested yet)
#pragma unroll
        for (int i = A_ITERS / NP; i < MB; ++i) {
            const T* rp; int ln_; TDX_R_PTR(i, rp)
#pragma unroll
            for (int j = 0; j < NP; ++j) rx[i * NP + j - A_ITERS] = *(const u32x4*)(rp + TDX_R_OFF(i * NP + j));
        }
    }
    static_assert(A_ITERS % NP == 0, "the prefetched residual runs are whole pixel blocks");
#pragma unroll
    for (int i = 0; i < MB; ++i) {
        int ty, tx;
        w16_pixel(elane >> 6, i, elane, ty, tx);
        const int n = n0, y = y0 + ty, x = x0 + tx;
        const bool ok = n < k_N && y < k_H && x < k_W;
        float ssj[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) ssj[j] = 0.f;
        const size_t pix = ((size_t)n * k_H + y) * k_W + x;
        if (ok) {
            const float rn = e_hrss ? s_rn[(ty + 1) * PW + (tx + 1)] : 1.f;
            T* orow = (T*)p.out + pix * e_ocs + co0 + 8 * elg;
            const float rs = e_rsc * rn;
            const bool want_ss = e_hoss, want_o2 = e_ho2;
            const SiluK k_o2 = silu_k(e_o2s);
            auto body = [&](auto KIND) __attribute__((always_inline)) {
                constexpr int K = decltype(KIND)::value;
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    f32x4 ca = {0.f, 0.f, 0.f, 0.f}, cb = ca;
                    u32x4 rw = {0u, 0u, 0u, 0u};
                    if constexpr (K == 1) {
                        const float* c_ = s_cv + j * 32 + 8 * elg;
                        ca = *(const f32x4*)c_; cb = *(const f32x4*)(c_ + 4);
                    }
                    if constexpr (K == 2) rw = i * NP + j < A_ITERS ? av[i * NP + j < A_ITERS ? i * NP + j : 0] : rx[i * NP + j >= A_ITERS ? i * NP + j - A_ITERS : 0];
                    u32x4 o, o2;
                    epi_unit8n<T>(e_epi, has_res, e_clip, want_ss, want_o2, acc[i][2 * j], acc[i][2 * j + 1], ca, cb, rw, rs, k_o2, o, o2, ssj[j]);
                    if (co0 + j * 32 + 8 * elg < e_Cout) {
                        *(u32x4*)(orow + j * 32) = o;
                        if (want_o2) *(u32x4*)((T*)p.out2 + (orow - (T*)p.out) + j * 32) = o2;
                    } else ssj[j] = 0.f;
                }
            };
            if (e_epi == EPI_EMB_SILU) body(std::integral_constant<int, 1>{});
            else if (has_res) body(std::integral_constant<int, 2>{});
            else body(std::integral_constant<int, 0>{});
        }
        if (e_hoss) {
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                float ss = ssj[j] + __shfl_xor(ssj[j], 16);
                ss += __shfl_xor(ss, 32);
                if (ok && elg == 0 && co0 + j * 32 < k_cpad) p.out_sumsq[(size_t)((unsigned)co0 / 32u + j) * M + pix] = ss;
            }
        }
    }
#undef TDX_TOFF
#undef TDX_XOFF
#undef TDX_HS
#undef TDX_READ_W
#undef TDX_READ_X
#undef TDX_MFMA
#undef TDX_LOAD_A
#undef TDX_PIN_A
#undef TDX_STORE_A
#undef TDX_SEG_BEGIN
#undef TDX_DMA
#undef TDX_SLOT_NEXT
#undef TDX_R_PTR
#undef TDX_R_OFF
#undef TDX_LOAD_R
#ifdef TD_TRACE
    // clock stamps of the diagnostic build, into the launch's scratch planes (p.partial: the harness allocates them), never into an output
    TDX_T(tr_eissue);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    TDX_T(tr_end);
    if (lane == 0) {
        unsigned long long* tb = (unsigned long long*)p.partial + ((size_t)blockIdx.x * 4 + wave) * 16;
        tb[0] = tr_pro - tr_start; tb[1] = tr_loop - tr_pro; tb[2] = tr_end - tr_loop; tb[3] = tr_wait; tb[4] = tr_stage; tb[5] = tr_start; tb[6] = tr_end;
        tb[8] = tr_rt0; tb[9] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 8) | __builtin_amdgcn_s_getreg((3 << 11) | 20);
        tb[10] = __builtin_amdgcn_s_memrealtime();
        tb[7] = tb[10] - tr_rt0; tb[11] = tr_end - tr_eissue;
    }
#endif
}

template <typename T>
static hipError_t launch_glds_wide16_cfg(const ConvParams& p, hipStream_t st) {
    constexpr int BN = 96, NPATCH = 18 * 18;
    constexpr size_t LDS = 4 * (size_t)(BN * 64) + 2048 + 2 * (size_t)NPATCH * 80 + (size_t)(NPATCH * 4 + 15) / 16 * 16 + (size_t)BN * 4;
    static_assert(2 * LDS <= 160 * 1024, "two workgroups per CU");
    if (p.ksplit != 1 || p.persist != 0 || p.W < 16 || p.CoutPad % BN || p.nseg < 1 || p.nseg > 3 || p.kgroups < 1) return hipErrorInvalidValue;
    if (p.out_f32 || (p.Cout & 7) || p.epi == EPI_DPM_STEP) return hipErrorInvalidValue;   // the 16-byte-run epilogue only
    int units = 0;
    for (int s = 0; s < p.nseg; ++s) { if (p.seg[s].taps != 9 || p.seg[s].C % 64) return hipErrorInvalidValue; units += p.seg[s].C / 64; }   // pure 3x3
    if (units != p.kgroups) return hipErrorInvalidValue;
    ConvParams pd = p;
    for (int s = p.nseg; s < 3; ++s) { pd.seg[s].C = 0; pd.seg[s].taps = 0; }   // (the kernel reads all three descriptors in one burst)
    const int mtiles = p.tiles_x * p.tiles_y * p.img_groups, grid = p.n_ntiles * mtiles;
    if (grid <= 0 || (long long)grid * std::max(mtiles, p.n_ntiles) >= ((long long)1 << 32)) return hipErrorInvalidValue;
    pd.sb_d0 = mtiles; pd.sb_m0 = td_magic(mtiles); pd.sb_d1 = p.n_ntiles; pd.sb_m1 = td_magic(p.n_ntiles); pd.sb_m2 = td_magic(p.tiles_x); pd.sb_m3 = td_magic(p.tiles_y);
    pd.sb_grid = grid; pd.sb_grid8 = (grid & 7) == 0 ? (unsigned)grid >> 3 : 0u;
    auto kern = conv_glds_kernel_x16<T>;
    static bool attr_set[64] = {};
    int dev_ = 0; (void)hipGetDevice(&dev_);
    if (dev_ < 0 || dev_ >= 64 || !attr_set[dev_]) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
        if (e != hipSuccess) return e;
        if (dev_ >= 0 && dev_ < 64) attr_set[dev_] = true;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), LDS, st, pd);
    return hipGetLastError();
}

// dtype: 1 bf16, 2 fp16.  96-cout tiles, pure 3x3 launches; the tiling fields as for launch_conv_glds_wide.
hipError_t launch_conv_glds_wide16(const ConvParams& p, int dtype, hipStream_t st) {
    return dtype == 2 ? launch_glds_wide16_cfg<_Float16>(p, st) : launch_glds_wide16_cfg<__bf16>(p, st);
}

}  // namespace td
