// Shaded-relief rendering of an elevation image: get_relief_map (terrain_diffusion/inference/relief_map.py:64-199).  Two passes:
//   relief_blur_rows_kernel   scipy gaussian_filter's axis-0 pass for BOTH sigmas from one read of the elevation (NaN fill applied on load,
//                             mode='reflect'), two fp32 planes out; fused land min / max of the unfilled input for the automatic colour range.
//   relief_shade_kernel       the axis-1 pass of both blurs on a row tile staged in LDS, np.gradient, the two hillshades, the terrain colormap,
//                             relief blend, NaN and ocean colouring -> (H, W, 3) fp32.  A template: <false> is the picture without biome, flow
//                             or a caller's colours (libtd_relief.so launches only that one), <true> adds those overlays (libtd_rivers.so).
// Per pixel the elementwise arithmetic is the reference's, in its order and in fp32 with no contraction (numpy does not fuse), through the
// precise device libm; the blurs accumulate in fp32 in tap order (scipy accumulates in fp64 and stores fp32 between the passes, as here).
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

namespace td {

constexpr int RELIEF_MAX_RADIUS = 64;     // int(4 sigma + 0.5) <= 64, i.e. sigma < 15.9: LDS tiles below are sized for it
constexpr int RELIEF_THREADS = 256;
constexpr int RELIEF_P1_COLS = 64;        // pass 1: one thread per (column, strip of rows); 4 strips of 16 rows per workgroup
constexpr int RELIEF_P1_ROWS = 64;
constexpr int RELIEF_P2_TX = 128;         // pass 2: output tile 128 x 16, staged with R + 1 columns and 1 row of halo on each side
constexpr int RELIEF_P2_TY = 16;

// scipy.ndimage mode='reflect' (d c b a | a b c d | d c b a): period 2n, folds any number of times for images narrower than the radius
__device__ __forceinline__ int relief_reflect(int i, int n) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// np.clip(x, 0, 1): NaN passes through
__device__ __forceinline__ float relief_clip01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

// Scalars of one render, resolved on the host from the call's arguments in the reference's precision.
struct ReliefParams {
    float az;            // deg2rad(azimuths[0])
    float sin_alt, cos_alt;
    float scale;         // 15 * resolution / 90
    float relief, one_minus_relief;
    double vmin, vmax;   // explicit colour range (has_range)
    int has_range;
    int has_fill;
    float fill;          // NaN fill (nanmedian), applied only when has_fill
};

// The overlays of relief_shade_kernel<true>; a null pointer leaves that overlay out.  relief_shade_kernel<false> ignores the whole struct.
struct ReliefOverlay {
    const float* rgb;        // (H, W, 3) base colour in place of the terrain colormap
    const int* biome;        // (H, W) class ids; where clip(id, 0, 30) > 0 the base colour is palette[id]
    const float* palette;    // 31 x 3
    const float* flow;       // (H, W) flow accumulation; a river where flow > flow_threshold
    float flow_threshold;
};

__device__ __forceinline__ float relief_fill(float v, int has_fill, float fill) {
    // np.nan_to_num(elev, nan=fill): NaN -> fill, +-inf -> +-FLT_MAX (the reference only calls it when the image holds a NaN)
    if (!has_fill) return v;
    return isnan(v) ? fill : (isinf(v) ? (v > 0.f ? FLT_MAX : -FLT_MAX) : v);
}

// Pass 1.  Grid (ceil(W / 64), ceil(H / 64)); dynamic LDS = (64 + 2R) * 64 + (2 rl + 1) + (2 rs + 1) floats, R = max(rl, rs).
// range_bits (null: explicit range, no reduction): [0] = max of ~bits(min land), [1] = max of bits(max land), both cleared to 0 before the launch.
// Land = max(0, elev) >= 0 over the non-NaN pixels: its IEEE bit patterns order as uint32, so the two integer maxima are order-independent.
__global__ __launch_bounds__(RELIEF_THREADS) void relief_blur_rows_kernel(const float* __restrict__ elev, float* __restrict__ bl, float* __restrict__ bs,
                                                                          int H, int W, const float* __restrict__ wl, int rl, const float* __restrict__ ws,
                                                                          int rs, int has_fill, float fill, unsigned* __restrict__ range_bits) {
    extern __shared__ float relief_smem[];
    __shared__ unsigned red[2 * (RELIEF_THREADS / 64)];
    __shared__ int src_row[RELIEF_P1_ROWS + 2 * RELIEF_MAX_RADIUS];   // reflected image row of each tile row
    const int R = rl > rs ? rl : rs;
    const int rows = RELIEF_P1_ROWS + 2 * R;
    float* tile = relief_smem;                       // [rows][64]
    float* wts = relief_smem + rows * RELIEF_P1_COLS;  // wl then ws
    const int tid = threadIdx.x, lx = tid % RELIEF_P1_COLS, grp = tid / RELIEF_P1_COLS;
    const int x0 = blockIdx.x * RELIEF_P1_COLS, y0 = blockIdx.y * RELIEF_P1_ROWS;
    const bool col_ok = x0 + lx < W;
    const int x = col_ok ? x0 + lx : W - 1;           // clamped: every load stays inside the image, stores are guarded
    for (int i = tid; i < 2 * rl + 1; i += RELIEF_THREADS) wts[i] = wl[i];
    for (int i = tid; i < 2 * rs + 1; i += RELIEF_THREADS) wts[2 * rl + 1 + i] = ws[i];
    for (int i = tid; i < rows; i += RELIEF_THREADS) src_row[i] = relief_reflect(y0 - R + i, H);
    __syncthreads();
    unsigned lo = 0u, hi = 0u;
    constexpr int STEP = RELIEF_THREADS / RELIEF_P1_COLS, BATCH = 4;   // BATCH loads in flight per thread
#pragma unroll 1
    for (int r0 = grp; r0 < rows; r0 += STEP * BATCH) {
        float v[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int r = r0 + u * STEP;
            v[u] = r < rows ? elev[(size_t)src_row[r] * W + x] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int r = r0 + u * STEP;
            if (r >= rows) break;
            const int yr = y0 - R + r;
            // each pixel of the image belongs to exactly one workgroup's strip: count it there
            if (range_bits && col_ok && r >= R && r < R + RELIEF_P1_ROWS && yr < H && !isnan(v[u])) {
                const unsigned b = __float_as_uint(v[u] > 0.f ? v[u] : 0.f);
                lo = max(lo, ~b);
                hi = max(hi, b);
            }
            tile[r * RELIEF_P1_COLS + lx] = relief_fill(v[u], has_fill, fill);
        }
    }
    __syncthreads();
    if (col_ok) {
        const float* wsm = wts + 2 * rl + 1;
#pragma unroll 1
        for (int k = 0; k < RELIEF_P1_ROWS / 4; ++k) {
            const int r = grp * (RELIEF_P1_ROWS / 4) + k;
            const int y = y0 + r;
            if (y >= H) break;
            const float* c = tile + (r + R) * RELIEF_P1_COLS + lx;
            float al = 0.f, as = 0.f;
            for (int t = -rl; t <= rl; ++t) al += wts[t + rl] * c[t * RELIEF_P1_COLS];
            for (int t = -rs; t <= rs; ++t) as += wsm[t + rs] * c[t * RELIEF_P1_COLS];
            bl[(size_t)y * W + x] = al;
            bs[(size_t)y * W + x] = as;
        }
    }
    if (range_bits) {   // grid-uniform branch
        for (int o = 32; o > 0; o >>= 1) {
            lo = max(lo, (unsigned)__shfl_xor((int)lo, o, 64));
            hi = max(hi, (unsigned)__shfl_xor((int)hi, o, 64));
        }
        if ((tid & 63) == 0) { red[2 * (tid >> 6)] = lo; red[2 * (tid >> 6) + 1] = hi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < RELIEF_THREADS / 64; ++w) { lo = max(lo, red[2 * w]); hi = max(hi, red[2 * w + 1]); }
            if (lo) atomicMax(range_bits, lo);
            if (hi) atomicMax(range_bits + 1, hi);
        }
    }
}

// hillshade of one gradient sample (compute_hillshade, relief_map.py): the reference forms the final sum in fp64 from fp32 slope / aspect;
// here it stays fp32 (|difference| ~1e-7 against the 1e-4 output bound)
__device__ __forceinline__ float relief_hillshade(float dy, float dx, const ReliefParams& p) {
#pragma clang fp contract(off)
    dy = dy / p.scale;
    dx = dx / p.scale;
    const float slope = 1.57079632679489661923f - atanf(hypotf(dx, dy));
    const float aspect = atan2f(dy, -dx);
    const float hs = p.sin_alt * sinf(slope) + p.cos_alt * cosf(slope) * cosf(p.az - aspect);
    return relief_clip01(hs);
}

// np.gradient along one axis (unit spacing, edge_order=1) at index i of n >= 2, f(j) = sample j
#define RELIEF_GRAD(i, n, f) ((i) == 0 ? (f(1) - f(0)) : ((i) == (n) - 1 ? (f((n) - 1) - f((n) - 2)) : (f((i) + 1) - f((i) - 1)) / 2.f))

// Pass 2.  Grid (ceil(W / 128), ceil(H / 16)); dynamic LDS = relief_shade_lds_floats(R) floats.
// With OVERLAY and ov.rgb the colormap and its range are skipped (range_bits may then be null whatever has_range says).
template <bool OVERLAY>
__global__ __launch_bounds__(RELIEF_THREADS) void relief_shade_kernel(const float* __restrict__ elev, const float* __restrict__ bl, const float* __restrict__ bs,
                                                                      int H, int W, const float* __restrict__ wl, int rl, const float* __restrict__ ws, int rs,
                                                                      const float* __restrict__ lut, const unsigned* __restrict__ range_bits, ReliefParams p,
                                                                      ReliefOverlay ov, float* __restrict__ out) {
#pragma clang fp contract(off)
    extern __shared__ float relief_smem[];
    const int R = rl > rs ? rl : rs;
    constexpr int NR = RELIEF_P2_TY + 2, FW = RELIEF_P2_TX + 2;
    const int SW = FW + 2 * R;
    float* sl = relief_smem;       // [NR][SW] axis-0-blurred planes, staged
    float* ss = sl + NR * SW;
    float* fl = ss + NR * SW;      // [NR][FW] fully blurred, rows y0-1 .. y0+TY, columns x0-1 .. x0+TX
    float* fs = fl + NR * FW;
    float* lut_s = fs + NR * FW;   // [256][3]
    float* wts = lut_s + 256 * 3;  // wl then ws
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * RELIEF_P2_TX, y0 = blockIdx.y * RELIEF_P2_TY;
    for (int i = tid; i < 256 * 3; i += RELIEF_THREADS) lut_s[i] = lut[i];
    for (int i = tid; i < 2 * rl + 1; i += RELIEF_THREADS) wts[i] = wl[i];
    for (int i = tid; i < 2 * rs + 1; i += RELIEF_THREADS) wts[2 * rl + 1 + i] = ws[i];
    // stage: row y0-1+r (clamped into the image; rows outside it are never read below), column x0-1-R+j reflected
    for (int i = tid; i < NR * SW; i += RELIEF_THREADS) {
        const int r = i / SW, j = i - r * SW;
        int gy = y0 - 1 + r;
        gy = gy < 0 ? 0 : (gy >= H ? H - 1 : gy);
        const size_t g = (size_t)gy * W + relief_reflect(x0 - 1 - R + j, W);
        sl[i] = bl[g];
        ss[i] = bs[g];
    }
    __syncthreads();
    {   // axis-1 pass of both blurs (fused multiply-adds allowed here, as in pass 1)
#pragma clang fp contract(fast)
        const float* wsm = wts + 2 * rl + 1;
        for (int i = tid; i < NR * FW; i += RELIEF_THREADS) {
            const int r = i / FW, c = i - r * FW;
            const float* a = sl + r * SW + c + R;
            const float* b = ss + r * SW + c + R;
            float al = 0.f, as = 0.f;
            for (int t = -rl; t <= rl; ++t) al += wts[t + rl] * a[t];
            for (int t = -rs; t <= rs; ++t) as += wsm[t + rs] * b[t];
            fl[i] = al;
            fs[i] = as;
        }
    }
    __syncthreads();
    // colour range (step 5 of the reference), resolved here so that the automatic range needs no host round trip
    const bool colormap = !OVERLAY || !ov.rgb;   // grid-uniform
    double vmin = 0.0, vmax = 1.0;
    if (colormap && p.has_range) {
        vmin = p.vmin > 0.0 ? p.vmin : 0.0;
        vmax = p.vmax;
    } else if (colormap) {
        const float lo = __uint_as_float(~range_bits[0]), hi = __uint_as_float(range_bits[1]);
        vmin = lo;
        vmax = hi;
        if (!isfinite(lo) || !isfinite(hi) || lo == hi) { vmin = 0.0; vmax = 1.0; }
    }
    const bool offset = vmin == 0.0;
    const float vmin_f = (float)vmin, den = (float)(vmax - vmin + 1e-8);
    const float relief = p.relief, omr = p.one_minus_relief;

    for (int k = 0; k < RELIEF_P2_TX * RELIEF_P2_TY / RELIEF_THREADS; ++k) {
        const int q = tid + k * RELIEF_THREADS;
        const int ty = q / RELIEF_P2_TX, tx = q - ty * RELIEF_P2_TX;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        const size_t px = (size_t)y * W + x;
        const float e = elev[px];
        const bool is_nan = isnan(e);
        const float ef = relief_fill(e, p.has_fill, p.fill);
        // np.gradient of both blurred fields; LDS row (ty+1)+d is image row y+d, column (tx+1)+d is image column x+d
        const int cy = ty + 1, cx = tx + 1;
#define FLY(j) fl[(cy + (j) - y) * FW + cx]
#define FLX(j) fl[cy * FW + cx + (j) - x]
#define FSY(j) fs[(cy + (j) - y) * FW + cx]
#define FSX(j) fs[cy * FW + cx + (j) - x]
        const float hl = relief_hillshade(RELIEF_GRAD(y, H, FLY), RELIEF_GRAD(x, W, FLX), p);
        const float hsm = relief_hillshade(RELIEF_GRAD(y, H, FSY), RELIEF_GRAD(x, W, FSX), p);
#undef FLY
#undef FLX
#undef FSY
#undef FSX
        const float hs = powf(relief_clip01(0.75f * hl + 0.25f * hsm), 0.85f);
        float r = 0.f, g = 0.f, b = 0.f;
        if (colormap) {
            // base colour: terrain colormap of the unfilled land elevation; NaN argument -> the colormap's bad colour (0, 0, 0)
            const float land = is_nan ? e : (e > 0.f ? e : 0.f);
            float cm = relief_clip01(powf((land - vmin_f) / den, 0.7f));
            if (offset) cm = 0.25f + cm * 0.75f;
            if (!isnan(cm)) {
                float xi = cm * 256.f;
                if (xi == 256.f) xi = 255.f;
                int idx = (int)xi;
                idx = idx < 0 ? 0 : (idx > 255 ? 255 : idx);   // under / over colours are the first / last entries
                r = lut_s[idx * 3];
                g = lut_s[idx * 3 + 1];
                b = lut_s[idx * 3 + 2];
            }
        } else {
            r = ov.rgb[px * 3];
            g = ov.rgb[px * 3 + 1];
            b = ov.rgb[px * 3 + 2];
        }
        if constexpr (OVERLAY) {
            if (ov.biome) {   // np.where(clip(biome, 0, 30) > 0, palette[biome], base): on top of a caller's rgb too
                const int id = ov.biome[px];
                if (id > 0) {
                    const float* c = ov.palette + (id > 30 ? 30 : id) * 3;
                    r = c[0];
                    g = c[1];
                    b = c[2];
                }
            }
        }
        const float m = relief * (0.35f + 0.65f * hs) + omr;
        r = relief_clip01(r * m);
        g = relief_clip01(g * m);
        b = relief_clip01(b * m);
        if (is_nan) r = g = b = __builtin_nanf("");
        if constexpr (OVERLAY) {
            // river: 0.25 * shaded + 0.75 * (0.100, 0.450, 0.850), each product rounded to fp32, then one add; a NaN flow compares false,
            // a river on a NaN pixel stays NaN
            if (ov.flow && ov.flow[px] > ov.flow_threshold) {
                r = 0.25f * r + 0.75f * 0.100f;
                g = 0.25f * g + 0.75f * 0.450f;
                b = 0.25f * b + 0.75f * 0.850f;
            }
        }
        if (ef < 0.f) {   // ocean, on the filled elevation
            const float t = powf(relief_clip01(-ef / 10000.f), 0.7f), u = 1.f - t;
            r = u * 0.68f + t * 0.00f;
            g = u * 0.88f + t * 0.10f;
            b = u * 1.00f + t * 0.45f;
        }
        float* o = out + px * 3;
        o[0] = r;
        o[1] = g;
        o[2] = b;
    }
}
#undef RELIEF_GRAD

__host__ __device__ constexpr int relief_shade_lds_floats(int R) {
    return 2 * (RELIEF_P2_TY + 2) * (RELIEF_P2_TX + 2 + 2 * R) + 2 * (RELIEF_P2_TY + 2) * (RELIEF_P2_TX + 2) + 256 * 3 + 2 * (2 * RELIEF_MAX_RADIUS + 1);
}
__host__ __device__ constexpr int relief_blur_lds_floats(int R) { return (RELIEF_P1_ROWS + 2 * R) * RELIEF_P1_COLS + 2 * (2 * RELIEF_MAX_RADIUS + 1); }

}  // namespace td
