// Kernels of libtd_dataset.so (include/td_dataset.h): the device half of the reference's dataset preparation, the tail of
// process_single_file_base (terrain_diffusion/data/preprocessing/elevation_dataset.py:231-301) -- the void fill towards a low-resolution
// base, the signed square root, the r x r block median, the residual of laplacian_encode (data/laplacian_encoder.py:63-91), the land counts
// per sub-chunk -- and the chunk summary calculate_stats_welford (data/preprocessing/calculate_stds.py:7-71) accumulates.
//
// Arithmetic is restated in tests/_dataset_twin.py; keep the two in step.  Contraction is off (and the library is built with
// -ffp-contract=off): the void fill rounds one float64 product once, the residual rounds every fp32 product and sum of its bilinear
// expression on its own, the moments square and add in float64 without fusing.  Every kernel is order-independent: distances are integers,
// the median ranks by counting with an index tie-break, counts use integer atomics, and the float64 sums go through a fixed tree (no
// floating-point atomic anywhere), so two runs give the same bits.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace td {

constexpr int DS_THREADS = 256;
constexpr int DS_MAX_RADIUS = 64;                        // td_dataset.h TD_DATASET_MAX_RADIUS
constexpr int DS_BAND = 128;                             // rows one block of the column pass sweeps (plus `radius` rows of halo on either side)
constexpr int DS_UNROLL = 8;                             // rows a column sweep keeps in flight
constexpr int DS_ROW_TILE = DS_THREADS + 2 * (DS_MAX_RADIUS - 1);   // column distances the row pass stages: its 256 columns and radius - 1 either side
constexpr int DS_MED_ITEMS = 1024;                       // values one block of the median holds: 32 x 32, or 1024 / r^2 neighbouring blocks
constexpr int DS_MOM_BLOCKS = 512;                       // partial sums per plane at most (the width of the fixed reduction tree)

__device__ __forceinline__ int ds_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------------------------------------ void fill
// Pass 1, one thread per column and band of DS_BAND rows (neighbouring threads read neighbouring columns of a row: coalesced):
// g[r, c] = min(radius, vertical distance from (r, c) to the nearest valid pixel of column c), 0 on a valid pixel.  Distances of `radius`
// and more are all the same to the fill, so a sweep starts `radius` rows outside its band and needs nothing from further away: the bands
// are independent.  Down sweep: the nearest valid row at or above; up sweep: the nearest below, where nearer.  DS_UNROLL rows are loaded
// before the carried distance is updated, so the loads of a sweep overlap.  The number of voids goes to *voids (zeroed by the caller), one
// integer atomic per wave.
__global__ void __launch_bounds__(DS_THREADS) ds_void_columns_kernel(const float* __restrict__ dem, int H, int W, int radius,
                                                                     unsigned char* __restrict__ g, int* __restrict__ voids) {
    const int c = blockIdx.x * DS_THREADS + threadIdx.x;
    const int r0 = blockIdx.y * DS_BAND, r1 = min(H, r0 + DS_BAND);      // the band [r0, r1)
    int count = 0;
    if (c < W) {
        int d = radius;                                                   // distance to the nearest valid pixel above the row to come, capped
        for (int rb = max(0, r0 - radius); rb < r1; rb += DS_UNROLL) {
            float v[DS_UNROLL];
#pragma unroll
            for (int k = 0; k < DS_UNROLL; ++k) v[k] = rb + k < r1 ? dem[(size_t)(rb + k) * W + c] : 0.f;
#pragma unroll
            for (int k = 0; k < DS_UNROLL; ++k) {
                const int r = rb + k;
                if (r < r1) {
                    const bool hole = isnan(v[k]);
                    d = hole ? min(d + 1, radius) : 0;
                    if (r >= r0) {
                        g[(size_t)r * W + c] = (unsigned char)d;
                        count += hole;
                    }
                }
            }
        }
        d = radius;
        for (int rb = min(H, r1 + radius) - 1; rb >= r0; rb -= DS_UNROLL) {
            float v[DS_UNROLL];
            unsigned char up[DS_UNROLL];
#pragma unroll
            for (int k = 0; k < DS_UNROLL; ++k) {
                const int r = rb - k;
                v[k] = (r >= r1) ? dem[(size_t)r * W + c] : 0.f;         // halo: the DEM itself (another block writes g there)
                up[k] = (r >= r0 && r < r1) ? g[(size_t)r * W + c] : 0;  // band: this thread's own down sweep, 0 on a valid pixel
            }
#pragma unroll
            for (int k = 0; k < DS_UNROLL; ++k) {
                const int r = rb - k;
                if (r >= r0) {
                    const bool hole = r >= r1 ? isnan(v[k]) : up[k] != 0;
                    d = hole ? min(d + 1, radius) : 0;
                    if (r < r1 && d < (int)up[k]) g[(size_t)r * W + c] = (unsigned char)d;
                }
            }
        }
    }
    count = ds_wave_sum(count);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(voids, count);
}

__device__ __forceinline__ float ds_signed_sqrt(float v) { return copysignf(sqrtf(fabsf(v)), v); }

// Pass 2, one thread per pixel of a row segment of DS_THREADS columns.  A valid pixel passes through.  A void (r, c) takes
// d2 = min over |dx| < radius of dx^2 + g[r, c + dx]^2, the exact squared Euclidean distance to the nearest valid pixel wherever that is
// below radius^2 (a capped g contributes radius^2 or more, and so does every column further away); its own column bounds the search
// further: |dx| > g[r, c] cannot improve on dx = 0.  The stored value is fp32((double)base * alpha), alpha = sqrt((double)d2) / radius in
// float64 for d2 < radius^2 and 1 otherwise.  The squared column distances of the segment and radius - 1 columns either side are staged
// in LDS.  signed_sqrt maps every stored value v to sign(v) sqrtf(|v|).
__global__ void __launch_bounds__(DS_THREADS) ds_void_rows_kernel(const float* __restrict__ dem, const float* __restrict__ base,
                                                                  const unsigned char* __restrict__ g, int H, int W, int radius,
                                                                  int signed_sqrt, float* __restrict__ out) {
    __shared__ int sq[DS_ROW_TILE];
    const int tid = threadIdx.x;
    const int r = blockIdx.y, c0 = blockIdx.x * DS_THREADS, c = c0 + tid;
    const size_t row = (size_t)r * W;
    float v = 0.f;
    bool hole = false;
    if (c < W) {
        v = dem[row + c];
        hole = isnan(v);
    }
    if (__syncthreads_or(hole)) {                         // block-uniform
        const int reach = radius - 1, first = c0 - reach, width = DS_THREADS + 2 * reach;
        for (int k = tid; k < width; k += DS_THREADS) {
            const int cc = first + k;
            int d = radius;                               // outside the image: no valid pixel
            if (cc >= 0 && cc < W) d = g[row + cc];
            sq[k] = d * d;
        }
        __syncthreads();
        if (hole) {
            const int own = tid + reach;                  // this pixel's slot
            int best = sq[own];
            const int gown = (int)g[row + c];             // <= radius
            const int span = min(reach, gown);
            for (int dx = 1; dx <= span; ++dx) {
                const int dd = dx * dx;
                best = min(best, dd + min(sq[own - dx], sq[own + dx]));
            }
            double alpha = 1.0;
            if (best < radius * radius) alpha = sqrt((double)best) / (double)radius;
            v = (float)((double)base[row + c] * alpha);
        }
    }
    if (c < W) out[row + c] = signed_sqrt ? ds_signed_sqrt(v) : v;
}

// ------------------------------------------------------------------------------------------------------------------------------ block median
// One block per row of output blocks and group of G = max(1, DS_MED_ITEMS / r^2) neighbouring output blocks: the r x G r tile is read row by
// row (contiguous) into LDS, grouped per output block.  Each value's rank is the number of values of its block that are smaller, or equal
// and earlier in the block: a permutation of 0 .. r^2 - 1 whatever the order of the visits.  Ranks (r^2 - 1) / 2 and r^2 / 2 are the
// middle values: the median is the one for odd r^2, fp32(a + b) * 0.5f for even r^2 (np.median of float32; a zero median is +0 there, since
// its mean is a sum that starts at +0).  A block that holds a NaN gives NaN (its ranks mean nothing and are not used).
__global__ void __launch_bounds__(DS_THREADS) ds_block_median_kernel(const float* __restrict__ x, int W, int r, int Wb, int G,
                                                                     float* __restrict__ out) {
    __shared__ float val[DS_MED_ITEMS];
    __shared__ float mid[DS_MED_ITEMS][2];                // [group][lower, upper middle]; G <= DS_MED_ITEMS
    __shared__ int has_nan[DS_MED_ITEMS];
    const int tid = threadIdx.x;
    const int n = r * r;
    const int b0 = blockIdx.x * G;                        // first output block of the group, in a row of Wb
    const int groups = min(G, Wb - b0);
    const int items = groups * n, tile_w = groups * r;
    const float* __restrict__ src = x + (size_t)blockIdx.y * r * W + (size_t)b0 * r;
    for (int i = tid; i < groups; i += DS_THREADS) { has_nan[i] = 0; mid[i][0] = 0.f; mid[i][1] = 0.f; }
    for (int i = tid; i < items; i += DS_THREADS) {
        const int ty = i / tile_w, tx = i - ty * tile_w;  // tile row, tile column: consecutive threads read consecutive addresses
        const int gi = tx / r, ex = tx - gi * r;
        val[gi * n + ty * r + ex] = src[(size_t)ty * W + tx];
    }
    __syncthreads();
    const int lo = (n - 1) / 2, hi = n / 2;
    for (int i = tid; i < items; i += DS_THREADS) {
        const int gi = i / n, e = i - gi * n;
        const float v = val[i];
        if (isnan(v)) { has_nan[gi] = 1; continue; }      // every writer stores the same 1
        const float* __restrict__ u = val + gi * n;
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (u[j] < v) || (u[j] == v && j < e);
        if (rank == lo) mid[gi][0] = v;
        if (rank == hi) mid[gi][1] = v;
    }
    __syncthreads();
    for (int i = tid; i < groups; i += DS_THREADS) {
        float m = mid[i][0] + 0.f;                        // np.median takes the mean of the middle value(s), and that sum starts at +0: -0 -> +0
        if (lo != hi) m = (m + mid[i][1]) * 0.5f;
        if (has_nan[i]) m = __builtin_nanf("");
        out[(size_t)blockIdx.y * Wb + b0 + i] = m;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ residual
// torch's upsample_bilinear2d source index, align_corners=False, in fp32 as composition.bilinear_taps spells it: scale = fp32(n_in) /
// fp32(n_out); src = max(scale * (dst + 0.5f) - 0.5f, 0); i0 = min(int(src), n_in - 1); i1 = i0 + (i0 < n_in - 1); l1 = src - i0; l0 = 1 - l1
__device__ __forceinline__ void ds_taps(int dst, float scale, int n_in, int& i0, int& i1, float& l0, float& l1) {
    const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    i0 = min((int)src, n_in - 1);
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}

__device__ __forceinline__ float ds_up(const float* __restrict__ top, const float* __restrict__ bot, float wy0, float wy1, int x, float sx,
                                       int w) {
    int j0, j1;
    float wx0, wx1;
    ds_taps(x, sx, w, j0, j1, wx0, wx1);
    return wy0 * (wx0 * top[j0] + wx1 * top[j1]) + wy1 * (wx0 * bot[j0] + wx1 * bot[j1]);
}

// out = x - up(low), four neighbouring pixels of a row per thread: one 16-byte load and store where `vec` (W a multiple of 4 and both
// buffers 16-byte aligned), element-wise otherwise.  The upsampled plane is never written; low (h, w) is read through the caches.  A thread
// reads its own pixels of x before it writes them: out may alias x.
__global__ void __launch_bounds__(DS_THREADS) ds_residual_kernel(const float* x, const float* __restrict__ low, int H, int W, int h, int w,
                                                                 float sy, float sx, int vec, float* out) {
    const int x0 = 4 * (blockIdx.x * DS_THREADS + threadIdx.x), y = blockIdx.y;
    if (x0 >= W) return;
    int i0, i1;
    float wy0, wy1;
    ds_taps(y, sy, h, i0, i1, wy0, wy1);
    const float* __restrict__ top = low + (size_t)i0 * w;
    const float* __restrict__ bot = low + (size_t)i1 * w;
    const size_t at = (size_t)y * W + x0;
    if (vec) {                                            // W % 4 == 0: x0 + 4 <= W
        float4 v = *reinterpret_cast<const float4*>(x + at);
        v.x = v.x - ds_up(top, bot, wy0, wy1, x0, sx, w);
        v.y = v.y - ds_up(top, bot, wy0, wy1, x0 + 1, sx, w);
        v.z = v.z - ds_up(top, bot, wy0, wy1, x0 + 2, sx, w);
        v.w = v.w - ds_up(top, bot, wy0, wy1, x0 + 3, sx, w);
        *reinterpret_cast<float4*>(out + at) = v;
    } else {
        for (int k = 0; k < 4 && x0 + k < W; ++k) out[at + k] = x[at + k] - ds_up(top, bot, wy0, wy1, x0 + k, sx, w);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ land counts
// grid.y = sub-chunk ch * num_chunks + cw of side (sh, sw); the blocks of a sub-chunk share its pixels; counts (zeroed by the caller)
// receives the number of low > 0 (false for NaN), one integer atomic per wave.
__global__ void __launch_bounds__(DS_THREADS) ds_land_counts_kernel(const float* __restrict__ low, int w, int num_chunks, int sh, int sw,
                                                                    int* __restrict__ counts) {
    const int ch = blockIdx.y / num_chunks, cw = blockIdx.y - ch * num_chunks;
    const int px = sh * sw;                               // < 2^28
    int count = 0;
    for (int i = blockIdx.x * DS_THREADS + threadIdx.x; i < px; i += gridDim.x * DS_THREADS) {
        const int yy = i / sw, xx = i - yy * sw;
        count += low[(size_t)(ch * sh + yy) * w + cw * sw + xx] > 0.f;
    }
    count = ds_wave_sum(count);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(&counts[blockIdx.y], count);
}

// ------------------------------------------------------------------------------------------------------------------------------ moments
// usable[i] = 1 where no plane holds a NaN at position i (C > 1; one plane tests its own values instead)
__global__ void __launch_bounds__(DS_THREADS) ds_usable_kernel(const float* __restrict__ x, int C, long long n, unsigned char* __restrict__ usable) {
    const long long i = (long long)blockIdx.x * DS_THREADS + threadIdx.x;
    if (i >= n) return;
    bool ok = true;
    for (int c = 0; c < C; ++c) ok &= !isnan(x[(size_t)c * n + i]);
    usable[i] = ok;
}

// the fixed tree of a block: xor-shuffles inside a wave, then the waves' sums in wave order; every thread must call it; thread 0 holds the sum
__device__ __forceinline__ double ds_block_sum(double v, double* wave_sums) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < DS_THREADS / 64; ++k) s += wave_sums[k];
    __syncthreads();
    return s;
}

// One pass over plane c = blockIdx.y: block b sums the usable positions b * 256 + t, stepping gridDim.x * 256, thread by thread in
// ascending order and then through the block's tree: part[c * gridDim.x + b].  centred = 0: the values, and for plane 0 the number of
// usable positions (part_count[b]); centred = 1: the squares of value - mean[c] in float64.  The grid is a function of n alone, so the
// order of every addition is fixed.
__global__ void __launch_bounds__(DS_THREADS) ds_moments_partial_kernel(const float* __restrict__ x, const unsigned char* __restrict__ usable,
                                                                        long long n, int centred, const double* __restrict__ mean,
                                                                        double* __restrict__ part, long long* __restrict__ part_count) {
    __shared__ double wave_sums[DS_THREADS / 64];
    __shared__ double wave_counts[DS_THREADS / 64];
    const int c = blockIdx.y;
    const float* __restrict__ plane = x + (size_t)c * n;
    const double m = centred ? mean[c] : 0.0;
    double acc = 0.0;
    long long cnt = 0;
    for (long long i = (long long)blockIdx.x * DS_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * DS_THREADS) {
        const float v = plane[i];
        const bool ok = usable ? usable[i] != 0 : !isnan(v);
        if (ok) {
            const double d = (double)v - m;
            acc += centred ? d * d : d;
            ++cnt;
        }
    }
    const double s = ds_block_sum(acc, wave_sums);
    if (threadIdx.x == 0) part[(size_t)c * gridDim.x + blockIdx.x] = s;
    if (!centred && c == 0) {                             // block-uniform; counts are far below 2^53: exact in float64
        const double k = ds_block_sum((double)cnt, wave_counts);
        if (threadIdx.x == 0) part_count[blockIdx.x] = (long long)k;
    }
}

// One block per plane: the B partial sums through the same tree.  centred = 0 writes the count (plane 0) and mean = sum / count;
// centred = 1 writes m2 = sum.  count = 0 leaves 0 in both.
__global__ void __launch_bounds__(DS_THREADS) ds_moments_final_kernel(const double* __restrict__ part, const long long* __restrict__ part_count,
                                                                      int B, int centred, long long* __restrict__ out_count,
                                                                      double* __restrict__ out) {
    __shared__ double wave_sums[DS_THREADS / 64];
    __shared__ double wave_counts[DS_THREADS / 64];
    const int c = blockIdx.x;
    double acc = 0.0, cnt = 0.0;
    for (int b = threadIdx.x; b < B; b += DS_THREADS) {
        acc += part[(size_t)c * B + b];
        cnt += (double)part_count[b];
    }
    const double s = ds_block_sum(acc, wave_sums);
    const double k = ds_block_sum(cnt, wave_counts);
    if (threadIdx.x == 0) {
        if (!centred && c == 0) *out_count = (long long)k;
        out[c] = k > 0.0 ? (centred ? s : s / k) : 0.0;
    }
}

}  // namespace td
