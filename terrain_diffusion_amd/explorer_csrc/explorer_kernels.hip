// Kernels of libtd_explorer.so (include/td_explorer.h): the per-request tails of the reference's terrain explorer (inference/explorer/
// server.py) and of its random sampler's land-tile search (inference/random_sampler.py).
//
// Arithmetic is restated in tests/_explorer_twin.py; keep the two in step.  Contraction is off (and the library is built with
// -ffp-contract=off): every product and sum rounds on its own, as NumPy does.  Divisions are taken in float64 and rounded once: the correctly
// rounded fp32 quotient whatever the fp32 flags (a double quotient of two floats rounds to fp32 without a double-rounding error).
// Minima and maxima: a float that is not NaN maps to an order-preserving uint32 key, and both extremes are integer atomicMax on words that
// start at 0 (the minimum as the maximum of ~key), so the result does not depend on the order of the atomics.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace td {

constexpr int EX_THREADS = 256;
constexpr int EX_WAVES = EX_THREADS / 64;
constexpr int EX_MAX_FILTERS = 8;
constexpr unsigned EX_REDUCE_BLOCKS = 1024;   // grid-stride cap of the reducing kernels

__device__ __forceinline__ float ex_div(float a, float b) { return (float)((double)a / (double)b); }

// total order of the non-NaN floats (-inf < ... < -0 < +0 < ... < +inf) as uint32; no non-NaN value maps to 0 or to 0xffffffff
__device__ __forceinline__ unsigned ex_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ex_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// words[0] = max of ~key, words[1] = max of key; both 0 (which decodes to NaN) when nothing was accumulated
__device__ __forceinline__ float ex_decode_min(unsigned w) { return ex_unkey(~w); }
__device__ __forceinline__ float ex_decode_max(unsigned w) { return ex_unkey(w); }

__device__ __forceinline__ void ex_accumulate(float v, unsigned& lo, unsigned& hi) {
    if (!isnan(v)) {
        const unsigned k = ex_key(v);
        lo = max(lo, ~k);
        hi = max(hi, k);
    }
}

// block-wide maximum of (lo, hi) -> one atomicMax pair per workgroup on words[0 .. 2); every thread of the block calls it
__device__ __forceinline__ void ex_block_max(unsigned lo, unsigned hi, unsigned* __restrict__ words) {
    __shared__ unsigned red[2 * EX_WAVES];
    for (int o = 32; o > 0; o >>= 1) {
        lo = max(lo, (unsigned)__shfl_xor((int)lo, o, 64));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o, 64));
    }
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) { red[2 * (tid >> 6)] = lo; red[2 * (tid >> 6) + 1] = hi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < EX_WAVES; ++w) { lo = max(lo, red[2 * w]); hi = max(hi, red[2 * w + 1]); }
        if (lo) atomicMax(words, lo);
        if (hi) atomicMax(words + 1, hi);
    }
}

// np.sign(v) * np.square(v) in fp32
__device__ __forceinline__ float ex_signed_square(float v) {
    const float s = v > 0.f ? 1.f : (v < 0.f ? -1.f : (v == 0.f ? 0.f : v));
    return s * (v * v);
}

// ---- channels.  Grid (min(ceil(n / 256), 1024), C): plane blockIdx.y, grid-stride over its n = H W pixels.  words (C, 2) or null.
__global__ __launch_bounds__(EX_THREADS) void ex_channels_kernel(const float* __restrict__ sums, int C, long long n, int n_signed_sq, int add_eps,
                                                                 float eps, float* __restrict__ out, unsigned* __restrict__ words) {
    const int c = blockIdx.y;
    const float* __restrict__ num = sums + (size_t)c * n;
    const float* __restrict__ den = sums + (size_t)C * n;
    float* __restrict__ dst = out + (size_t)c * n;
    unsigned lo = 0u, hi = 0u;
    for (long long p = (long long)blockIdx.x * EX_THREADS + threadIdx.x; p < n; p += (long long)gridDim.x * EX_THREADS) {
        const float w = den[p];
        float v = ex_div(num[p], add_eps ? w + eps : w);
        if (c < n_signed_sq) v = ex_signed_square(v);
        dst[p] = v;
        ex_accumulate(v, lo, hi);
    }
    if (words) ex_block_max(lo, hi, words + 2 * c);   // grid-uniform branch
}

// words (count, 2) -> minmax (count, 2) floats; one block of 64 threads, count <= 8
__global__ void ex_decode_kernel(const unsigned* __restrict__ words, int count, float* __restrict__ minmax) {
    const int t = threadIdx.x;
    if (t < 2 * count) minmax[t] = (t & 1) ? ex_decode_max(words[t]) : ex_decode_min(words[t]);
}

// ---- colorize
__device__ __forceinline__ float ex_display(float x, int log1p_on) {
    if (!log1p_on) return x;
    const float m = x > 0.f ? x : (x <= 0.f ? 0.f : x);   // np.maximum(x, 0): NaN stays NaN
    return (float)log1p((double)m);
}

// NaN-ignoring range of the displayed field.  Grid min(ceil(n / 256), 1024).
__global__ __launch_bounds__(EX_THREADS) void ex_range_kernel(const float* __restrict__ field, long long n, int log1p_on, unsigned* __restrict__ words) {
    unsigned lo = 0u, hi = 0u;
    for (long long p = (long long)blockIdx.x * EX_THREADS + threadIdx.x; p < n; p += (long long)gridDim.x * EX_THREADS)
        ex_accumulate(ex_display(field[p], log1p_on), lo, hi);
    ex_block_max(lo, hi, words);
}

struct ExColorArgs {
    const float* field;
    long long n;
    int log1p_on;
    int has_range;
    double vmin, vmax;              // has_range
    const unsigned* words;          // !has_range: the range words of ex_range_kernel
    const float* lut;               // 256 x 3
    int n_filters;
    const float* planes[EX_MAX_FILTERS];
    float lo[EX_MAX_FILTERS], hi[EX_MAX_FILTERS];
    int use_lo[EX_MAX_FILTERS], use_hi[EX_MAX_FILTERS];
    uchar4* out;
    float* range_out;               // 2 floats or null
};

// imsave's quantisation of a channel after np.clip(c, 0, 1); a NaN channel (relief only) is written as 0
__device__ __forceinline__ unsigned char ex_quant(float c) {
    if (isnan(c)) return 0;
    c = c < 0.f ? 0.f : (c > 1.f ? 1.f : c);
    return (unsigned char)(c * 255.0f);
}

// Grid ceil(n / 256): one pixel per thread.
__global__ __launch_bounds__(EX_THREADS) void ex_color_kernel(ExColorArgs a) {
    const long long p = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
    double vmin, vmax;
    float fmin, fmax;
    if (a.has_range) {
        vmin = a.vmin; vmax = a.vmax;
        fmin = (float)vmin; fmax = (float)vmax;
    } else {
        fmin = ex_decode_min(a.words[0]); fmax = ex_decode_max(a.words[1]);
        vmin = (double)fmin;
        vmax = fmin == fmax ? vmin + 1.0 : (double)fmax;
    }
    if (p == 0 && a.range_out) { a.range_out[0] = fmin; a.range_out[1] = fmax; }
    if (p >= a.n) return;
    const float d = ex_display(a.field[p], a.log1p_on);
    const float t = (float)((double)d - vmin);
    const float x = (float)((double)t / (vmax - vmin));
    float xa = x * 256.0f;
    float r = 0.f, g = 0.f, b = 0.f, alpha = 0.f;
    if (!isnan(xa)) {
        if (xa == 256.0f) xa = 255.0f;
        const int idx = xa < 0.f ? 0 : (xa >= 256.0f ? 255 : (int)xa);
        r = a.lut[3 * idx]; g = a.lut[3 * idx + 1]; b = a.lut[3 * idx + 2];
        alpha = 1.f;
    }
    bool pass = true;
    for (int f = 0; f < a.n_filters; ++f) {
        const float v = a.planes[f][p];
        if (a.use_lo[f] && !(v >= a.lo[f])) pass = false;
        if (a.use_hi[f] && !(v <= a.hi[f])) pass = false;
    }
    if (!pass) { r = r * 0.3f; g = g * 0.3f; b = b * 0.3f; }
    a.out[p] = make_uchar4(ex_quant(r), ex_quant(g), ex_quant(b), ex_quant(alpha));
}

// ---- quantize: (n, 3) fp32 -> (n, 4) uint8, alpha 255
__global__ __launch_bounds__(EX_THREADS) void ex_quantize_kernel(const float* __restrict__ rgb, long long n, uchar4* __restrict__ out) {
    const long long p = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
    if (p >= n) return;
    const float* s = rgb + 3 * (size_t)p;
    out[p] = make_uchar4(ex_quant(s[0]), ex_quant(s[1]), ex_quant(s[2]), 255);
}

// ---- raw: out as uint16 words: [0, n) the int16 elevation, [n, 3 n) the temperature's fp32 words as two halves each (n may be odd)
__global__ __launch_bounds__(EX_THREADS) void ex_raw_kernel(const float* __restrict__ elev, const float* __restrict__ temp, long long n,
                                                            uint16_t* __restrict__ out) {
    const long long p = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
    if (p >= n) return;
    const float e = floorf(elev[p]);
    const int v = isnan(e) ? 0 : (e < -32768.f ? -32768 : (e > 32767.f ? 32767 : (int)e));
    out[p] = (uint16_t)(int16_t)v;
    if (temp) {
        const unsigned u = __float_as_uint(temp[p]);
        out[n + 2 * p] = (uint16_t)(u & 0xffffu);
        out[n + 2 * p + 1] = (uint16_t)(u >> 16);
    }
}

// ---- land tiles.  Pass 1: rows[i][j] = number of land cells in row i, columns [j - half, j + half), for half <= j < W - half (other j: unused).
__global__ __launch_bounds__(EX_THREADS) void ex_land_rows_kernel(const float* __restrict__ elev, int H, int W, int half, uint16_t* __restrict__ rows) {
    const long long p = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
    if (p >= (long long)H * W) return;
    const int i = (int)(p / W), j = (int)(p % W);
    if (j < half || j >= W - half) return;
    const float* r = elev + (size_t)i * W;
    int c = 0;
    for (int x = j - half; x < j + half; ++x) c += r[x] > 0.f ? 1 : 0;   // j - half >= 0, j + half <= W - 1 + 1
    rows[p] = (uint16_t)c;
}

// Pass 2: the column sum of rows over [i - half, i + half), the fp32 mean, the comparison; flags[p] and the number of valid positions of
// each block of 256 consecutive flat indices.
__global__ __launch_bounds__(EX_THREADS) void ex_land_flags_kernel(const uint16_t* __restrict__ rows, int H, int W, int half, float cells, double min_frac,
                                                                   uint8_t* __restrict__ flags, unsigned* __restrict__ block_counts) {
    __shared__ unsigned wave_counts[EX_WAVES];
    const long long p = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
    bool valid = false;
    if (p < (long long)H * W) {
        const int i = (int)(p / W), j = (int)(p % W);
        if (i >= half && i < H - half && j >= half && j < W - half) {
            int c = 0;
            for (int y = i - half; y < i + half; ++y) c += rows[(size_t)y * W + j];
            const float m = ex_div((float)c, cells);
            valid = (double)m >= min_frac;
        }
        flags[p] = valid ? 1 : 0;
    }
    const unsigned long long ballot = __ballot(valid);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) wave_counts[tid >> 6] = (unsigned)__popcll(ballot);
    __syncthreads();
    if (tid == 0) {
        unsigned s = 0;
        for (int w = 0; w < EX_WAVES; ++w) s += wave_counts[w];
        block_counts[blockIdx.x] = s;
    }
}

// One block of 1024 threads: block_counts[0 .. nb) -> exclusive prefix sums in place, total -> *out_count.
__global__ __launch_bounds__(1024) void ex_land_scan_kernel(unsigned* __restrict__ block_counts, int nb, int32_t* __restrict__ out_count) {
    __shared__ unsigned wave_sums[16];
    __shared__ unsigned carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0u;
    __syncthreads();
    for (int base = 0; base < nb; base += 1024) {
        const int k = base + tid;
        const unsigned v = k < nb ? block_counts[k] : 0u;
        unsigned incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = (unsigned)__shfl_up((int)incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wave_sums[wave] = incl;
        __syncthreads();
        unsigned before = carry;
        for (int w = 0; w < wave; ++w) before += wave_sums[w];
        if (k < nb) block_counts[k] = before + incl - v;
        __syncthreads();
        if (tid == 1023) carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) *out_count = (int32_t)carry;
}

// Scatter: the valid positions of each block, in index order, to out_idx[offset of the block ...].
__global__ __launch_bounds__(EX_THREADS) void ex_land_scatter_kernel(const uint8_t* __restrict__ flags, long long n, const unsigned* __restrict__ block_offsets,
                                                                     long long capacity, int32_t* __restrict__ out_idx) {
    __shared__ unsigned wave_counts[EX_WAVES];
    const long long p = (long long)blockIdx.x * EX_THREADS + threadIdx.x;
    const bool valid = p < n && flags[p] != 0;
    const unsigned long long ballot = __ballot(valid);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (lane == 0) wave_counts[wave] = (unsigned)__popcll(ballot);
    __syncthreads();
    if (valid) {
        unsigned at = block_offsets[blockIdx.x];
        for (int w = 0; w < wave; ++w) at += wave_counts[w];
        at += (unsigned)__popcll(ballot & ((1ull << lane) - 1ull));
        if ((long long)at < capacity) out_idx[at] = (int32_t)p;   // at < capacity by construction; the guard keeps a wrong count inside the buffer
    }
}

}  // namespace td
