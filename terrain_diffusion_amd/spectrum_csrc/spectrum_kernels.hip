// Kernels of libtd_spectrum.so (include/td_spectrum.h): the device half of the reference's beauty score
// (terrain_diffusion/data/preprocessing/beauty_score.py) -- the head of calculate_beauty_score (laplacian_decode, sign(d) d^2, the share of
// pixels <= 0, the clamp, torch.std) and analyze_terrain_frequency (fft2, log|F|, the radial bin means).
//
// Arithmetic is restated in tests/_beauty_twin.py; keep the two in step.  Contraction is off (and the library is built with
// -ffp-contract=off): the decode rounds every fp32 product and sum of its bilinear expression on its own, as td_dataset_residual does; a
// butterfly is four fp32 products and six sums, each rounded once; the moments and the bin sums square and add in float64 without fusing.
// Every kernel is order-independent: counts use integer atomics, every float64 sum goes through a fixed tree whose shape is a function of
// the sizes alone (no floating-point atomic anywhere), so two runs give the same bits.
//
// The FFT is radix-2 decimation in time in LDS, twiddles from a host-built table (cos and sin in float64, rounded once to fp32):
//   row pass     one block per PAIR of real rows a, b: z = a + i b goes through one complex transform of length W, and
//                A[k] = (Z[k] + conj Z[W - k]) / 2, B[k] = (Z[k] - conj Z[W - k]) / (2 i) for k = 0 .. W / 2 (the halvings are exact);
//   column pass  one block per tile of SP_TILE / H neighbouring columns of the half spectrum (W / 2 + 1 columns), transformed in place in
//                LDS; its epilogue writes the half spectrum and / or log|F| with the second half of each row by Hermitian symmetry.
// A flat plane comes out with exact zeros off the DC coefficient: the first butterfly of equal values subtracts them.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace td {

constexpr int SP_THREADS = 256;
constexpr int SP_MAX_N = 4096;                           // td_spectrum.h TD_SPECTRUM_MAX_SIDE: the longest transform
constexpr int SP_TW = SP_MAX_N / 2;                      // twiddles of the table: exp(-2 pi i k / 4096), k = 0 .. 2047
constexpr int SP_TILE = 8192;                            // complex values of one column tile: 64 KiB of LDS, two columns of 4096
constexpr int SP_MAX_COLS = 16;                          // columns of a tile at most: 128 bytes of a row
constexpr int SP_SUM_BLOCKS = 512;                       // partial sums per plane at most (the width of the fixed reduction tree)
constexpr int SP_BIN_THREADS = 128;                      // the bin sums keep one float64 slot per thread and bin in LDS: bins KiB
constexpr int SP_MAX_BINS = 64;                          // td_spectrum.h TD_SPECTRUM_MAX_BINS

// ------------------------------------------------------------------------------------------------------------------------------ FFT
__device__ __forceinline__ int sp_bitrev(int v, int bits) { return (int)(__brev((unsigned)v) >> (32 - bits)); }

// `count` independent transforms of length n = 2^bits, transform q at s[q * n ..], input in bit-reversed order, output in natural order.
// Stage t joins pairs `half` = 2^(t-1) apart with the twiddle exp(-2 pi i j / 2^t) = tw[j * (4096 >> t)].  Every thread of the block calls it.
__device__ __forceinline__ void sp_fft_lds(float2* __restrict__ s, int n, int bits, int count, const float2* __restrict__ tw) {
    const int flies = count * (n >> 1);
    for (int t = 1; t <= bits; ++t) {
        const int half = 1 << (t - 1);
        __syncthreads();
        for (int i = threadIdx.x; i < flies; i += SP_THREADS) {
            const int q = i >> (bits - 1), f = i & ((n >> 1) - 1);
            const int j = f & (half - 1);
            const int at = q * n + ((f >> (t - 1)) << t) + j;
            const float2 w = tw[j * (SP_MAX_N >> t)];
            const float2 a = s[at], b = s[at + half];
            const float br = b.x * w.x - b.y * w.y, bi = b.x * w.y + b.y * w.x;
            s[at] = make_float2(a.x + br, a.y + bi);
            s[at + half] = make_float2(a.x - br, a.y - bi);
        }
    }
    __syncthreads();
}

// grid (H / 2, B): rows 2 p and 2 p + 1 of plane b -> their half spectra, (B, H, W / 2 + 1) interleaved complex
__global__ void __launch_bounds__(SP_THREADS) sp_fft_rows_kernel(const float* __restrict__ x, int H, int W, int bits,
                                                                 const float2* __restrict__ tw, float2* __restrict__ half) {
    __shared__ float2 s[SP_MAX_N];
    const int Wh = W / 2 + 1;
    const size_t row = (size_t)blockIdx.y * H + 2 * blockIdx.x;
    const float* __restrict__ a = x + row * W;
    for (int i = threadIdx.x; i < W; i += SP_THREADS) s[sp_bitrev(i, bits)] = make_float2(a[i], a[W + i]);
    sp_fft_lds(s, W, bits, 1, tw);
    float2* __restrict__ oa = half + row * Wh;
    for (int k = threadIdx.x; k < Wh; k += SP_THREADS) {
        const float2 z = s[k], c = s[(W - k) & (W - 1)];
        oa[k] = make_float2((z.x + c.x) * 0.5f, (z.y - c.y) * 0.5f);
        oa[Wh + k] = make_float2((z.y + c.y) * 0.5f, (c.x - z.x) * 0.5f);
    }
}

// grid (ceil((W / 2 + 1) / cols), B), cols = min(16, SP_TILE / H): columns k0 .. k0 + cols - 1 of plane b's row spectra, transformed along H in
// place (a tile's columns belong to its block alone).  half_out and logf may each be NULL.  log|F| = 0.5 log(re^2 + im^2) in float64, rounded
// once to fp32: no overflow at 1e10, no flush at 1e-30, -inf at an exact zero; position (r, k) also fills ((H - r) % H, W - k) for 0 < k < W / 2.
__global__ void __launch_bounds__(SP_THREADS) sp_fft_cols_kernel(const float2* half_in, int H, int W, int bits, int cols,
                                                                 const float2* __restrict__ tw, float2* half_out, float* __restrict__ logf) {
    __shared__ float2 s[SP_TILE];
    const int Wh = W / 2 + 1;
    const int k0 = blockIdx.x * cols, nc = min(cols, Wh - k0);
    const size_t plane = (size_t)blockIdx.y * H;
    for (int i = threadIdx.x; i < H * cols; i += SP_THREADS) {
        const int r = i / cols, c = i - r * cols;
        // a column beyond the spectrum is transformed as zeros and never written
        s[c * H + sp_bitrev(r, bits)] = c < nc ? half_in[(plane + r) * Wh + k0 + c] : make_float2(0.f, 0.f);
    }
    sp_fft_lds(s, H, bits, cols, tw);
    for (int i = threadIdx.x; i < H * cols; i += SP_THREADS) {
        const int r = i / cols, c = i - r * cols, k = k0 + c;
        if (c >= nc) continue;
        const float2 f = s[c * H + r];
        if (half_out) half_out[(plane + r) * Wh + k] = f;
        if (logf) {
            const double re = (double)f.x, im = (double)f.y;
            const float v = (float)(0.5 * log(re * re + im * im));
            logf[(plane + r) * W + k] = v;
            if (k > 0 && k < W / 2) logf[(plane + ((H - r) & (H - 1))) * W + (W - k)] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ sums
// the fixed tree of a block of `waves` waves: xor-shuffles inside a wave, then the waves' sums in wave order; every thread must call it;
// thread 0 holds the sum
__device__ __forceinline__ double sp_block_sum(double v, double* wave_sums, int waves) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < waves; ++k) s += wave_sums[k];
    __syncthreads();
    return s;
}

__device__ __forceinline__ int sp_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------------------------------------ decode
// torch's upsample_bilinear2d source index, align_corners=False, in fp32: td_dataset_residual's tap arithmetic (dataset_kernels.hip ds_taps)
__device__ __forceinline__ void sp_taps(int dst, float scale, int n_in, int& i0, int& i1, float& l0, float& l1) {
    const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    i0 = min((int)src, n_in - 1);
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}

// grid (blocks, B), blocks a function of H W alone.  d = residual + up(low), v = sign(d) d^2 (np.sign(d) * d**2: NaN stays NaN), the number
// of v <= 0 to nonpos[b] (zeroed by the caller; one integer atomic per wave), out = v < 0 ? 0 : v, and the block's float64 sum of out to
// part[b * gridDim.x + block]: thread by thread in ascending order, then the block's tree.
__global__ void __launch_bounds__(SP_THREADS) sp_decode_kernel(const float* __restrict__ low, const float* __restrict__ res, int H, int W, int h,
                                                               int w, float sy, float sx, float* __restrict__ out, int* __restrict__ nonpos,
                                                               double* __restrict__ part) {
    __shared__ double wave_sums[SP_THREADS / 64];
    const size_t n = (size_t)H * W;
    const float* __restrict__ lo = low + (size_t)blockIdx.y * h * w;
    const float* __restrict__ rs = res + (size_t)blockIdx.y * n;
    float* __restrict__ o = out + (size_t)blockIdx.y * n;
    double acc = 0.0;
    int count = 0;
    for (size_t i = (size_t)blockIdx.x * SP_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * SP_THREADS) {
        const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
        int i0, i1, j0, j1;
        float wy0, wy1, wx0, wx1;
        sp_taps(y, sy, h, i0, i1, wy0, wy1);
        sp_taps(x, sx, w, j0, j1, wx0, wx1);
        const float* __restrict__ top = lo + (size_t)i0 * w;
        const float* __restrict__ bot = lo + (size_t)i1 * w;
        const float up = wy0 * (wx0 * top[j0] + wx1 * top[j1]) + wy1 * (wx0 * bot[j0] + wx1 * bot[j1]);
        const float d = rs[i] + up;
        const float sq = d * d;
        float v = d > 0.f ? sq : (d < 0.f ? -sq : d);    // sign(d) * d^2; a zero stays a zero, a NaN a NaN
        count += v <= 0.f;
        v = v < 0.f ? 0.f : v;
        o[i] = v;
        acc += (double)v;
    }
    count = sp_wave_sum(count);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(&nonpos[blockIdx.y], count);
    const double sum = sp_block_sum(acc, wave_sums, SP_THREADS / 64);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// the second pass over the written plane: the squares of out - mean[b] in float64, the same walk and tree
__global__ void __launch_bounds__(SP_THREADS) sp_centred_kernel(const float* __restrict__ x, size_t n, const double* __restrict__ mean,
                                                                double* __restrict__ part) {
    __shared__ double wave_sums[SP_THREADS / 64];
    const float* __restrict__ p = x + (size_t)blockIdx.y * n;
    const double m = mean[blockIdx.y];
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * SP_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * SP_THREADS) {
        const double d = (double)p[i] - m;
        acc += d * d;
    }
    const double sum = sp_block_sum(acc, wave_sums, SP_THREADS / 64);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// one block per plane: the `blocks` partial sums through the same tree.  centred = 0: mean = sum / n; centred = 1: m2 = sum and
// std = fp32(sqrt(m2 / (n - 1))), the unbiased one, rounded once
__global__ void __launch_bounds__(SP_THREADS) sp_moments_final_kernel(const double* __restrict__ part, int blocks, double n, int centred,
                                                                      double* __restrict__ mean, double* __restrict__ m2, float* __restrict__ std) {
    __shared__ double wave_sums[SP_THREADS / 64];
    double acc = 0.0;
    for (int b = threadIdx.x; b < blocks; b += SP_THREADS) acc += part[(size_t)blockIdx.x * blocks + b];
    const double s = sp_block_sum(acc, wave_sums, SP_THREADS / 64);
    if (threadIdx.x == 0) {
        if (!centred) {
            mean[blockIdx.x] = s / n;
        } else {
            m2[blockIdx.x] = s;
            std[blockIdx.x] = (float)sqrt(s / (n - 1.0));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ radial bins
// grid (blocks, B), blocks a function of H W alone; dynamic LDS: bins * SP_BIN_THREADS float64 slots, slot[bin * 128 + thread].  A thread adds
// the values of its positions (ascending) into its own slot of their bin -- a position of bin 255 into none --, then every bin's 128 slots go
// through the block's tree: part[(b * gridDim.x + block) * bins + bin].  Infinities and NaNs are added as IEEE arithmetic has them.
// counts[b * bins + bin] (zeroed by the caller) receives the number of positions: integer atomics.
__global__ void __launch_bounds__(SP_BIN_THREADS) sp_bins_partial_kernel(const float* __restrict__ logf, const unsigned char* __restrict__ map,
                                                                         int n, int bins, double* __restrict__ part, int* __restrict__ counts) {
    extern __shared__ double slot[];
    __shared__ double wave_sums[SP_BIN_THREADS / 64];
    __shared__ int cnt[SP_MAX_BINS];
    const int tid = threadIdx.x;
    for (int b = 0; b < bins; ++b) slot[b * SP_BIN_THREADS + tid] = 0.0;
    if (tid < bins) cnt[tid] = 0;
    __syncthreads();
    const float* __restrict__ p = logf + (size_t)blockIdx.y * n;
    for (int i = blockIdx.x * SP_BIN_THREADS + tid; i < n; i += gridDim.x * SP_BIN_THREADS) {
        const int b = map[i];
        if (b < bins) {
            slot[b * SP_BIN_THREADS + tid] += (double)p[i];
            atomicAdd(&cnt[b], 1);
        }
    }
    __syncthreads();
    for (int b = 0; b < bins; ++b) {
        const double s = sp_block_sum(slot[b * SP_BIN_THREADS + tid], wave_sums, SP_BIN_THREADS / 64);
        if (tid == 0) part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * bins + b] = s;
    }
    if (tid < bins && cnt[tid]) atomicAdd(&counts[blockIdx.y * bins + tid], cnt[tid]);
}

// one block per plane: per bin the `blocks` partial sums through the same tree; mean = fp32(sum / count), 0 for an empty bin
__global__ void __launch_bounds__(SP_BIN_THREADS) sp_bins_final_kernel(const double* __restrict__ part, int blocks, int bins,
                                                                       const int* __restrict__ counts, float* __restrict__ means) {
    __shared__ double wave_sums[SP_BIN_THREADS / 64];
    for (int b = 0; b < bins; ++b) {
        double acc = 0.0;
        for (int k = threadIdx.x; k < blocks; k += SP_BIN_THREADS) acc += part[((size_t)blockIdx.x * blocks + k) * bins + b];
        const double s = sp_block_sum(acc, wave_sums, SP_BIN_THREADS / 64);
        if (threadIdx.x == 0) {
            const int c = counts[blockIdx.x * bins + b];
            means[blockIdx.x * bins + b] = c > 0 ? (float)(s / (double)c) : 0.f;
        }
    }
}

}  // namespace td
