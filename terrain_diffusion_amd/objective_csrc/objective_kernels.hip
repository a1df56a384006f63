// Kernels of libtd_objective.so (include/td_objective.h): the forward half of the reference's training objective
// (terrain_diffusion/training/trainers/diffusion.py, training/dev_utils/noise_loss_curve.py, models/edm_unet.py:181-183) -- the per-item level
// table, the fused trigflow noising, the logvar head, the squared error per item and channel, the three loss forms, terrain as uint8 images.
//
// Arithmetic is restated in tests/_objective_twin.py; keep the two in step.  Contraction is off (and the library is built with
// -ffp-contract=off): every product and sum rounds on its own, as torch's CPU kernels do.  Every floating sum goes thread by thread in
// ascending order and then through a fixed tree in float64 (no floating-point atomic anywhere), so two runs give the same bits.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/td_objective.h"

namespace td {

constexpr int OB_THREADS = 256;
constexpr int OB_WAVES = OB_THREADS / 64;
static_assert(OB_WAVES == 4, "ob_block_sum adds four wave sums");

struct ObList {
    int n;
    int v[TD_OBJECTIVE_MAX_LIST];
};

// the fixed tree of a block: xor-shuffles inside a wave (every lane ends with the same bits), then the waves' sums pairwise; every thread
// must call it and every thread receives the sum
__device__ __forceinline__ double ob_block_sum(double v, double* wave_sums) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3]);
    __syncthreads();
    return s;
}

// ------------------------------------------------------------------------------------------------------------------------------ levels
// One block per item.  The std (mode 0 with channels) takes two float64 passes over the listed channels; thread 0 writes the row.
__global__ void __launch_bounds__(OB_THREADS) ob_levels_kernel(int mode, const float* __restrict__ in, float P_mean, float P_std, float sigma_data,
                                                               const float* __restrict__ images, int C, long long HW, ObList ch, float eps,
                                                               float* __restrict__ table) {
    __shared__ double wave_sums[OB_WAVES];
    const int n = blockIdx.x;
    const double sd = (double)sigma_data;
    double std64 = 0.0;
    if (mode == TD_OBJECTIVE_MODE_DRAW && ch.n > 0) {
        const float* __restrict__ img = images + (size_t)n * C * HW;
        const long long M = (long long)ch.n * HW;
        double s = 0.0;
        for (int k = 0; k < ch.n; ++k) {
            const float* __restrict__ p = img + (size_t)ch.v[k] * HW;
            for (long long i = threadIdx.x; i < HW; i += OB_THREADS) s += (double)p[i];
        }
        const double mean = ob_block_sum(s, wave_sums) / (double)M;
        double q = 0.0;
        for (int k = 0; k < ch.n; ++k) {
            const float* __restrict__ p = img + (size_t)ch.v[k] * HW;
            for (long long i = threadIdx.x; i < HW; i += OB_THREADS) {
                const double d = (double)p[i] - mean;
                q += d * d;
            }
        }
        std64 = sqrt(ob_block_sum(q, wave_sums) / (double)(M - 1));      // M = 1: 0 / 0 = NaN, as torch.std
    }
    if (threadIdx.x != 0) return;
    const double a = (double)in[n];
    double sigma;
    float t32;
    if (mode == TD_OBJECTIVE_MODE_T) {
        t32 = in[n];
        sigma = tan((double)t32) * sd;
    } else {
        sigma = mode == TD_OBJECTIVE_MODE_DRAW ? exp(a * (double)P_std + (double)P_mean) : a;
        if (mode == TD_OBJECTIVE_MODE_DRAW && ch.n > 0) {
            const double r = std64 / sd, e = (double)eps;
            sigma *= (r != r) ? r : (r > e ? r : e);                      // torch.maximum: a NaN propagates
        }
        t32 = (float)atan(sigma / sd);
    }
    const double t = (double)t32;
    float* __restrict__ row = table + (size_t)n * TD_OBJECTIVE_LEVEL_COLS;
    row[0] = (float)sigma;
    row[1] = t32;
    row[2] = (float)cos(t);
    row[3] = (float)sin(t);
    row[4] = (float)log(tan(t) / 8.0);
    row[5] = (float)std64;
}

// ------------------------------------------------------------------------------------------------------------------------------ noise
struct ObNoiseOut {
    float x, v;
};

__device__ __forceinline__ ObNoiseOut ob_noise_one(float img, float noise, float c, float s, float sd) {
    const float nz = noise * sd;
    const float a = c * img;
    const float b = s * nz;
    const float xt = a + b;
    const float p = c * nz;
    const float q = s * img;
    return {xt / sd, p - q};
}

// One thread per V consecutive elements of a plane of x (N, C + Cc, HW); V = 4 needs HW % 4 == 0 and 16-byte aligned bases (the host checks), so
// that a group of four never crosses a plane.  The grid is (blocks over the HW / V groups of a plane, C + Cc, min(N, 65535)): the channel and the
// item are block indices, no thread divides; the items beyond the grid's z extent are taken by the loop.
template <int V>
__global__ void __launch_bounds__(OB_THREADS) ob_noise_kernel(const float* __restrict__ images, const float* __restrict__ noise,
                                                              const float* __restrict__ cond, const float* __restrict__ table, int N, int C, int Cc,
                                                              unsigned HW, float sd, float* __restrict__ x, float* __restrict__ v) {
    const unsigned g = blockIdx.x * OB_THREADS + threadIdx.x;
    if (g >= HW / V) return;
    const unsigned p = g * V;
    const int ch = blockIdx.y;
    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        const size_t xo = ((size_t)n * (C + Cc) + ch) * HW + p;
        if (ch >= C) {
            const size_t co = ((size_t)n * Cc + (ch - C)) * HW + p;
            if (V == 4) *(float4*)(x + xo) = *(const float4*)(cond + co);
            else x[xo] = cond[co];
            continue;
        }
        const float c = table[(size_t)n * TD_OBJECTIVE_LEVEL_COLS + 2], s = table[(size_t)n * TD_OBJECTIVE_LEVEL_COLS + 3];
        const size_t io = ((size_t)n * C + ch) * HW + p;
        if (V == 4) {
            const float4 im = *(const float4*)(images + io), nz = *(const float4*)(noise + io);
            const ObNoiseOut r0 = ob_noise_one(im.x, nz.x, c, s, sd), r1 = ob_noise_one(im.y, nz.y, c, s, sd);
            const ObNoiseOut r2 = ob_noise_one(im.z, nz.z, c, s, sd), r3 = ob_noise_one(im.w, nz.w, c, s, sd);
            *(float4*)(x + xo) = make_float4(r0.x, r1.x, r2.x, r3.x);
            *(float4*)(v + io) = make_float4(r0.v, r1.v, r2.v, r3.v);
        } else {
            const ObNoiseOut r = ob_noise_one(images[io], noise[io], c, s, sd);
            x[xo] = r.x;
            v[io] = r.v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ logvar
// One wave per item: the engine's 'float' conditional input (csrc/small_kernels.hip emb_kernel) without mp_silu.
__global__ void __launch_bounds__(64) ob_logvar_kernel(const float* __restrict__ table, const float* __restrict__ freqs,
                                                       const float* __restrict__ phases, const float* __restrict__ weight, int K,
                                                       float* __restrict__ logvar) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const float xlv = table[(size_t)n * TD_OBJECTIVE_LEVEL_COLS + 4];
    float a = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float f = cosf(__fadd_rn(__fmul_rn(xlv, freqs[k]), phases[k])) * 1.41421356237309515f;
        a += weight[k] * f;
    }
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) logvar[n] = a;
}

// ------------------------------------------------------------------------------------------------------------------------------ sqerr
// One block per (n, c) plane.
__global__ void __launch_bounds__(OB_THREADS) ob_sqerr_kernel(const float* __restrict__ out, const float* __restrict__ v, long long HW, float sd,
                                                              double* __restrict__ S) {
    __shared__ double wave_sums[OB_WAVES];
    const size_t base = (size_t)blockIdx.x * HW;
    const float nsd = -sd;
    double s = 0.0;
    for (long long i = threadIdx.x; i < HW; i += OB_THREADS) {
        const float pred = nsd * out[base + i];
        const float d = pred - v[base + i];
        s += (double)d * (double)d;
    }
    s = ob_block_sum(s, wave_sums);
    if (threadIdx.x == 0) S[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------ loss
// One block.  Thread i takes the items i, i + 256, ... in order; the channel sums of an item run in ascending order.
__global__ void __launch_bounds__(OB_THREADS) ob_loss_kernel(const double* __restrict__ S, const float* __restrict__ logvar, int N, int C,
                                                             long long HW, float sigma_data, int form, ObList groups,
                                                             double* __restrict__ item_loss, double* __restrict__ loss64,
                                                             float* __restrict__ loss32) {
    __shared__ double wave_sums[OB_WAVES];
    const double sd2 = (double)sigma_data * (double)sigma_data, hw = (double)HW;
    double acc = 0.0;
    for (int n = threadIdx.x; n < N; n += OB_THREADS) {
        const double* __restrict__ row = S + (size_t)n * C;
        double item;
        if (form == TD_OBJECTIVE_LOSS_GROUPED) {
            double g = 0.0;
            int c = 0;
            for (int k = 0; k < groups.n; ++k) {
                double s = 0.0;
                for (int j = 0; j < groups.v[k]; ++j) s += row[c + j];
                c += groups.v[k];
                g += s / ((double)groups.v[k] * hw) / sd2;
            }
            item = g / (double)groups.n;
        } else {
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += row[c];
            const double m = s / ((double)C * hw);
            if (form == TD_OBJECTIVE_LOSS_WEIGHTED) {
                const double lv = (double)logvar[n];
                item = m / (exp(lv) * sd2) + lv;
            } else {
                item = m / sd2;
            }
        }
        item_loss[n] = item;
        acc += item;
    }
    const double mean = ob_block_sum(acc, wave_sums) / (double)N;
    if (threadIdx.x == 0) {
        loss64[0] = mean;
        loss32[0] = (float)mean;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ terrain_u8
// min / max of one item, one block per item: order-independent (min and max are exact); a NaN anywhere makes both NaN, as amin / amax
__global__ void __launch_bounds__(OB_THREADS) ob_minmax_kernel(const float* __restrict__ x, long long M, float* __restrict__ mm) {
    __shared__ float lo_s[OB_WAVES], hi_s[OB_WAVES];
    __shared__ int nan_s[OB_WAVES];
    const float* __restrict__ p = x + (size_t)blockIdx.x * M;
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (long long i = threadIdx.x; i < M; i += OB_THREADS) {
        const float v = p[i];
        bad |= (v != v);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        bad |= __shfl_xor(bad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        lo_s[threadIdx.x >> 6] = lo;
        hi_s[threadIdx.x >> 6] = hi;
        nan_s[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < OB_WAVES; ++w) {
            lo = fminf(lo, lo_s[w]);
            hi = fmaxf(hi, hi_s[w]);
            bad |= nan_s[w];
        }
        const float q = __builtin_nanf("");
        mm[2 * blockIdx.x] = bad ? q : lo;
        mm[2 * blockIdx.x + 1] = bad ? q : hi;
    }
}

__device__ __forceinline__ uint8_t ob_u8_one(float x, float mid, float range) {
    const float d = x - mid;
    const float q = d / range;
    const float h = q + 0.5f;
    float y = h * 255.f;
    if (!(y == y)) return 0;                             // NaN: the reference's conversion is undefined there
    y = y < 0.f ? 0.f : (y > 255.f ? 255.f : y);
    return (uint8_t)(int)y;
}

// One thread per V consecutive pixels of a plane of terrain (N, C, HW); V = 4 needs HW % 4 == 0, a 16-byte aligned input and a 4-byte aligned
// output.  The grid is (blocks over the HW / V groups of a plane, C, min(N, 65535)), as ob_noise_kernel's: no thread divides.
template <int V>
__global__ void __launch_bounds__(OB_THREADS) ob_u8_kernel(const float* __restrict__ x, const float* __restrict__ mm, int N, int C, unsigned HW,
                                                           uint8_t* __restrict__ out) {
    const unsigned g = blockIdx.x * OB_THREADS + threadIdx.x;
    if (g >= HW / V) return;
    const unsigned p = g * V;
    const int c = blockIdx.y;
    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        const float lo = mm[2 * (size_t)n], hi = mm[2 * (size_t)n + 1];
        const float r0 = hi - lo;
        const float range = (r0 != r0) ? r0 : (r0 > 255.f ? r0 : 255.f);       // torch.maximum(range, 255): a NaN propagates
        const float sum = lo + hi;
        const float mid = sum / 2.f;
        const size_t io = ((size_t)n * C + c) * HW + p;
        if (V == 4) {
            const float4 t = *(const float4*)(x + io);
            uchar4 b;
            b.x = ob_u8_one(t.x, mid, range);
            b.y = ob_u8_one(t.y, mid, range);
            b.z = ob_u8_one(t.z, mid, range);
            b.w = ob_u8_one(t.w, mid, range);
            for (int r = 0; r < 3; ++r) *(uchar4*)(out + ((size_t)n * 3 * C + (size_t)r * C + c) * HW + p) = b;
        } else {
            const uint8_t b = ob_u8_one(x[io], mid, range);
            for (int r = 0; r < 3; ++r) out[((size_t)n * 3 * C + (size_t)r * C + c) * HW + p] = b;
        }
    }
}

}  // namespace td
