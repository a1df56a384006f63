// Kernels of libtd_batch.so (include/td_batch.h): the device half of the reference's training items
// (terrain_diffusion/training/datasets/h5_latents_dataset.py, h5_decoder_terrain_dataset.py, h5_autoencoder_dataset.py) -- dihedral views of
// resident planes, the latent reparameterisation in both precisions, the conditioning image of 32 x 32 block statistics and the conditioning
// vector built from it.
//
// Arithmetic is restated in tests/_train_data_twin.py; keep the two in step.  Contraction is off (and the library is built with
// -ffp-contract=off): every product and sum rounds on its own, as torch's and NumPy's CPU kernels do.  Every kernel is order-independent:
// the order statistics come from an exact radix select whose LDS counters are integers, and every floating sum goes thread by thread in
// ascending order and then through a fixed tree (no floating-point atomic anywhere), so two runs give the same bits.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/td_batch.h"

namespace td {

constexpr int BA_THREADS = 256;
constexpr int BA_WAVES = BA_THREADS / 64;
constexpr int BA_BLOCK = TD_BATCH_HALO;                  // side of a block of the cond image
constexpr int BA_ITEMS = BA_BLOCK * BA_BLOCK;            // 1024 values per block
constexpr int BA_PER_THREAD = BA_ITEMS / BA_THREADS;     // 4
constexpr int BA_RANK = 51;                              // floor(fl(1023) fl(0.05))
static_assert(BA_WAVES == 4 && BA_PER_THREAD == 4, "ba_block_sum adds four wave sums; a thread of the cond image holds four values");

struct BaItem {
    int group, i, j, t, li, lj;
};

// item n of the table, or group = -1 when its group or transform is out of range
__device__ __forceinline__ BaItem ba_item(const int* __restrict__ items, int n, int G) {
    const int* __restrict__ f = items + (size_t)n * TD_BATCH_ITEM_FIELDS;
    BaItem it{f[0], f[1], f[2], f[3], f[4], f[5]};
    if (it.group < 0 || it.group >= G || it.t < 0 || it.t > 7) it.group = -1;
    return it;
}

// The position (ar, ac) of the untransformed window that the view rot90(flip?(A), k) of shape (h, w) shows at (r, c); t = 4 flip + k.
// A has the shape (h, w) for an even k and (w, h) for an odd one.
__device__ __forceinline__ void ba_unview(int t, int h, int w, int r, int c, int& ar, int& ac) {
    const int k = t & 3;
    const int hA = (k & 1) ? w : h, wA = (k & 1) ? h : w;
    int br, bc;
    if (k == 0) { br = r; bc = c; }
    else if (k == 1) { br = c; bc = wA - 1 - r; }
    else if (k == 2) { br = hA - 1 - r; bc = wA - 1 - c; }
    else { br = hA - 1 - c; bc = r; }
    ar = br;
    ac = (t >> 2) ? wA - 1 - bc : bc;
}

// the fixed tree of a block: xor-shuffles inside a wave (every lane ends with the same bits), then the waves' sums pairwise; every thread
// must call it and every thread receives the sum
__device__ __forceinline__ double ba_block_sum(double v, double* wave_sums) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3]);
    __syncthreads();
    return s;
}

// ------------------------------------------------------------------------------------------------------------------------------ views
// One thread per output element.
__global__ void __launch_bounds__(BA_THREADS) ba_views_kernel(const td_batch_group* __restrict__ groups, int G, const int* __restrict__ items,
                                                              long long total, int plane, int origin, int offset, int h, int w, int affine,
                                                              float a, float b, float c, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * BA_THREADS + threadIdx.x;
    if (e >= total) return;
    const int col = (int)(e % w);
    const long long rest = e / w;
    const int row = (int)(rest % h), n = (int)(rest / h);
    const BaItem it = ba_item(items, n, G);
    float v = __builtin_nanf("");
    if (it.group >= 0) {
        const td_batch_group g = groups[it.group];
        const float* __restrict__ src = plane == TD_BATCH_PLANE_LOWFREQ ? g.lowfreq : plane == TD_BATCH_PLANE_LOWRES_EXACT ? g.lowres_exact : g.residual;
        const int S = plane == TD_BATCH_PLANE_RESIDUAL ? g.residual_side : g.side;
        int ar, ac;
        ba_unview(it.t, h, w, row, col, ar, ac);
        const long long pr = (long long)(origin ? it.i : it.li) + offset + ar, pc = (long long)(origin ? it.j : it.lj) + offset + ac;
        if (src && pr >= 0 && pr < S && pc >= 0 && pc < S) v = src[(size_t)pr * S + pc];
    }
    if (affine) {
        const float d = v - a;
        const float q = d / b;
        v = q * c;
    }
    out[e] = v;
}

// ------------------------------------------------------------------------------------------------------------------------------ latents
// e = fp16(exp(fp16(0.5 v))): the product is exact in fp32; the exponential is taken in float64 and rounded to fp32 and then to half, which
// is one rounding of the float64 value wherever it is not within 2^-24 of a half rounding midpoint.
__device__ __forceinline__ _Float16 ba_half_std(_Float16 logvar) {
    const _Float16 hv = (_Float16)((float)logvar * 0.5f);
    return (_Float16)(float)exp((double)(float)hv);
}

// mode 0, one thread per output element: fp32 from the promoted halves
__global__ void __launch_bounds__(BA_THREADS) ba_latents_f32_kernel(const td_batch_group* __restrict__ groups, int G, const int* __restrict__ items,
                                                                    long long total, int lc, int h, int w, const float* __restrict__ noise,
                                                                    const float* __restrict__ mean, const float* __restrict__ std,
                                                                    float sigma_data, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * BA_THREADS + threadIdx.x;
    if (e >= total) return;
    const int q = (int)(e % w);
    long long rest = e / w;
    const int r = (int)(rest % h);
    rest /= h;
    const int ch = (int)(rest % lc), n = (int)(rest / lc);
    const BaItem it = ba_item(items, n, G);
    float v = 0.f;
    if (it.group >= 0) {
        const td_batch_group g = groups[it.group];
        const long long S = g.side, pr = (long long)it.i + r, pc = (long long)it.j + q;
        if (g.latent && pr >= 0 && pr < S && pc >= 0 && pc < S) {
            const _Float16* __restrict__ slab = (const _Float16*)g.latent + (size_t)it.t * 2 * lc * S * S;
            const _Float16 m = slab[((size_t)ch * S + pr) * S + pc], lv = slab[((size_t)(lc + ch) * S + pr) * S + pc];
            const float s = noise[e] * (float)ba_half_std(lv);
            const float x = s + (float)m;
            const float d = x - mean[ch];
            const float z = d / std[ch];
            v = z * sigma_data;
        }
    }
    out[e] = v;
}

// mode 1, one thread per eight output pixels of a row (one 16-byte store): half arithmetic, each operation rounded to half
__global__ void __launch_bounds__(BA_THREADS) ba_latents_f16_kernel(const td_batch_group* __restrict__ groups, int G, const int* __restrict__ items,
                                                                    long long total, int lc, int h, int w, const _Float16* __restrict__ noise,
                                                                    _Float16* __restrict__ out) {
    const long long e = (long long)blockIdx.x * BA_THREADS + threadIdx.x;      // over (n, ch, 8 h rows, w)
    if (e >= total) return;
    const int q = (int)(e % w);
    long long rest = e / w;
    const int orow = (int)(rest % (8 * h));
    rest /= 8 * h;
    const int ch = (int)(rest % lc), n = (int)(rest / lc);
    const int r = orow >> 3;
    const BaItem it = ba_item(items, n, G);
    _Float16 v = (_Float16)0.f;
    if (it.group >= 0) {
        const td_batch_group g = groups[it.group];
        const long long S = g.side, pr = (long long)it.i + r, pc = (long long)it.j + q;
        if (g.latent && pr >= 0 && pr < S && pc >= 0 && pc < S) {
            const _Float16* __restrict__ slab = (const _Float16*)g.latent + (size_t)it.t * 2 * lc * S * S;
            const _Float16 m = slab[((size_t)ch * S + pr) * S + pc], lv = slab[((size_t)(lc + ch) * S + pr) * S + pc];
            const _Float16 nz = noise[(((size_t)n * lc + ch) * h + r) * w + q];
            const _Float16 p = (_Float16)((float)nz * (float)ba_half_std(lv));
            v = (_Float16)((float)p + (float)m);
        }
    }
    union { _Float16 h8[8]; uint4 u; } pack;
    for (int k = 0; k < 8; ++k) pack.h8[k] = v;
    *(uint4*)(out + e * 8) = pack.u;             // e * 8 halves: 16-byte aligned whenever out is
}

// ------------------------------------------------------------------------------------------------------------------------------ cond image
// an order-preserving key of a non-NaN float: a < b as floats exactly when key(a) < key(b), with -0 below +0
__device__ __forceinline__ unsigned ba_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ba_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct BaSelect {
    int hist[256];
    int wave_tot[BA_WAVES];
    int digit, rank, count_le;
    unsigned min_gt;
};

// The keys of ranks `rank` and `rank + 1` (0-based, ascending) among the BA_ITEMS keys of a block, four per thread: a radix select from the
// top byte down -- a 256-bin histogram of the keys that still match the prefix, its prefix sums, the bin the rank falls in --, then the
// number of keys <= the selected one and the least key above it.  Every thread must call it; every thread receives both keys.
__device__ __forceinline__ void ba_select2(const unsigned (&key)[BA_PER_THREAD], int rank, BaSelect* s, unsigned& k0, unsigned& k1) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        s->hist[tid] = 0;
        __syncthreads();
        for (int e = 0; e < BA_PER_THREAD; ++e)
            if ((key[e] & mask) == prefix) atomicAdd(&s->hist[(key[e] >> shift) & 255u], 1);
        __syncthreads();
        const int cnt = s->hist[tid];
        int incl = cnt;
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) s->wave_tot[wave] = incl;
        __syncthreads();
        for (int wv = 0; wv < wave; ++wv) incl += s->wave_tot[wv];
        const int excl = incl - cnt;
        if (excl <= rank && rank < incl) { s->digit = tid; s->rank = rank - excl; }      // exactly one thread: the sums end at the match count > rank
        __syncthreads();
        prefix |= (unsigned)s->digit << shift;
        mask |= 255u << shift;
        rank = s->rank;
        __syncthreads();
    }
    if (tid == 0) { s->count_le = 0; s->min_gt = 0xffffffffu; }
    __syncthreads();
    int le = 0;
    unsigned gt = 0xffffffffu;
    for (int e = 0; e < BA_PER_THREAD; ++e) {
        if (key[e] <= prefix) ++le;
        else gt = min(gt, key[e]);
    }
    atomicAdd(&s->count_le, le);
    atomicMin(&s->min_gt, gt);
    __syncthreads();
    k0 = prefix;
    k1 = s->count_le >= BA_RANK + 2 ? prefix : s->min_gt;
}

// One workgroup per (item, block of the view), all five source planes.  Value idx = 32 r + c of the block is held by thread idx % 256 as
// its (idx / 256)-th value; a thread adds its four values in that order in float64, then the block's tree.
__global__ void __launch_bounds__(BA_THREADS) ba_cond_image_kernel(const td_batch_group* __restrict__ groups, int G, const int* __restrict__ items,
                                                                   int crop, float dropout_p, const float* __restrict__ u_drop, float max_noise,
                                                                   const float* __restrict__ u_noise, const float* __restrict__ z_mean,
                                                                   const float* __restrict__ z_p5, const float* __restrict__ norm_mean,
                                                                   const float* __restrict__ norm_std, int raw, float* __restrict__ out) {
    __shared__ double wave_sums[BA_WAVES];
    __shared__ BaSelect sel;
    const int tid = threadIdx.x;
    const int V = crop + 2 * TD_BATCH_HALO, g = V / BA_BLOCK;
    const int blk = blockIdx.x % (g * g), n = blockIdx.x / (g * g);
    const int by = blk / g, bx = blk - by * g;
    const BaItem it = ba_item(items, n, G);                // block-uniform
    const float nan = __builtin_nanf("");
    float lowres[BA_PER_THREAD];
    double sums[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int has_nan = 0;
    td_batch_group grp{};
    if (it.group >= 0) grp = groups[it.group];
    const long long S = grp.side;
    for (int e = 0; e < BA_PER_THREAD; ++e) {
        const int idx = tid + BA_THREADS * e;
        int ar, ac;
        ba_unview(it.t, V, V, by * BA_BLOCK + (idx >> 5), bx * BA_BLOCK + (idx & 31), ar, ac);
        const long long pr = (long long)it.li - TD_BATCH_HALO + ar, pc = (long long)it.lj - TD_BATCH_HALO + ac;
        const bool inside = it.group >= 0 && pr >= 0 && pr < S && pc >= 0 && pc < S;
        const size_t at = inside ? (size_t)pr * S + pc : 0;
        const float v = inside && grp.lowres_exact ? grp.lowres_exact[at] : nan;
        lowres[e] = v;
        has_nan |= isnan(v);
        sums[0] += (double)v;
        for (int p = 0; p < 4; ++p) sums[1 + p] += (double)(inside && grp.climate ? grp.climate[(size_t)p * S * S + at] : nan);
    }
    for (int p = 0; p < 5; ++p) sums[p] = ba_block_sum(sums[p], wave_sums);
    has_nan = __syncthreads_or(has_nan);                   // block-uniform from here
    unsigned k0 = 0, k1 = 0;
    if (!has_nan) {
        unsigned key[BA_PER_THREAD];
        for (int e = 0; e < BA_PER_THREAD; ++e) key[e] = ba_key(lowres[e]);
        ba_select2(key, BA_RANK, &sel, k0, k1);
    }
    if (tid != 0) return;
    float mean = (float)(sums[0] / (double)BA_ITEMS);
    float p5 = nan;
    if (!has_nan) {
        const float r = 1023.0f * 0.05f;                   // fl(1023) fl(0.05), rounded once
        const float t = r - (float)BA_RANK;
        const float a = ba_unkey(k0), b = ba_unkey(k1);
        const float d = b - a;
        const float dt = d * t;
        p5 = a + dt;
    }
    float mask = 1.0f - (isnan(mean) ? 1.0f : 0.0f);
    const size_t cell = ((size_t)n * g + by) * g + bx;
    if (u_drop) {
        mask = mask * (u_drop[cell] > dropout_p ? 1.0f : 0.0f);
        if (mask == 0.0f) { mean = nan; p5 = nan; }
    }
    if (u_noise) {
        const float s = u_noise[n] * max_noise;
        const float zm = z_mean[cell] * s, zp = z_p5[cell] * s;
        mean = mean + zm;
        p5 = p5 + zp;
    }
    float stack[TD_BATCH_COND_CHANNELS] = {mean, p5, 0.f, 0.f, 0.f, 0.f, mask};
    for (int p = 0; p < 4; ++p) stack[2 + p] = (float)(sums[1 + p] / (double)BA_ITEMS);
    if (!raw) {
        for (int ch = 0; ch < 2; ++ch) {                   // nan_to_num(nan = mean_ch): infinities go to the largest finite values
            const float v = stack[ch];
            stack[ch] = isnan(v) ? norm_mean[ch] : isinf(v) ? copysignf(FLT_MAX, v) : v;
        }
        for (int ch = 0; ch < TD_BATCH_COND_CHANNELS; ++ch) {
            const float d = stack[ch] - norm_mean[ch];
            stack[ch] = d / norm_std[ch];
        }
    }
    for (int ch = 0; ch < TD_BATCH_COND_CHANNELS; ++ch) out[(((size_t)n * TD_BATCH_COND_CHANNELS + ch) * g + by) * g + bx] = stack[ch];
}

// ------------------------------------------------------------------------------------------------------------------------------ cond vector
struct BaFactors {
    float f[6];
};

// One thread per output element (n, slot).
__global__ void __launch_bounds__(BA_THREADS) ba_cond_vector_kernel(const float* __restrict__ cond_img, int N, int g, const float* __restrict__ hist,
                                                                    const float* __restrict__ noise_level, const float* __restrict__ z_replace,
                                                                    float sqrt12, BaFactors fac, float* __restrict__ out, int* __restrict__ nan_flags) {
    const int e = blockIdx.x * BA_THREADS + threadIdx.x;
    if (e >= N * TD_BATCH_COND_LEN) return;
    const int n = e / TD_BATCH_COND_LEN, slot = e - n * TD_BATCH_COND_LEN;
    const int c0 = g / 2 - 2;
    const float* __restrict__ img = cond_img + (size_t)n * TD_BATCH_COND_CHANNELS * g * g;
    auto at = [&](int ch, int r, int c) { return img[((size_t)ch * g + r) * g + c]; };
    float v;
    if (slot < 32 || (slot >= 36 && slot < 52)) {
        const int part = slot < 16 ? 0 : slot < 32 ? 1 : 3;
        const int k = slot < 32 ? slot & 15 : slot - 36;
        v = at(part == 3 ? 6 : part, c0 + (k >> 2), c0 + (k & 3)) * fac.f[part];
    } else if (slot < 36) {
        const int ch = 2 + (slot - 32), r = c0 + 1;
        const float s01 = at(ch, r, r) + at(ch, r, r + 1);
        const float s2 = s01 + at(ch, r + 1, r);
        const float s3 = s2 + at(ch, r + 1, r + 1);
        float m = s3 / 4.0f;
        const bool bad = isnan(m);
        nan_flags[n * 4 + (slot - 32)] = bad ? 1 : 0;
        if (bad && z_replace) m = z_replace[n * 4 + (slot - 32)];
        v = m * fac.f[2];
    } else if (slot < 57) {
        v = hist[n * 5 + (slot - 52)] * fac.f[4];
    } else {
        const float d = noise_level[n] - 0.5f;
        const float s = d * sqrt12;
        v = s * fac.f[5];
    }
    out[e] = v;
}

}  // namespace td
