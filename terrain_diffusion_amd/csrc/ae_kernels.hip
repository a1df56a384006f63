// Kernels around the EDMAutoencoder graphs (gfx950): input normalisation + dihedral views, latent head, reparameterisation, decode finish.
// terrain_diffusion/models/edm_autoencoder.py:107-158, terrain_diffusion/data/preprocessing/build_encoded_dataset.py:68-94.
// All of them move a few bytes per pixel once; the convs between them do the work.
#include "td_device.h"

namespace td {

// How the encoder input is read from the caller's fp32 NCHW source: (x - mean) / std, and for the dihedral form 8 views per source image.
struct AeSrc {
    const float* x;            // (n_src, C, H, W)
    int C, H, W;
    int dihedral;              // 0: image n = source n; 1: image n = view (n & 7) of source n >> 3 (needs H == W)
    float mean, std;
};

// Source pixel of pixel (i, j) of view k = 4 * flip + r: torch.rot90(torch.flip(x, [-1]) if flip else x, k=r, dims=[-2, -1])[i][j]
// (build_encoded_dataset.py:75-81).  rot90: r=1 -> in[j][S-1-i], r=2 -> in[S-1-i][S-1-j], r=3 -> in[S-1-j][i].
__device__ __forceinline__ void ae_view_src(int view, int H, int W, int i, int j, int* a, int* b) {
    const int r = view & 3;
    int y = i, x = j;
    if (r == 1) { y = j; x = W - 1 - i; }
    else if (r == 2) { y = H - 1 - i; x = W - 1 - j; }
    else if (r == 3) { y = H - 1 - j; x = i; }
    if (view & 4) x = W - 1 - x;
    *a = y; *b = x;
}

// one subtraction, then one true division, each rounded once in fp32 (build_encoded_dataset.py:69 on a float32 array)
__device__ __forceinline__ float ae_norm(float v, float mean, float std) {
    float d = __fsub_rn(v, mean);
    asm("" : "+v"(d));
    return __fdiv_rn(d, std);
}

__device__ __forceinline__ float ae_src_value(const AeSrc& s, int n, int c, int i, int j) {
    int a = i, b = j, src = n;
    if (s.dihedral) { src = n >> 3; ae_view_src(n & 7, s.H, s.W, i, j, &a, &b); }
    return ae_norm(s.x[(((size_t)src * s.C + c) * s.H + a) * s.W + b], s.mean, s.std);
}

// fp32 NCHW source -> the encoder's NHWC input in the storage type, ones channel at index C (edm_unet.py:168), n_out images.
// One thread per output pixel, consecutive threads on consecutive output pixels: the NHWC writes are those of prep_input_kernel.  The source is read by
// plain gather: for the odd rotations consecutive threads read one source COLUMN (stride W floats), uncoalesced, but a chunk is 1 MB, read 8 times and
// L2-resident after the first view, and the whole kernel moves ~1/1000 of what the convs behind it do.  A staged 32 x 32 LDS transpose would coalesce the
// source side too and was not built.  mean = 0, std = 1, no views: (x - 0) / 1 = x, the bits of prep_input_kernel with scale 1.
template <typename T>
__global__ void ae_prep_input_kernel(AeSrc s, T* __restrict__ xin, int n_out, int cstride) {
    const size_t HW = (size_t)s.H * s.W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_out * HW) return;
    const int n = (int)(i / HW), p = (int)(i % HW), y = p / s.W, x = p % s.W;
    for (int c = 0; c < s.C; ++c) xin[i * cstride + c] = (T)ae_src_value(s, n, c, y, x);
    xin[i * cstride + s.C] = (T)1.f;
}

struct AeDirect {
    int n;                     // len(direct_skips) <= 8
    int ch[8];                 // channel of the model input / output each one carries
};

// Encoder F (NHWC fp32, stride `fstride`, 2L channels at h x w) -> means, logvars (n, L + D, h, w) fp32 and, optionally, cat(means, logvars) as fp16
// (round-to-nearest-even: build_encoded_dataset.py:87,94).  edm_autoencoder.py:108-123: the first L channels are F's two halves; direct channel d of the
// means is the mean of the s x s block of input channel ch[d] (adaptive_avg_pool2d with H = s h), read from the fp32 source through the same
// normalisation and view as the encoder input -- never from the 16-bit staged input; of the logvars, -20.  Fixed summation order: each row of the block
// left to right, then the row sums top to bottom, then one division by s * s.  One thread per latent pixel.
__global__ void ae_latent_head_kernel(const float* __restrict__ F, int fstride, AeSrc s, AeDirect dir, int n_out, int L, int h, int w, int sdown,
                                      float* __restrict__ means, float* __restrict__ logvars, _Float16* __restrict__ packed) {
    const size_t hw = (size_t)h * w;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_out * hw) return;
    const int n = (int)(i / hw), p = (int)(i % hw), oy = p / w, ox = p % w;
    const int LD = L + dir.n;
    for (int c = 0; c < LD; ++c) {
        float m, lv;
        if (c < L) { m = F[i * fstride + c]; lv = F[i * fstride + L + c]; }
        else {
            const int ch = dir.ch[c - L];
            float tot = 0.f;
            for (int dy = 0; dy < sdown; ++dy) {
                float row = 0.f;
                for (int dx = 0; dx < sdown; ++dx) row += ae_src_value(s, n, ch, oy * sdown + dy, ox * sdown + dx);
                tot += row;
            }
            m = tot / (float)(sdown * sdown);
            lv = -20.f;
        }
        const size_t o = ((size_t)n * LD + c) * hw + p;
        means[o] = m; logvars[o] = lv;
        if (packed) {
            packed[((size_t)n * 2 * LD + c) * hw + p] = (_Float16)m;
            packed[((size_t)n * 2 * LD + LD + c) * hw + p] = (_Float16)lv;
        }
    }
}

// z = means + eps * exp(0.5 * logvars)  (edm_autoencoder.py:128-130): the product and the sum are rounded separately, as torch's two ops are
__global__ void ae_postencode_kernel(const float* __restrict__ means, const float* __restrict__ logvars, const float* __restrict__ eps, float* __restrict__ z, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float pr = eps[i] * expf(logvars[i] * 0.5f);
    asm("" : "+v"(pr));
    z[i] = means[i] + pr;
}

// Decoder F (NHWC fp32, stride `fstride`) -> (n, Co, H, W) fp32.  Output channel ch[d] is the nearest-neighbour upsampling of latent channel L + d of z
// (edm_autoencoder.py:146-153: mask * direct + (1 - mask) * out, an exact copy for finite decoder outputs); then, with denorm, y * std + mean as a
// multiply and an add that are rounded one after the other (torch's two ops).  One thread per output pixel.
__global__ void ae_decode_finish_kernel(const float* __restrict__ F, int fstride, const float* __restrict__ z, AeDirect dir, int n, int Co, int L, int H, int W,
                                        int sup, int denorm, float std, float mean, float* __restrict__ out) {
    const size_t HW = (size_t)H * W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * HW) return;
    const int b = (int)(i / HW), p = (int)(i % HW), y = p / W, x = p % W;
    const int h = H / sup, w = W / sup, LD = L + dir.n;
    for (int c = 0; c < Co; ++c) {
        float v = F[i * fstride + c];
        for (int d = 0; d < dir.n; ++d)
            if (dir.ch[d] == c) v = z[(((size_t)b * LD + L + d) * h + y / sup) * w + x / sup];
        if (denorm) {
            float pr = __fmul_rn(v, std);
            asm("" : "+v"(pr));
            v = __fadd_rn(pr, mean);
        }
        out[((size_t)b * Co + c) * HW + p] = v;
    }
}

// UNetBlock.attn (unet_block.py:102-108) for more than 64 tokens in the fp32 / fp16 modes, where the scalar attn_kernel's LDS tiles do not reach and
// the MFMA kernel's bf16 operands would cost the mode its precision: the autoencoder's mid block sees (H / 2^(levels-1)) (W / 2^(levels-1)) tokens, which
// nothing bounds.  One wave per query, lane = channel of the 64-channel head; keys are walked once with a running maximum (online softmax), every sum a
// fixed butterfly over the wave.  qkv layout as attn_kernel: NHWC, channel = (head * 64 + c) * 3 + {q, k, v}.  Used by the autoencoder graphs only.
__device__ __forceinline__ float ae_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <typename T>
__global__ __launch_bounds__(256) void ae_attn_wave_kernel(const T* __restrict__ qkv, T* __restrict__ out, int tokens, int C) {
    const int n = blockIdx.x, head = blockIdx.y, lane = threadIdx.x & 63, q = blockIdx.z * 4 + (threadIdx.x >> 6);
    if (q >= tokens) return;   // (a whole wave: no workgroup barrier below)
    const size_t base = (size_t)n * tokens * 3 * C;
    const int ch = (head * 64 + lane) * 3;
    const float qv = (float)qkv[base + (size_t)q * 3 * C + ch];
    const float qn = qv * (1.f / (1e-4f + sqrtf(ae_wave_sum(qv * qv)) * 0.125f));
    float m = -3.0e38f, den = 0.f, acc = 0.f;
    for (int k = 0; k < tokens; ++k) {
        const T* p = qkv + base + (size_t)k * 3 * C + ch;
        const float kv = (float)p[1], vv = (float)p[2];
        const float kn = kv * (1.f / (1e-4f + sqrtf(ae_wave_sum(kv * kv)) * 0.125f)) * 0.125f;   // k / sqrt(64)
        const float vn = vv * (1.f / (1e-4f + sqrtf(ae_wave_sum(vv * vv)) * 0.125f));
        const float logit = ae_wave_sum(qn * kn);
        const float mn = fmaxf(m, logit), sc = expf(m - mn), e = expf(logit - mn);
        den = den * sc + e;
        acc = acc * sc + e * vn;
        m = mn;
    }
    out[((size_t)n * tokens + q) * C + head * 64 + lane] = (T)(acc / den);
}
template __global__ void ae_attn_wave_kernel<float>(const float*, float*, int, int);
template __global__ void ae_attn_wave_kernel<__bf16>(const __bf16*, __bf16*, int, int);
template __global__ void ae_attn_wave_kernel<_Float16>(const _Float16*, _Float16*, int, int);

template __global__ void ae_prep_input_kernel<float>(AeSrc, float*, int, int);
template __global__ void ae_prep_input_kernel<__bf16>(AeSrc, __bf16*, int, int);
template __global__ void ae_prep_input_kernel<_Float16>(AeSrc, _Float16*, int, int);

}  // namespace td
