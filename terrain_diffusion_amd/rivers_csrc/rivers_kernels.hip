// Kernels of libtd_rivers.so (include/td_rivers.h).  The relief picture with overlays is relief_shade_kernel<true> of
// relief_csrc/relief_kernels.hip; this file holds what the relief library has no use for:
//   rivers_smooth_kernel   one iteration of smooth_river_bumps (terrain_diffusion/inference/postprocessing.py:87-135), one pixel per thread.
// All fp32 in the reference's operation order, with no contraction (numpy does not fuse) and the precise device expf / sqrtf / division.
#include <hip/hip_runtime.h>
#include <math.h>

namespace td {

constexpr int RIVERS_THREADS = 256;
constexpr int RIVERS_MAX_ITERATIONS = 64;

// h_safe of the reference: NaN -> 0
__device__ __forceinline__ float rivers_safe(float v) { return isnan(v) ? 0.f : v; }

// dst = one smoothing iteration of src, (H, W) with 2 <= H, W and H * W < 2^31; src and dst do not overlap.  Grid ceil(H * W / 256).
//   gradient    np.gradient of h_safe: central differences / 2 inside, one-sided at the image's edges (not wrapped);
//   neighbours  np.roll: they wrap around the image; a NaN neighbour adds 0 to the sum and nothing to the count;
//   update      h + (strength * exp(-(slope / thresh)^2)) * (sum - count * h); a NaN cell stays NaN.
__global__ __launch_bounds__(RIVERS_THREADS) void rivers_smooth_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, float thresh,
                                                                       float strength) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * RIVERS_THREADS + threadIdx.x;
    if (i >= (long long)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const float c = src[i];
    if (isnan(c)) {
        dst[i] = c;
        return;
    }
    const float* row = src + (size_t)y * W;
    const float up_raw = src[(size_t)(y == 0 ? H - 1 : y - 1) * W + x], dn_raw = src[(size_t)(y == H - 1 ? 0 : y + 1) * W + x];
    const float lf_raw = row[x == 0 ? W - 1 : x - 1], rt_raw = row[x == W - 1 ? 0 : x + 1];
    const float up = rivers_safe(up_raw), dn = rivers_safe(dn_raw), lf = rivers_safe(lf_raw), rt = rivers_safe(rt_raw);
    // the wrapped neighbours are the gradient's samples everywhere but at the image's edges, where the difference is one-sided
    const float gy = y == 0 ? dn - c : (y == H - 1 ? c - up : (dn - up) / 2.f);
    const float gx = x == 0 ? rt - c : (x == W - 1 ? c - lf : (rt - lf) / 2.f);
    const float slope = sqrtf(gx * gx + gy * gy);
    const float sum = ((up + dn) + lf) + rt;
    const float cnt = (((isnan(up_raw) ? 0.f : 1.f) + (isnan(dn_raw) ? 0.f : 1.f)) + (isnan(lf_raw) ? 0.f : 1.f)) + (isnan(rt_raw) ? 0.f : 1.f);
    const float lap = sum - cnt * c;
    const float q = slope / thresh;
    const float w = expf(-(q * q));
    dst[i] = c + (strength * w) * lap;
}

}  // namespace td
