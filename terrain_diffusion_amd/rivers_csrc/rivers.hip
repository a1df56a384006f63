// libtd_rivers.so: the C-ABI of include/td_rivers.h.  The relief picture is relief_csrc's render with the overlay instantiation of its shade
// kernel (no arithmetic of it is restated here); the smoothing kernel is rivers_kernels.hip.
#include <stdint.h>

#include "../side_csrc/td_side_host.h"
#include "../../include/td_rivers.h"
#include "../relief_csrc/relief_host.h"
#include "rivers_kernels.hip"

using namespace td;

extern "C" {

const char* td_rivers_last_error(void) { return g_err.c_str(); }

int td_rivers_relief(void* hip_stream, const float* elev, int H, int W, const float* lut, const float* wl, int rl, const float* ws, int rs,
                     double azimuth_deg, double resolution, double relief, int has_range, double vmin, double vmax, int has_fill, double fill,
                     const float* rgb, const int32_t* biome, const float* palette, const float* flow, double flow_threshold, float* out,
                     int synchronize) {
    ReliefOverlay ov;
    ov.rgb = rgb;
    ov.biome = biome;
    ov.palette = palette;
    ov.flow = flow;
    ov.flow_threshold = (float)flow_threshold;   // NumPy >= 2 compares a float32 array with fl32(python float)
    return relief_render<true>("td_rivers_relief", hip_stream, elev, H, W, lut, wl, rl, ws, rs, azimuth_deg, resolution, relief, has_range, vmin, vmax,
                               has_fill, fill, ov, out, synchronize);
}

int td_rivers_smooth(void* hip_stream, const float* h, int H, int W, double slope_thresh, double smooth_strength, int iterations, float* out,
                     int synchronize) {
    if (H < 2 || W < 2 || H > (1 << 20) || W > (1 << 20) || (long long)H * W >= (1LL << 31))
        return fail(ERR_ARG, "td_rivers_smooth: the image needs 2 <= H, W <= 2^20 and H * W < 2^31 (np.gradient needs 2 samples per axis)");
    if (iterations < 0 || iterations > RIVERS_MAX_ITERATIONS)
        return fail(ERR_ARG, "td_rivers_smooth: iterations outside [0, " + std::to_string(RIVERS_MAX_ITERATIONS) + "]");
    if (!h || !out) return fail(ERR_ARG, "td_rivers_smooth: null buffer");
    if (!is_device_ptr(h) || !is_device_ptr(out)) return fail(ERR_ARG, "td_rivers_smooth: device buffers only");
    const size_t npx = (size_t)H * W;
    if ((uintptr_t)h < (uintptr_t)(out + npx) && (uintptr_t)out < (uintptr_t)(h + npx))
        return fail(ERR_ARG, "td_rivers_smooth: out must not overlap h (an iteration reads its neighbours' old values)");
    hipStream_t st = (hipStream_t)hip_stream;
    if (iterations == 0) return finish(st, nullptr, hipMemcpyAsync(out, h, npx * 4, hipMemcpyDeviceToDevice, st), synchronize);
    // one launch per iteration, alternating between `out` and one scratch plane so that the last iteration writes `out`
    void* scratch = nullptr;
    if (iterations > 1) TD_HIP_TRY(hipMallocAsync(&scratch, npx * 4, st));
    const float thresh = (float)slope_thresh, strength = (float)smooth_strength;   // fl32 of the python floats, as NumPy >= 2 takes them
    const float* src = h;
    for (int it = 0; it < iterations; ++it) {
        float* dst = ((iterations - 1 - it) & 1) ? (float*)scratch : out;
        hipLaunchKernelGGL(rivers_smooth_kernel, dim3(blocks((long long)npx, RIVERS_THREADS)), dim3(RIVERS_THREADS), 0, st, src, dst, H, W, thresh, strength);
        src = dst;
    }
    return finish(st, scratch, hipGetLastError(), synchronize);
}

}  // extern "C"
