// libtd_relief.so: the C-ABI of include/td_relief.h over the two kernels of relief_kernels.hip.
#include <math.h>

#include "../side_csrc/td_side_host.h"
#include "../../include/td_relief.h"
#include "relief_kernels.hip"

using namespace td;

extern "C" {

const char* td_relief_last_error(void) { return g_err.c_str(); }

int td_relief_map(void* hip_stream, const float* elev, int H, int W, const float* lut, const float* wl, int rl, const float* ws, int rs,
                  double azimuth_deg, double resolution, double relief, int has_range, double vmin, double vmax, int has_fill, double fill,
                  float* out, int synchronize) {
    if (H < 2 || W < 2 || H > (1 << 20) || W > (1 << 20)) return fail(ERR_ARG, "td_relief_map: the image needs 2 <= H, W <= 2^20 (np.gradient needs 2 samples per axis)");
    if (rl < 0 || rl > RELIEF_MAX_RADIUS || rs < 0 || rs > RELIEF_MAX_RADIUS)
        return fail(ERR_ARG, "td_relief_map: blur radius outside [0, " + std::to_string(RELIEF_MAX_RADIUS) + "] (sigma below 15.9)");
    if (!elev || !lut || !wl || !ws || !out) return fail(ERR_ARG, "td_relief_map: null buffer");
    if (!is_device_ptr(elev) || !is_device_ptr(lut) || !is_device_ptr(wl) || !is_device_ptr(ws) || !is_device_ptr(out))
        return fail(ERR_ARG, "td_relief_map: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t npx = (size_t)H * W;
    // scratch: the two axis-0-blurred planes and the two range words, from the stream-ordered pool
    void* scratch = nullptr;
    TD_HIP_TRY(hipMallocAsync(&scratch, 2 * npx * 4 + 256, st));
    float* bl = (float*)scratch;
    float* bs = bl + npx;
    unsigned* range_bits = has_range ? nullptr : (unsigned*)(bs + npx);
    hipError_t err = hipSuccess;
    if (range_bits) err = hipMemsetAsync(range_bits, 0, 2 * sizeof(unsigned), st);
    ReliefParams p;
    const double deg = 3.14159265358979323846 / 180.0;   // np.deg2rad
    p.az = (float)(azimuth_deg * deg);
    p.sin_alt = (float)sin(45.0 * deg);
    p.cos_alt = (float)cos(45.0 * deg);
    p.scale = (float)(15.0 * resolution / 90.0);
    p.relief = (float)relief;
    p.one_minus_relief = (float)(1.0 - relief);
    p.vmin = vmin;
    p.vmax = vmax;
    p.has_range = has_range ? 1 : 0;
    p.has_fill = has_fill ? 1 : 0;
    p.fill = (float)fill;
    const int R = rl > rs ? rl : rs;
    if (err == hipSuccess) {
        hipLaunchKernelGGL(relief_blur_rows_kernel, dim3((W + RELIEF_P1_COLS - 1) / RELIEF_P1_COLS, (H + RELIEF_P1_ROWS - 1) / RELIEF_P1_ROWS),
                           dim3(RELIEF_THREADS), relief_blur_lds_floats(R) * 4, st, elev, bl, bs, H, W, wl, rl, ws, rs, p.has_fill, p.fill, range_bits);
        hipLaunchKernelGGL(relief_shade_kernel, dim3((W + RELIEF_P2_TX - 1) / RELIEF_P2_TX, (H + RELIEF_P2_TY - 1) / RELIEF_P2_TY), dim3(RELIEF_THREADS),
                           relief_shade_lds_floats(R) * 4, st, elev, (const float*)bl, (const float*)bs, H, W, wl, rl, ws, rs, lut,
                           (const unsigned*)range_bits, p, out);
        err = hipGetLastError();
    }
    return finish(st, scratch, err, synchronize);   // the scratch goes back to the pool behind the two kernels
}

}  // extern "C"
