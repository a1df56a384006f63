// The host half of a relief render, shared by libtd_relief.so (td_relief_map: relief_render<false>, which ignores `ov`) and libtd_rivers.so
// (td_rivers_relief: relief_render<true>); each library holds only its own instantiation of the shade kernel.  Argument checks, the scalars
// of ReliefParams in the reference's precision, the scratch and the two launches.  Included after side_csrc/td_side_host.h by a library's
// one translation unit; `who` heads the error messages.
#pragma once
#include <math.h>

#include "relief_kernels.hip"

namespace td {

template <bool OVERLAY>
int relief_render(const char* who, void* hip_stream, const float* elev, int H, int W, const float* lut, const float* wl, int rl, const float* ws,
                  int rs, double azimuth_deg, double resolution, double relief, int has_range, double vmin, double vmax, int has_fill,
                  double fill, const ReliefOverlay& ov, float* out, int synchronize) {
    const std::string me = std::string(who) + ": ";
    if (H < 2 || W < 2 || H > (1 << 20) || W > (1 << 20)) return fail(ERR_ARG, me + "the image needs 2 <= H, W <= 2^20 (np.gradient needs 2 samples per axis)");
    if (rl < 0 || rl > RELIEF_MAX_RADIUS || rs < 0 || rs > RELIEF_MAX_RADIUS)
        return fail(ERR_ARG, me + "blur radius outside [0, " + std::to_string(RELIEF_MAX_RADIUS) + "] (sigma below 15.9)");
    if (!elev || !lut || !wl || !ws || !out) return fail(ERR_ARG, me + "null buffer");
    if (!is_device_ptr(elev) || !is_device_ptr(lut) || !is_device_ptr(wl) || !is_device_ptr(ws) || !is_device_ptr(out))
        return fail(ERR_ARG, me + "device buffers only");
    if (OVERLAY) {
        if (ov.biome && !ov.palette) return fail(ERR_ARG, me + "a biome image needs the palette");
        for (const void* q : {(const void*)ov.rgb, (const void*)ov.biome, (const void*)ov.flow, (const void*)(ov.biome ? ov.palette : nullptr)})
            if (q && !is_device_ptr(q)) return fail(ERR_ARG, me + "device buffers only");
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t npx = (size_t)H * W;
    // scratch: the two axis-0-blurred planes and the two range words, from the stream-ordered pool; a caller's rgb replaces the colormap, so
    // there is no colour range then and no reduction for it
    void* scratch = nullptr;
    TD_HIP_TRY(hipMallocAsync(&scratch, 2 * npx * 4 + 256, st));
    float* bl = (float*)scratch;
    float* bs = bl + npx;
    unsigned* range_bits = (has_range || (OVERLAY && ov.rgb)) ? nullptr : (unsigned*)(bs + npx);
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
        const dim3 grid2((W + RELIEF_P2_TX - 1) / RELIEF_P2_TX, (H + RELIEF_P2_TY - 1) / RELIEF_P2_TY);
        hipLaunchKernelGGL(relief_blur_rows_kernel, dim3((W + RELIEF_P1_COLS - 1) / RELIEF_P1_COLS, (H + RELIEF_P1_ROWS - 1) / RELIEF_P1_ROWS),
                           dim3(RELIEF_THREADS), relief_blur_lds_floats(R) * 4, st, elev, bl, bs, H, W, wl, rl, ws, rs, p.has_fill, p.fill, range_bits);
        hipLaunchKernelGGL(relief_shade_kernel<OVERLAY>, grid2, dim3(RELIEF_THREADS), relief_shade_lds_floats(R) * 4, st, elev, (const float*)bl,
                           (const float*)bs, H, W, wl, rl, ws, rs, lut, (const unsigned*)range_bits, p, ov, out);
        err = hipGetLastError();
    }
    return finish(st, scratch, err, synchronize);   // the scratch goes back to the pool behind the two kernels
}

}  // namespace td
