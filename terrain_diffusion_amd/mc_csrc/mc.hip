// libtd_mc.so: the C-ABI of include/td_mc.h over the kernels of mc_kernels.hip.
#include "../side_csrc/td_side_host.h"
#include "../../include/td_mc.h"
#include "mc_kernels.hip"

using namespace td;

namespace {
bool size_ok(int H, int W) {
    return H >= 1 && W >= 1 && H <= TD_MC_MAX_SIDE && W <= TD_MC_MAX_SIDE && (long long)H * W <= TD_MC_MAX_PIXELS;
}
}  // namespace

extern "C" {

const char* td_mc_last_error(void) { return g_err.c_str(); }

int td_mc_upsample(void* hip_stream, const float* src, int C, int Hn, int Wn, int scale, long long r0, long long c0, int H, int W, float* out,
                   int synchronize) {
    if (!size_ok(H, W)) return fail(ERR_ARG, "td_mc_upsample: needs 1 <= H, W <= 2^16 and H * W <= 2^26");
    if (C < 1 || C > 64 || Hn < 1 || Wn < 1 || scale < 1 || scale > 1024 || (long long)Hn * Wn > (1LL << 30))
        return fail(ERR_ARG, "td_mc_upsample: needs 1 <= C <= 64, Hn, Wn >= 1, Hn * Wn <= 2^30 and 1 <= scale <= 1024");
    if (r0 < 0 || c0 < 0 || r0 + H > (long long)Hn * scale || c0 + W > (long long)Wn * scale)
        return fail(ERR_ARG, "td_mc_upsample: the box must lie inside the (Hn * scale, Wn * scale) upsampled image");
    if (!is_device_ptr(src) || !is_device_ptr(out)) return fail(ERR_ARG, "td_mc_upsample: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(mc_upsample_kernel, dim3(blocks((long long)H * W, MC_THREADS), C), dim3(MC_THREADS), 0, st, src, C, Hn, Wn, scale, (float)(1.0 / scale), r0, c0, H, W,
                       out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_mc_finish(void* hip_stream, const float* elev, long long elev_ld, const float* elev_padded, const float* climate, int n_climate, int H,
                 int W, long long i0, long long j0, const float* noise_planes, double noise_scale, double detail_pixel_size_m,
                 double native_resolution, double biome_pixel_size_m, float* elev_out, int16_t* biome_out, int synchronize) {
    if (!size_ok(H, W)) return fail(ERR_ARG, "td_mc_finish: needs 1 <= H, W <= 2^16 and H * W <= 2^26");
    if (elev_ld < W) return fail(ERR_ARG, "td_mc_finish: elev_ld must be >= W");
    if (!is_device_ptr(elev) || !is_device_ptr(elev_padded)) return fail(ERR_ARG, "td_mc_finish: device buffers only");
    const bool has_climate = climate != nullptr && n_climate >= 4;
    if ((has_climate && !is_device_ptr(climate)) || (noise_planes && !is_device_ptr(noise_planes)) || (elev_out && !is_device_ptr(elev_out)) ||
        (biome_out && !is_device_ptr(biome_out)))
        return fail(ERR_ARG, "td_mc_finish: device buffers only");
    if (!elev_out && !biome_out) return OK;
    McFinishArgs a;
    a.elev = elev; a.elev_ld = elev_ld; a.padded = elev_padded;
    a.climate = has_climate ? climate : nullptr; a.has_climate = has_climate ? 1 : 0;
    a.planes = noise_planes; a.H = H; a.W = W; a.i0 = i0; a.j0 = j0;
    // the reference's mixed scalar / tensor expressions: the leading all-Python part folded in double, each scalar then rounded to fp32
    a.detail_div = (float)(40.0 * detail_pixel_size_m / 90.0);
    a.amp_c = (float)(noise_scale * 100.0); a.amp_f = (float)(noise_scale * 70.0);
    a.px_m = (float)detail_pixel_size_m; a.nr = (float)native_resolution;
    a.detail_on = noise_scale > 0.0 ? 1 : 0;
    a.biome_px = (float)biome_pixel_size_m;
    a.bare_span = (float)(1.19 - 0.7);
    a.elev_out = elev_out; a.biome_out = biome_out;
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(mc_finish_kernel, dim3((W + MC_TILE - 1) / MC_TILE, (H + MC_TILE - 1) / MC_TILE), dim3(MC_TILE * MC_TILE), 0, st, a);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_mc_noise(void* hip_stream, int H, int W, long long i0, long long j0, float* out, int synchronize) {
    if (!size_ok(H, W)) return fail(ERR_ARG, "td_mc_noise: needs 1 <= H, W <= 2^16 and H * W <= 2^26");
    if (!is_device_ptr(out)) return fail(ERR_ARG, "td_mc_noise: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(mc_noise_kernel, dim3(blocks((long long)H * W, MC_THREADS)), dim3(MC_THREADS), 0, st, H, W, i0, j0, out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_mc_payload(void* hip_stream, const float* elev, const int16_t* biome, int H, int W, int16_t* out, int synchronize) {
    if (!size_ok(H, W)) return fail(ERR_ARG, "td_mc_payload: needs 1 <= H, W <= 2^16 and H * W <= 2^26");
    if (!is_device_ptr(elev) || !is_device_ptr(out) || (biome && !is_device_ptr(biome))) return fail(ERR_ARG, "td_mc_payload: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(mc_payload_kernel, dim3(blocks(n, MC_THREADS)), dim3(MC_THREADS), 0, st, elev, biome, n, out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

}  // extern "C"
