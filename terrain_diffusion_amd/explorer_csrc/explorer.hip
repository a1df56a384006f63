// libtd_explorer.so: the C-ABI of include/td_explorer.h over the kernels of explorer_kernels.hip.
#include <math.h>

#include "../side_csrc/td_side_host.h"
#include "../../include/td_explorer.h"
#include "explorer_kernels.hip"

using namespace td;

namespace {
bool size_ok(int H, int W) {
    return H >= 1 && W >= 1 && H <= TD_EXPLORER_MAX_SIDE && W <= TD_EXPLORER_MAX_SIDE && (long long)H * W <= TD_EXPLORER_MAX_PIXELS;
}
const char* const SIZE_MSG = ": needs 1 <= H, W <= 2^16 and H * W <= 2^26";
unsigned reduce_blocks(long long n) { return blocks(n, EX_THREADS) < EX_REDUCE_BLOCKS ? blocks(n, EX_THREADS) : EX_REDUCE_BLOCKS; }
}  // namespace

extern "C" {

const char* td_explorer_last_error(void) { return g_err.c_str(); }

int td_explorer_channels(void* hip_stream, const float* sums, int C, int H, int W, int n_signed_sq, double eps, float* out, float* minmax,
                         int synchronize) {
    if (!size_ok(H, W)) return fail(ERR_ARG, std::string("td_explorer_channels") + SIZE_MSG);
    if (C < 1 || C > TD_EXPLORER_MAX_CHANNELS) return fail(ERR_ARG, "td_explorer_channels: needs 1 <= C <= 8");
    if (n_signed_sq < 0 || n_signed_sq > C) return fail(ERR_ARG, "td_explorer_channels: needs 0 <= n_signed_sq <= C");
    if (!(eps >= 0.0) || !isfinite(eps)) return fail(ERR_ARG, "td_explorer_channels: eps must be finite and >= 0");
    if (!is_device_ptr(sums) || !is_device_ptr(out) || (minmax && !is_device_ptr(minmax)))
        return fail(ERR_ARG, "td_explorer_channels: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    const long long n = (long long)H * W;
    void* scratch = nullptr;
    hipError_t err = hipSuccess;
    if (minmax) {
        TD_HIP_TRY(hipMallocAsync(&scratch, 2 * TD_EXPLORER_MAX_CHANNELS * sizeof(unsigned), st));
        err = hipMemsetAsync(scratch, 0, 2 * TD_EXPLORER_MAX_CHANNELS * sizeof(unsigned), st);
    }
    if (err == hipSuccess) {
        hipLaunchKernelGGL(ex_channels_kernel, dim3(reduce_blocks(n), C), dim3(EX_THREADS), 0, st, sums, C, n, n_signed_sq, eps != 0.0 ? 1 : 0, (float)eps,
                           out, (unsigned*)scratch);
        if (minmax) hipLaunchKernelGGL(ex_decode_kernel, dim3(1), dim3(64), 0, st, (const unsigned*)scratch, C, minmax);
        err = hipGetLastError();
    }
    return finish(st, scratch, err, synchronize);
}

int td_explorer_colorize(void* hip_stream, const float* field, int H, int W, int log1p, int has_range, double vmin, double vmax, const float* lut,
                         int n_filters, const float* const* planes, const double* lo, const double* hi, const int* use_lo, const int* use_hi,
                         uint8_t* out, float* range_out, int synchronize) {
    if (!size_ok(H, W)) return fail(ERR_ARG, std::string("td_explorer_colorize") + SIZE_MSG);
    if (n_filters < 0 || n_filters > TD_EXPLORER_MAX_FILTERS) return fail(ERR_ARG, "td_explorer_colorize: at most 8 filter planes");
    if (n_filters > 0 && (!planes || !lo || !hi || !use_lo || !use_hi)) return fail(ERR_ARG, "td_explorer_colorize: null filter arrays");
    if (has_range && !(isfinite(vmin) && isfinite(vmax) && vmin < vmax)) return fail(ERR_ARG, "td_explorer_colorize: needs finite vmin < vmax");
    if (!is_device_ptr(field) || !is_device_ptr(lut) || !is_device_ptr(out) || (range_out && !is_device_ptr(range_out)))
        return fail(ERR_ARG, "td_explorer_colorize: device buffers only");
    ExColorArgs a;
    for (int f = 0; f < n_filters; ++f) {
        if (!is_device_ptr(planes[f])) return fail(ERR_ARG, "td_explorer_colorize: filter planes must be device buffers");
        a.planes[f] = planes[f];
        a.lo[f] = (float)lo[f]; a.hi[f] = (float)hi[f];
        a.use_lo[f] = use_lo[f] ? 1 : 0; a.use_hi[f] = use_hi[f] ? 1 : 0;
    }
    for (int f = n_filters; f < EX_MAX_FILTERS; ++f) { a.planes[f] = nullptr; a.lo[f] = a.hi[f] = 0.f; a.use_lo[f] = a.use_hi[f] = 0; }
    hipStream_t st = (hipStream_t)hip_stream;
    const long long n = (long long)H * W;
    void* scratch = nullptr;
    hipError_t err = hipSuccess;
    if (!has_range) {
        TD_HIP_TRY(hipMallocAsync(&scratch, 2 * sizeof(unsigned), st));
        err = hipMemsetAsync(scratch, 0, 2 * sizeof(unsigned), st);
    }
    a.field = field; a.n = n; a.log1p_on = log1p ? 1 : 0; a.has_range = has_range ? 1 : 0; a.vmin = vmin; a.vmax = vmax;
    a.words = (const unsigned*)scratch; a.lut = lut; a.n_filters = n_filters; a.out = (uchar4*)out; a.range_out = range_out;
    if (err == hipSuccess) {
        if (!has_range) hipLaunchKernelGGL(ex_range_kernel, dim3(reduce_blocks(n)), dim3(EX_THREADS), 0, st, field, n, a.log1p_on, (unsigned*)scratch);
        hipLaunchKernelGGL(ex_color_kernel, dim3(blocks(n, EX_THREADS)), dim3(EX_THREADS), 0, st, a);
        err = hipGetLastError();
    }
    return finish(st, scratch, err, synchronize);
}

int td_explorer_quantize(void* hip_stream, const float* rgb, int H, int W, uint8_t* out, int synchronize) {
    if (!size_ok(H, W)) return fail(ERR_ARG, std::string("td_explorer_quantize") + SIZE_MSG);
    if (!is_device_ptr(rgb) || !is_device_ptr(out)) return fail(ERR_ARG, "td_explorer_quantize: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(ex_quantize_kernel, dim3(blocks(n, EX_THREADS)), dim3(EX_THREADS), 0, st, rgb, n, (uchar4*)out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_explorer_raw(void* hip_stream, const float* elev, const float* temp, int H, int W, uint8_t* out, int synchronize) {
    if (!size_ok(H, W)) return fail(ERR_ARG, std::string("td_explorer_raw") + SIZE_MSG);
    if (!is_device_ptr(elev) || !is_device_ptr(out) || (temp && !is_device_ptr(temp))) return fail(ERR_ARG, "td_explorer_raw: device buffers only");
    if ((uintptr_t)out & 1u) return fail(ERR_ARG, "td_explorer_raw: out needs 2-byte alignment");
    hipStream_t st = (hipStream_t)hip_stream;
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(ex_raw_kernel, dim3(blocks(n, EX_THREADS)), dim3(EX_THREADS), 0, st, elev, temp, n, (uint16_t*)out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_explorer_land_tiles(void* hip_stream, const float* elev_m, int H, int W, int half, double min_land_frac, int32_t* out_idx,
                           int32_t* out_count, int synchronize) {
    if (!size_ok(H, W)) return fail(ERR_ARG, std::string("td_explorer_land_tiles") + SIZE_MSG);
    if (half < 0 || half > TD_EXPLORER_MAX_HALF) return fail(ERR_ARG, "td_explorer_land_tiles: needs 0 <= half <= 2047");
    if (2LL * half > H || 2LL * half > W) return fail(ERR_ARG, "td_explorer_land_tiles: the 2 half x 2 half window is larger than the plane");
    if (min_land_frac != min_land_frac) return fail(ERR_ARG, "td_explorer_land_tiles: min_land_frac is NaN");
    if (!is_device_ptr(elev_m) || !is_device_ptr(out_count)) return fail(ERR_ARG, "td_explorer_land_tiles: device buffers only");
    const long long capacity = half == 0 ? 0 : (long long)(H - 2 * half) * (W - 2 * half);
    if (capacity > 0 && !is_device_ptr(out_idx)) return fail(ERR_ARG, "td_explorer_land_tiles: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    if (capacity == 0) {
        TD_HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(int32_t), st));
        return finish(st, nullptr, hipSuccess, synchronize);
    }
    const long long n = (long long)H * W;
    const unsigned nb = blocks(n, EX_THREADS);
    // scratch: the row counts (uint16 per pixel), the flags (uint8 per pixel), the per-block counts (uint32)
    const size_t rows_bytes = ((size_t)n * 2 + 255) & ~(size_t)255, flags_bytes = ((size_t)n + 255) & ~(size_t)255;
    void* scratch = nullptr;
    TD_HIP_TRY(hipMallocAsync(&scratch, rows_bytes + flags_bytes + (size_t)nb * sizeof(unsigned), st));
    uint16_t* rows = (uint16_t*)scratch;
    uint8_t* flags = (uint8_t*)scratch + rows_bytes;
    unsigned* counts = (unsigned*)((uint8_t*)scratch + rows_bytes + flags_bytes);
    hipLaunchKernelGGL(ex_land_rows_kernel, dim3(nb), dim3(EX_THREADS), 0, st, elev_m, H, W, half, rows);
    hipLaunchKernelGGL(ex_land_flags_kernel, dim3(nb), dim3(EX_THREADS), 0, st, (const uint16_t*)rows, H, W, half, (float)(4LL * half * half),
                       min_land_frac, flags, counts);
    hipLaunchKernelGGL(ex_land_scan_kernel, dim3(1), dim3(1024), 0, st, counts, (int)nb, out_count);
    hipLaunchKernelGGL(ex_land_scatter_kernel, dim3(nb), dim3(EX_THREADS), 0, st, (const uint8_t*)flags, n, (const unsigned*)counts, capacity, out_idx);
    return finish(st, scratch, hipGetLastError(), synchronize);
}

}  // extern "C"
