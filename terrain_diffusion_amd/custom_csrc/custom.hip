// libtd_custom.so: the C-ABI of include/td_custom.h over the kernels of custom_kernels.hip.
#include "../side_csrc/td_side_host.h"
#include "../../include/td_custom.h"
#include "custom_kernels.hip"

using namespace td;

namespace {
bool side_ok(int H, int W) { return H >= 1 && W >= 1 && H <= TD_CUSTOM_MAX_SIDE && W <= TD_CUSTOM_MAX_SIDE; }
const char* const SIDE_MSG = ": needs 1 <= H, W <= 16384";
bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
}  // namespace

extern "C" {

const char* td_custom_last_error(void) { return g_err.c_str(); }

int td_custom_rasterize(void* hip_stream, const double* xy, int64_t n_xy, const int32_t* offsets, const float* values, int n, int H, int W,
                        double fill, float* out, int synchronize) {
    if (!side_ok(H, W)) return fail(ERR_ARG, std::string("td_custom_rasterize") + SIDE_MSG);
    if (n < 0 || n_xy < 0 || n_xy > INT32_MAX) return fail(ERR_ARG, "td_custom_rasterize: needs n >= 0 and 0 <= n_xy < 2^31 (int32 offsets)");
    if (!out) return fail(ERR_ARG, "td_custom_rasterize: null buffer");
    if (n > 0 && (!offsets || !values || (n_xy > 0 && !xy))) return fail(ERR_ARG, "td_custom_rasterize: null buffer");
    if (!is_device_ptr(out) || (n > 0 && (!is_device_ptr(offsets) || !is_device_ptr(values) || (n_xy > 0 && !is_device_ptr(xy)))))
        return fail(ERR_ARG, "td_custom_rasterize: device buffers only");
    if (n > 0 && n_xy > 0 && !aligned(xy, 16)) return fail(ERR_ARG, "td_custom_rasterize: xy needs 16-byte alignment");
    hipStream_t st = (hipStream_t)hip_stream;
    const int npx = H * W;
    void* scratch = nullptr;                              // the owner plane, from the stream-ordered pool
    TD_HIP_TRY(hipMallocAsync(&scratch, (size_t)npx * sizeof(int), st));
    int* owner = (int*)scratch;
    hipError_t err = hipMemsetAsync(owner, 0xff, (size_t)npx * sizeof(int), st);   // -1: no polygon
    if (err == hipSuccess) {
        if (n > 0 && n_xy > 0) {
            // few polygons on a large raster: up to CW_MAX_SLICES waves share each bounding box, so that one large cell is not one wave's work
            long long slices = ((long long)npx / 4096 + n - 1) / n;
            slices = slices < 1 ? 1 : (slices > CW_MAX_SLICES ? CW_MAX_SLICES : slices);
            hipLaunchKernelGGL(cw_owner_kernel, dim3(blocks(n, CW_WAVES), (unsigned)slices), dim3(CW_THREADS), 0, st, (const double2*)xy,
                               (long long)n_xy, offsets, n, H, W, owner);
        }
        hipLaunchKernelGGL(cw_paint_kernel, dim3(blocks(npx, CW_THREADS)), dim3(CW_THREADS), 0, st, (const int*)owner, values, (float)fill, npx, out);
        err = hipGetLastError();
    }
    return finish(st, scratch, err, synchronize);
}

int td_custom_fill_nearest(void* hip_stream, const float* in, int H, int W, double nodata, float* out, int32_t* out_index,
                           int32_t* out_valid, int synchronize) {
    if (!side_ok(H, W)) return fail(ERR_ARG, std::string("td_custom_fill_nearest") + SIDE_MSG);
    if (!in || !out || !out_valid) return fail(ERR_ARG, "td_custom_fill_nearest: null buffer");
    if (!is_device_ptr(in) || !is_device_ptr(out) || !is_device_ptr(out_valid) || (out_index && !is_device_ptr(out_index)))
        return fail(ERR_ARG, "td_custom_fill_nearest: device buffers only");
    const size_t bytes = (size_t)H * W * sizeof(float);
    if ((const char*)in < (const char*)out + bytes && (const char*)out < (const char*)in + bytes)
        return fail(ERR_ARG, "td_custom_fill_nearest: out overlaps in");
    hipStream_t st = (hipStream_t)hip_stream;
    void* scratch = nullptr;                              // the column plane, from the stream-ordered pool
    TD_HIP_TRY(hipMallocAsync(&scratch, (size_t)H * W * sizeof(int), st));
    int* off = (int*)scratch;
    hipError_t err = hipMemsetAsync(out_valid, 0, sizeof(int32_t), st);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(cw_fill_columns_kernel, dim3(blocks(W, CW_THREADS)), dim3(CW_THREADS), 0, st, in, H, W, (float)nodata, off, out_valid);
        hipLaunchKernelGGL(cw_fill_rows_kernel, dim3(blocks(W, CW_THREADS), (unsigned)H), dim3(CW_THREADS), 0, st, in, (const int*)off, H, W,
                           (float)nodata, out, out_index);
        err = hipGetLastError();
    }
    return finish(st, scratch, err, synchronize);
}

int td_custom_elev_int16(void* hip_stream, const float* elev, int64_t n, int16_t* out, int synchronize) {
    if (n < 0 || n > TD_CUSTOM_MAX_ELEMENTS) return fail(ERR_ARG, "td_custom_elev_int16: needs 0 <= n <= 2^30");
    hipStream_t st = (hipStream_t)hip_stream;
    if (n == 0) return finish(st, nullptr, hipSuccess, synchronize);
    if (!elev || !out) return fail(ERR_ARG, "td_custom_elev_int16: null buffer");
    if (!is_device_ptr(elev) || !is_device_ptr(out)) return fail(ERR_ARG, "td_custom_elev_int16: device buffers only");
    if (!aligned(out, 2) || !aligned(elev, 4)) return fail(ERR_ARG, "td_custom_elev_int16: elev needs 4-byte and out 2-byte alignment");
    const int vec = aligned(elev, 16) && aligned(out, 8);
    hipLaunchKernelGGL(cw_elev_int16_kernel, dim3(blocks((n + 3) / 4, CW_THREADS)), dim3(CW_THREADS), 0, st, elev, (long long)n, vec, (short*)out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

}  // extern "C"
