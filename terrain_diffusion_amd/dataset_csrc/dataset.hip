// libtd_dataset.so: the C-ABI of include/td_dataset.h over the kernels of dataset_kernels.hip.
#include "../side_csrc/td_side_host.h"
#include "../../include/td_dataset.h"
#include "dataset_kernels.hip"

using namespace td;

static_assert(DS_MAX_RADIUS == TD_DATASET_MAX_RADIUS, "the row pass stages radius - 1 columns either side");
static_assert(TD_DATASET_MAX_BLOCK * TD_DATASET_MAX_BLOCK <= DS_MED_ITEMS, "one block of the median holds a whole r x r block");

namespace {
bool side_ok(int H, int W) { return H >= 1 && W >= 1 && H <= TD_DATASET_MAX_SIDE && W <= TD_DATASET_MAX_SIDE; }
bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}
size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }
}  // namespace

extern "C" {

const char* td_dataset_last_error(void) { return g_err.c_str(); }

int td_dataset_fill_voids(void* hip_stream, const float* dem, const float* base, int H, int W, int radius, int signed_sqrt, float* out,
                          int32_t* out_void_count, int synchronize) {
    if (!side_ok(H, W)) return fail(ERR_ARG, "td_dataset_fill_voids: needs 1 <= H, W <= 16384");
    if (radius < 1 || radius > TD_DATASET_MAX_RADIUS) return fail(ERR_ARG, "td_dataset_fill_voids: needs 1 <= radius <= 64");
    if (!dem || !base || !out || !out_void_count) return fail(ERR_ARG, "td_dataset_fill_voids: null buffer");
    if (!is_device_ptr(dem) || !is_device_ptr(base) || !is_device_ptr(out) || !is_device_ptr(out_void_count))
        return fail(ERR_ARG, "td_dataset_fill_voids: device buffers only");
    const size_t bytes = (size_t)H * W * sizeof(float);
    if (overlap(dem, bytes, out, bytes)) return fail(ERR_ARG, "td_dataset_fill_voids: out overlaps dem");
    hipStream_t st = (hipStream_t)hip_stream;
    void* scratch = nullptr;                              // the plane of capped column distances, one byte per pixel
    TD_HIP_TRY(hipMallocAsync(&scratch, (size_t)H * W, st));
    unsigned char* g = (unsigned char*)scratch;
    hipError_t err = hipMemsetAsync(out_void_count, 0, sizeof(int32_t), st);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(ds_void_columns_kernel, dim3(blocks(W, DS_THREADS), blocks(H, DS_BAND)), dim3(DS_THREADS), 0, st, dem, H, W, radius, g,
                           out_void_count);
        hipLaunchKernelGGL(ds_void_rows_kernel, dim3(blocks(W, DS_THREADS), (unsigned)H), dim3(DS_THREADS), 0, st, dem, base,
                           (const unsigned char*)g, H, W, radius, signed_sqrt ? 1 : 0, out);
        err = hipGetLastError();
    }
    return finish(st, scratch, err, synchronize);
}

int td_dataset_block_median(void* hip_stream, const float* x, int H, int W, int r, float* out, int synchronize) {
    if (!side_ok(H, W)) return fail(ERR_ARG, "td_dataset_block_median: needs 1 <= H, W <= 16384");
    if (r < 1 || r > TD_DATASET_MAX_BLOCK) return fail(ERR_ARG, "td_dataset_block_median: needs 1 <= r <= 32");
    if (H % r != 0 || W % r != 0) return fail(ERR_ARG, "td_dataset_block_median: r must divide H and W");
    if (!x || !out) return fail(ERR_ARG, "td_dataset_block_median: null buffer");
    if (!is_device_ptr(x) || !is_device_ptr(out)) return fail(ERR_ARG, "td_dataset_block_median: device buffers only");
    const int Hb = H / r, Wb = W / r;
    if (overlap(x, (size_t)H * W * sizeof(float), out, (size_t)Hb * Wb * sizeof(float))) return fail(ERR_ARG, "td_dataset_block_median: out overlaps x");
    hipStream_t st = (hipStream_t)hip_stream;
    const int G = DS_MED_ITEMS / (r * r);                 // >= 1
    hipLaunchKernelGGL(ds_block_median_kernel, dim3(blocks(Wb, G), (unsigned)Hb), dim3(DS_THREADS), 0, st, x, W, r, Wb, G, out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_dataset_residual(void* hip_stream, const float* x, const float* low, int H, int W, int h, int w, float* out, int synchronize) {
    if (!side_ok(H, W) || !side_ok(h, w)) return fail(ERR_ARG, "td_dataset_residual: needs 1 <= H, W, h, w <= 16384");
    if (!x || !low || !out) return fail(ERR_ARG, "td_dataset_residual: null buffer");
    if (!is_device_ptr(x) || !is_device_ptr(low) || !is_device_ptr(out)) return fail(ERR_ARG, "td_dataset_residual: device buffers only");
    const size_t bytes = (size_t)H * W * sizeof(float);
    if (out != x && overlap(x, bytes, out, bytes)) return fail(ERR_ARG, "td_dataset_residual: out overlaps x without being x");
    if (overlap(low, (size_t)h * w * sizeof(float), out, bytes)) return fail(ERR_ARG, "td_dataset_residual: out overlaps low");
    hipStream_t st = (hipStream_t)hip_stream;
    const int vec = W % 4 == 0 && aligned(x, 16) && aligned(out, 16);
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    hipLaunchKernelGGL(ds_residual_kernel, dim3(blocks((W + 3) / 4, DS_THREADS), (unsigned)H), dim3(DS_THREADS), 0, st, x, low, H, W, h, w, sy, sx,
                       vec, out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_dataset_land_counts(void* hip_stream, const float* low, int h, int w, int num_chunks, int32_t* counts, int synchronize) {
    if (!side_ok(h, w)) return fail(ERR_ARG, "td_dataset_land_counts: needs 1 <= h, w <= 16384");
    if (num_chunks < 1 || num_chunks > TD_DATASET_MAX_CHUNKS || num_chunks > h || num_chunks > w)
        return fail(ERR_ARG, "td_dataset_land_counts: needs 1 <= num_chunks <= min(64, h, w)");
    if (!low || !counts) return fail(ERR_ARG, "td_dataset_land_counts: null buffer");
    if (!is_device_ptr(low) || !is_device_ptr(counts)) return fail(ERR_ARG, "td_dataset_land_counts: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    const int sh = h / num_chunks, sw = w / num_chunks;
    TD_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)num_chunks * num_chunks * sizeof(int32_t), st));
    unsigned per_chunk = blocks((long long)sh * sw, DS_THREADS * 8);      // about 8 pixels per thread
    per_chunk = per_chunk < 1 ? 1 : (per_chunk > 1024 ? 1024 : per_chunk);
    hipLaunchKernelGGL(ds_land_counts_kernel, dim3(per_chunk, (unsigned)(num_chunks * num_chunks)), dim3(DS_THREADS), 0, st, low, w, num_chunks,
                       sh, sw, counts);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_dataset_moments(void* hip_stream, const float* x, int C, int64_t n, int64_t* out_count, double* out_mean, double* out_m2,
                       int synchronize) {
    if (C < 1 || C > TD_DATASET_MAX_PLANES) return fail(ERR_ARG, "td_dataset_moments: needs 1 <= C <= 1024");
    if (n < 1 || n > TD_DATASET_MAX_ELEMENTS || (int64_t)C * n > ((int64_t)1 << 32))
        return fail(ERR_ARG, "td_dataset_moments: needs 1 <= n <= 2^30 and C * n <= 2^32");
    if (!x || !out_count || !out_mean || !out_m2) return fail(ERR_ARG, "td_dataset_moments: null buffer");
    if (!is_device_ptr(x) || !is_device_ptr(out_count) || !is_device_ptr(out_mean) || !is_device_ptr(out_m2))
        return fail(ERR_ARG, "td_dataset_moments: device buffers only");
    if (!aligned(out_count, 8) || !aligned(out_mean, 8) || !aligned(out_m2, 8)) return fail(ERR_ARG, "td_dataset_moments: outputs need 8-byte alignment");
    hipStream_t st = (hipStream_t)hip_stream;
    const unsigned all = blocks(n, DS_THREADS);
    const int B = (int)(all < (unsigned)DS_MOM_BLOCKS ? all : (unsigned)DS_MOM_BLOCKS);    // a function of n alone
    // scratch: the partial sums (C x B float64), the partial counts (B int64), the usable-position bytes (n, only for C > 1)
    const size_t part_bytes = round16((size_t)C * B * sizeof(double)), count_bytes = round16((size_t)B * sizeof(long long));
    void* scratch = nullptr;
    TD_HIP_TRY(hipMallocAsync(&scratch, part_bytes + count_bytes + (C > 1 ? (size_t)n : 0), st));
    double* part = (double*)scratch;
    long long* part_count = (long long*)((char*)scratch + part_bytes);
    unsigned char* usable = C > 1 ? (unsigned char*)scratch + part_bytes + count_bytes : nullptr;
    if (usable) hipLaunchKernelGGL(ds_usable_kernel, dim3(all), dim3(DS_THREADS), 0, st, x, C, (long long)n, usable);
    for (int centred = 0; centred < 2; ++centred) {
        hipLaunchKernelGGL(ds_moments_partial_kernel, dim3((unsigned)B, (unsigned)C), dim3(DS_THREADS), 0, st, x, (const unsigned char*)usable,
                           (long long)n, centred, (const double*)out_mean, part, part_count);
        hipLaunchKernelGGL(ds_moments_final_kernel, dim3((unsigned)C), dim3(DS_THREADS), 0, st, (const double*)part, (const long long*)part_count, B,
                           centred, (long long*)out_count, centred ? out_m2 : out_mean);
    }
    return finish(st, scratch, hipGetLastError(), synchronize);
}

}  // extern "C"
