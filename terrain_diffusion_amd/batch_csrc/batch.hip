// libtd_batch.so: the C-ABI of include/td_batch.h over the kernels of batch_kernels.hip.
#include "../side_csrc/td_side_host.h"
#include "../../include/td_batch.h"
#include "batch_kernels.hip"
#include <initializer_list>

using namespace td;

static_assert(sizeof(td_batch_group) == 48, "the group table is built by the binding as six 8-byte words per row");
static_assert(TD_BATCH_COND_LEN == 16 + 16 + 4 + 16 + 5 + 1, "the parts of the cond vector");

namespace {
// the checks every call over the two tables shares; null on success
const char* check_tables(const td_batch_group* groups, int G, const int32_t* items, int N) {
    if (G < 1 || G > TD_BATCH_MAX_GROUPS) return "needs 1 <= G <= 2^20";
    if (N < 1 || N > TD_BATCH_MAX_ITEMS) return "needs 1 <= N <= 65536";
    if (!groups || !items) return "null table";
    if (!is_device_ptr(groups) || !is_device_ptr(items)) return "device buffers only";
    return nullptr;
}
}  // namespace

extern "C" {

const char* td_batch_last_error(void) { return g_err.c_str(); }

int td_batch_views(void* hip_stream, const td_batch_group* groups, int G, const int32_t* items, int N, int plane, int origin, int offset,
                   int h, int w, int affine, float a, float b, float c, float* out, int synchronize) {
    if (const char* m = check_tables(groups, G, items, N)) return fail(ERR_ARG, std::string("td_batch_views: ") + m);
    if (plane < TD_BATCH_PLANE_LOWFREQ || plane > TD_BATCH_PLANE_RESIDUAL) return fail(ERR_ARG, "td_batch_views: plane must be 0, 1 or 2");
    if (origin < 0 || origin > 1 || affine < 0 || affine > 1) return fail(ERR_ARG, "td_batch_views: origin and affine must be 0 or 1");
    if (h < 1 || w < 1 || h > TD_BATCH_MAX_CROP || w > TD_BATCH_MAX_CROP || offset < -TD_BATCH_MAX_CROP || offset > TD_BATCH_MAX_CROP)
        return fail(ERR_ARG, "td_batch_views: needs 1 <= h, w <= 4096 and |offset| <= 4096");
    const long long total = (long long)N * h * w;
    if (total >= (1LL << 31)) return fail(ERR_ARG, "td_batch_views: needs N * h * w < 2^31");
    if (!out || !is_device_ptr(out)) return fail(ERR_ARG, "td_batch_views: out must be a device buffer");
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(ba_views_kernel, dim3(blocks(total, BA_THREADS)), dim3(BA_THREADS), 0, st, groups, G, (const int*)items, total, plane, origin,
                       offset, h, w, affine, a, b, c, out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_batch_latents(void* hip_stream, const td_batch_group* groups, int G, const int32_t* items, int N, int lc, int h, int w, int mode,
                     const void* noise, const float* mean, const float* std, float sigma_data, void* out, int synchronize) {
    if (const char* m = check_tables(groups, G, items, N)) return fail(ERR_ARG, std::string("td_batch_latents: ") + m);
    if (mode < 0 || mode > 1) return fail(ERR_ARG, "td_batch_latents: mode must be 0 or 1");
    if (lc < 1 || lc > 64 || h < 1 || w < 1 || h > TD_BATCH_MAX_CROP || w > TD_BATCH_MAX_CROP)
        return fail(ERR_ARG, "td_batch_latents: needs 1 <= lc <= 64 and 1 <= h, w <= 4096");
    const long long total = (long long)N * lc * h * w * (mode == 1 ? 8 : 1);      // threads; mode 1 writes eight halves per thread
    if (total * (mode == 1 ? 8 : 1) >= (1LL << 31)) return fail(ERR_ARG, "td_batch_latents: needs fewer than 2^31 output elements");
    if (!noise || !out || !is_device_ptr(noise) || !is_device_ptr(out)) return fail(ERR_ARG, "td_batch_latents: noise and out must be device buffers");
    hipStream_t st = (hipStream_t)hip_stream;
    if (mode == 0) {
        if (!mean || !std || !is_device_ptr(mean) || !is_device_ptr(std)) return fail(ERR_ARG, "td_batch_latents: mean and std must be device buffers");
        hipLaunchKernelGGL(ba_latents_f32_kernel, dim3(blocks(total, BA_THREADS)), dim3(BA_THREADS), 0, st, groups, G, (const int*)items, total, lc, h, w,
                           (const float*)noise, mean, std, sigma_data, (float*)out);
    } else {
        if ((uintptr_t)out & 15) return fail(ERR_ARG, "td_batch_latents: out needs 16-byte alignment in mode 1");
        hipLaunchKernelGGL(ba_latents_f16_kernel, dim3(blocks(total, BA_THREADS)), dim3(BA_THREADS), 0, st, groups, G, (const int*)items, total, lc, h, w,
                           (const _Float16*)noise, (_Float16*)out);
    }
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_batch_cond_image(void* hip_stream, const td_batch_group* groups, int G, const int32_t* items, int N, int crop, float dropout_p,
                        const float* u_drop, float max_noise, const float* u_noise, const float* z_mean, const float* z_p5,
                        const float* norm_mean, const float* norm_std, int raw, float* out, int synchronize) {
    if (const char* m = check_tables(groups, G, items, N)) return fail(ERR_ARG, std::string("td_batch_cond_image: ") + m);
    if (crop < 2 * TD_BATCH_HALO || crop > TD_BATCH_MAX_CROP || crop % TD_BATCH_HALO) return fail(ERR_ARG, "td_batch_cond_image: crop must be a multiple of 32 in 64 .. 4096");
    if (raw < 0 || raw > 1) return fail(ERR_ARG, "td_batch_cond_image: raw must be 0 or 1");
    if (!out || !is_device_ptr(out)) return fail(ERR_ARG, "td_batch_cond_image: out must be a device buffer");
    if (u_noise && (!z_mean || !z_p5)) return fail(ERR_ARG, "td_batch_cond_image: u_noise needs z_mean and z_p5");
    for (const float* p : {u_drop, u_noise, z_mean, z_p5})
        if (p && !is_device_ptr(p)) return fail(ERR_ARG, "td_batch_cond_image: device buffers only");
    if (!raw && (!norm_mean || !norm_std || !is_device_ptr(norm_mean) || !is_device_ptr(norm_std)))
        return fail(ERR_ARG, "td_batch_cond_image: norm_mean and norm_std must be device buffers unless raw");
    const int g = (crop + 2 * TD_BATCH_HALO) / TD_BATCH_HALO;
    const long long nblocks = (long long)N * g * g;
    if (nblocks >= (1LL << 31)) return fail(ERR_ARG, "td_batch_cond_image: needs N * g * g < 2^31");
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(ba_cond_image_kernel, dim3((unsigned)nblocks), dim3(BA_THREADS), 0, st, groups, G, (const int*)items, crop, dropout_p, u_drop,
                       max_noise, u_noise, z_mean, z_p5, norm_mean, norm_std, raw, out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_batch_cond_vector(void* hip_stream, const float* cond_img, int N, int g, const float* histogram_raw, const float* noise_level,
                         const float* z_replace, float sqrt12, float f0, float f1, float f2, float f3, float f4, float f5, float* out,
                         int32_t* nan_flags, int synchronize) {
    if (N < 1 || N > TD_BATCH_MAX_ITEMS) return fail(ERR_ARG, "td_batch_cond_vector: needs 1 <= N <= 65536");
    if (g < 4 || g > (TD_BATCH_MAX_CROP + 2 * TD_BATCH_HALO) / TD_BATCH_HALO) return fail(ERR_ARG, "td_batch_cond_vector: needs 4 <= g <= 130");
    for (const void* p : {(const void*)cond_img, (const void*)histogram_raw, (const void*)noise_level, (const void*)out, (const void*)nan_flags})
        if (!p || !is_device_ptr(p)) return fail(ERR_ARG, "td_batch_cond_vector: device buffers only");
    if (z_replace && !is_device_ptr(z_replace)) return fail(ERR_ARG, "td_batch_cond_vector: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    const BaFactors fac{{f0, f1, f2, f3, f4, f5}};
    hipLaunchKernelGGL(ba_cond_vector_kernel, dim3(blocks((long long)N * TD_BATCH_COND_LEN, BA_THREADS)), dim3(BA_THREADS), 0, st, cond_img, N, g,
                       histogram_raw, noise_level, z_replace, sqrt12, fac, out, (int*)nan_flags);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

}  // extern "C"
