// libtd_objective.so: the C-ABI of include/td_objective.h over the kernels of objective_kernels.hip.
#include "../side_csrc/td_side_host.h"
#include "../../include/td_objective.h"
#include "objective_kernels.hip"
#include <initializer_list>

using namespace td;

namespace {
// the shape checks every call over (N, C, H, W) shares; null on success.  `planes` is the channel count of the widest tensor of the call.
const char* check_shape(int N, int C, int H, int W, int planes) {
    if (N < 1 || N > TD_OBJECTIVE_MAX_ITEMS) return "needs 1 <= N <= 65536";
    if (C < 1 || planes > TD_OBJECTIVE_MAX_CHANNELS) return "needs 1 <= C and at most 1024 channels";
    if (H < 1 || W < 1 || H > TD_OBJECTIVE_MAX_SIDE || W > TD_OBJECTIVE_MAX_SIDE) return "needs 1 <= H, W <= 65536";
    if ((long long)N * planes * H * W >= (1LL << 31)) return "needs fewer than 2^31 elements per tensor";
    return nullptr;
}

bool all_device(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (!p || !is_device_ptr(p)) return false;
    return true;
}

bool aligned16(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if ((uintptr_t)p & 15) return false;
    return true;
}
}  // namespace

extern "C" {

const char* td_objective_last_error(void) { return g_err.c_str(); }

int td_objective_levels(void* hip_stream, int mode, const float* in, int N, float P_mean, float P_std, float sigma_data, const float* images,
                        int C, int H, int W, const int32_t* channels_host, int n_channels, float eps, float* table, int synchronize) {
    if (mode < TD_OBJECTIVE_MODE_DRAW || mode > TD_OBJECTIVE_MODE_T) return fail(ERR_ARG, "td_objective_levels: mode must be 0, 1 or 2");
    if (N < 1 || N > TD_OBJECTIVE_MAX_ITEMS) return fail(ERR_ARG, "td_objective_levels: needs 1 <= N <= 65536");
    if (n_channels < 0 || n_channels > TD_OBJECTIVE_MAX_LIST) return fail(ERR_ARG, "td_objective_levels: at most 64 listed channels");
    if (!all_device({in, table})) return fail(ERR_ARG, "td_objective_levels: in and table must be device buffers");
    ObList ch{};
    if (mode == TD_OBJECTIVE_MODE_DRAW && n_channels > 0) {
        if (const char* m = check_shape(N, C, H, W, C)) return fail(ERR_ARG, std::string("td_objective_levels: ") + m);
        if (!channels_host) return fail(ERR_ARG, "td_objective_levels: null channel list");
        if (is_device_ptr(channels_host)) return fail(ERR_ARG, "td_objective_levels: channels_host must be a host array");
        if (!all_device({images})) return fail(ERR_ARG, "td_objective_levels: images must be a device buffer");
        ch.n = n_channels;
        for (int k = 0; k < n_channels; ++k) {
            if (channels_host[k] < 0 || channels_host[k] >= C) return fail(ERR_ARG, "td_objective_levels: a listed channel is outside 0 .. C - 1");
            ch.v[k] = channels_host[k];
        }
    }
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(ob_levels_kernel, dim3((unsigned)N), dim3(OB_THREADS), 0, st, mode, in, P_mean, P_std, sigma_data, images, C,
                       (long long)H * W, ch, eps, table);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_objective_noise(void* hip_stream, const float* images, const float* noise, const float* cond_img, const float* table, int N, int C,
                       int Cc, int H, int W, float sigma_data, float* x, float* v, int synchronize) {
    if (Cc < 0) return fail(ERR_ARG, "td_objective_noise: Cc must be >= 0");
    if (const char* m = check_shape(N, C, H, W, C + Cc)) return fail(ERR_ARG, std::string("td_objective_noise: ") + m);
    if (!all_device({images, noise, table, x, v})) return fail(ERR_ARG, "td_objective_noise: device buffers only");
    if ((Cc > 0) != (cond_img != nullptr)) return fail(ERR_ARG, "td_objective_noise: cond_img goes with Cc > 0");
    if (cond_img && !is_device_ptr(cond_img)) return fail(ERR_ARG, "td_objective_noise: device buffers only");
    const unsigned HW = (unsigned)((long long)H * W);                  // below 2^31: check_shape
    const bool vec = HW % 4 == 0 && aligned16({images, noise, x, v}) && (!cond_img || aligned16({cond_img}));
    hipStream_t st = (hipStream_t)hip_stream;
    const unsigned per = vec ? HW / 4 : HW;
    const dim3 grid(blocks(per, OB_THREADS), (unsigned)(C + Cc), (unsigned)(N < 65535 ? N : 65535));
    if (vec)
        hipLaunchKernelGGL(ob_noise_kernel<4>, grid, dim3(OB_THREADS), 0, st, images, noise, cond_img, table, N, C, Cc, HW, sigma_data, x, v);
    else
        hipLaunchKernelGGL(ob_noise_kernel<1>, grid, dim3(OB_THREADS), 0, st, images, noise, cond_img, table, N, C, Cc, HW, sigma_data, x, v);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_objective_logvar(void* hip_stream, const float* table, int N, const float* freqs, const float* phases, const float* weight, int K,
                        int n_logvar, float* logvar, int synchronize) {
    if (n_logvar != 1) return fail(ERR_ARG, "td_objective_logvar: n_logvar must be 1 (the reference's reshape(-1, 1, 1, 1) only broadcasts for 1)");
    if (N < 1 || N > TD_OBJECTIVE_MAX_ITEMS) return fail(ERR_ARG, "td_objective_logvar: needs 1 <= N <= 65536");
    if (K < 1 || K > TD_OBJECTIVE_MAX_LOGVAR) return fail(ERR_ARG, "td_objective_logvar: needs 1 <= K <= 1024");
    if (!all_device({table, freqs, phases, weight, logvar})) return fail(ERR_ARG, "td_objective_logvar: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(ob_logvar_kernel, dim3((unsigned)N), dim3(64), 0, st, table, freqs, phases, weight, K, logvar);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_objective_sqerr(void* hip_stream, const float* out, const float* v, int N, int C, int H, int W, float sigma_data, double* S,
                       int synchronize) {
    if (const char* m = check_shape(N, C, H, W, C)) return fail(ERR_ARG, std::string("td_objective_sqerr: ") + m);
    if (!all_device({out, v, S})) return fail(ERR_ARG, "td_objective_sqerr: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(ob_sqerr_kernel, dim3((unsigned)((long long)N * C)), dim3(OB_THREADS), 0, st, out, v, (long long)H * W, sigma_data, S);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_objective_loss(void* hip_stream, const double* S, const float* logvar, int N, int C, int H, int W, float sigma_data, int form,
                      const int32_t* groups_host, int n_groups, double* item_loss, double* loss64, float* loss32, int synchronize) {
    if (form < TD_OBJECTIVE_LOSS_WEIGHTED || form > TD_OBJECTIVE_LOSS_GROUPED) return fail(ERR_ARG, "td_objective_loss: form must be 0, 1 or 2");
    if (const char* m = check_shape(N, C, H, W, C)) return fail(ERR_ARG, std::string("td_objective_loss: ") + m);
    if (!all_device({S, item_loss, loss64, loss32})) return fail(ERR_ARG, "td_objective_loss: device buffers only");
    if (form == TD_OBJECTIVE_LOSS_WEIGHTED && !all_device({logvar})) return fail(ERR_ARG, "td_objective_loss: the weighted form needs a device logvar");
    ObList groups{};
    if (form == TD_OBJECTIVE_LOSS_GROUPED) {
        if (!groups_host || n_groups < 1 || n_groups > TD_OBJECTIVE_MAX_LIST) return fail(ERR_ARG, "td_objective_loss: the grouped form needs 1 .. 64 group sizes");
        if (is_device_ptr(groups_host)) return fail(ERR_ARG, "td_objective_loss: groups_host must be a host array");
        long long sum = 0;
        groups.n = n_groups;
        for (int k = 0; k < n_groups; ++k) {
            if (groups_host[k] < 1) return fail(ERR_ARG, "td_objective_loss: a group size below 1");
            groups.v[k] = groups_host[k];
            sum += groups_host[k];
        }
        if (sum != C) return fail(ERR_ARG, "td_objective_loss: the group sizes do not sum to C");
    }
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(ob_loss_kernel, dim3(1), dim3(OB_THREADS), 0, st, S, logvar, N, C, (long long)H * W, sigma_data, form, groups, item_loss, loss64,
                       loss32);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_objective_terrain_u8(void* hip_stream, const float* terrain, int N, int C, int H, int W, uint8_t* out, int synchronize) {
    if (const char* m = check_shape(N, C, H, W, 3 * C)) return fail(ERR_ARG, std::string("td_objective_terrain_u8: ") + m);
    if (!all_device({terrain, out})) return fail(ERR_ARG, "td_objective_terrain_u8: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    float* mm = nullptr;
    TD_HIP_TRY(hipMallocAsync((void**)&mm, sizeof(float) * 2 * N, st));
    const unsigned HW = (unsigned)((long long)H * W);                  // below 2^31: check_shape
    hipLaunchKernelGGL(ob_minmax_kernel, dim3((unsigned)N), dim3(OB_THREADS), 0, st, terrain, (long long)C * HW, mm);
    const bool vec = HW % 4 == 0 && aligned16({terrain}) && !((uintptr_t)out & 3);
    const dim3 grid(blocks(vec ? HW / 4 : HW, OB_THREADS), (unsigned)C, (unsigned)(N < 65535 ? N : 65535));
    if (vec)
        hipLaunchKernelGGL(ob_u8_kernel<4>, grid, dim3(OB_THREADS), 0, st, terrain, mm, N, C, HW, out);
    else
        hipLaunchKernelGGL(ob_u8_kernel<1>, grid, dim3(OB_THREADS), 0, st, terrain, mm, N, C, HW, out);
    return finish(st, mm, hipGetLastError(), synchronize);
}

}  // extern "C"
