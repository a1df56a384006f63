// libtd_hydro.so: the C-ABI of include/td_hydro.h over the kernels of hydro_kernels.hip.
#include "../side_csrc/td_side_host.h"
#include "../../include/td_hydro.h"
#include "hydro_kernels.hip"

using namespace td;

namespace {
enum { ERR_CONVERGE = -3 };
constexpr long long MAX_SIDE = 1LL << 20, MAX_CELLS_D8 = (1LL << 31) - 1, MAX_CELLS_ACC = 1LL << 24;
// d8 and fill: 1 <= H, W <= 2^20, H W < 2^31; accumulation and indicator: H W <= 2^24 (upstream counts stay exact in fp32)
bool size_ok(int H, int W, long long max_cells) {
    return H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE && (long long)H * W <= max_cells;
}
constexpr int FILL_BATCH = 8;   // passes enqueued between two reads of the convergence flags
}  // namespace

extern "C" {

const char* td_hydro_last_error(void) { return g_err.c_str(); }

int td_hydro_d8(void* hip_stream, const float* z, int H, int W, double tol, int32_t* receiver, uint8_t* kmax, uint8_t* is_sink, int synchronize) {
    if (!size_ok(H, W, MAX_CELLS_D8)) return fail(ERR_ARG, "td_hydro_d8: needs 1 <= H, W <= 2^20 and H * W < 2^31");
    if (!is_device_ptr(z) || !is_device_ptr(receiver) || !is_device_ptr(kmax) || !is_device_ptr(is_sink))
        return fail(ERR_ARG, "td_hydro_d8: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(hydro_d8_kernel, dim3(blocks((long long)H * W, HYDRO_THREADS)), dim3(HYDRO_THREADS), 0, st, z, H, W, (float)tol, receiver, kmax, is_sink);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_hydro_accumulate(void* hip_stream, const float* z, int H, int W, const int32_t* receiver, const uint8_t* is_sink, float* acc,
                        uint32_t* bad_edges, int synchronize) {
    if (!size_ok(H, W, MAX_CELLS_ACC)) return fail(ERR_ARG, "td_hydro_accumulate: needs 1 <= H, W and H * W <= 2^24");
    if (!is_device_ptr(z) || !is_device_ptr(receiver) || !is_device_ptr(is_sink) || !is_device_ptr(acc) || !is_device_ptr(bad_edges))
        return fail(ERR_ARG, "td_hydro_accumulate: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    const int N = H * W;
    // scratch: the per-cell (count, pending) words and the counted-edge successors, from the stream-ordered pool
    void* scratch = nullptr;
    TD_HIP_TRY(hipMallocAsync(&scratch, (size_t)N * 12, st));
    unsigned long long* word = (unsigned long long*)scratch;
    int32_t* next = (int32_t*)(word + N);
    hipError_t err = hipMemsetAsync(bad_edges, 0, sizeof(uint32_t), st);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(hydro_acc_init_kernel, dim3(blocks(N, HYDRO_THREADS)), dim3(HYDRO_THREADS), 0, st, z, N, word);
        hipLaunchKernelGGL(hydro_acc_edges_kernel, dim3(blocks(N, HYDRO_THREADS)), dim3(HYDRO_THREADS), 0, st, z, N, receiver, is_sink, next, word, (unsigned*)bad_edges);
        hipLaunchKernelGGL(hydro_acc_walk_kernel, dim3(blocks(N, HYDRO_THREADS)), dim3(HYDRO_THREADS), 0, st, N, (const int32_t*)next, word);
        hipLaunchKernelGGL(hydro_acc_out_kernel, dim3(blocks(N, HYDRO_THREADS)), dim3(HYDRO_THREADS), 0, st, N, (const unsigned long long*)word, acc);
        err = hipGetLastError();
    }
    return finish(st, scratch, err, synchronize);
}

int td_hydro_indicator(void* hip_stream, const float* acc, int H, int W, int k, float* out, int synchronize) {
    if (!size_ok(H, W, MAX_CELLS_ACC)) return fail(ERR_ARG, "td_hydro_indicator: needs 1 <= H, W and H * W <= 2^24");
    if (k < 1 || H / k < 1 || W / k < 1) return fail(ERR_ARG, "td_hydro_indicator: needs 1 <= k <= min(H, W)");
    if (!is_device_ptr(acc) || !is_device_ptr(out)) return fail(ERR_ARG, "td_hydro_indicator: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    const int Ho = H / k, Wo = W / k;
    hipLaunchKernelGGL(hydro_indicator_kernel, dim3(blocks((long long)Ho * Wo, HYDRO_THREADS)), dim3(HYDRO_THREADS), 0, st, acc, W, k, Ho, Wo, out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_hydro_fill(void* hip_stream, const float* h, int H, int W, double epsilon, int connectivity, int has_nodata, double nodata, float* out,
                  int* passes) {
    if (!size_ok(H, W, MAX_CELLS_D8)) return fail(ERR_ARG, "td_hydro_fill: needs 1 <= H, W <= 2^20 and H * W < 2^31");
    if (!(epsilon >= 0.0)) return fail(ERR_ARG, "td_hydro_fill: epsilon must be >= 0 (a negative one makes the reference's result depend on heap order)");
    if (!is_device_ptr(h) || !is_device_ptr(out)) return fail(ERR_ARG, "td_hydro_fill: device buffers only");
    if (h == out) return fail(ERR_ARG, "td_hydro_fill: out must not alias h");
    hipStream_t st = (hipStream_t)hip_stream;
    const long long N = (long long)H * W;
    const int conn8 = connectivity == 4 ? 0 : 1;   // as in the reference: anything but 4 means 8
    const float eps = (float)epsilon, nd = (float)nodata;
    const int ntx = (W + FILL_TILE - 1) / FILL_TILE, nty = (H + FILL_TILE - 1) / FILL_TILE;
    const size_t ntiles = (size_t)ntx * nty;
    // scratch: hw (N floats), two tile-flag planes, FILL_BATCH + 1 pass flags
    void* scratch = nullptr;
    TD_HIP_TRY(hipMallocAsync(&scratch, (size_t)N * 4 + 2 * ntiles * 4 + (FILL_BATCH + 1) * 4, st));
    float* hw = (float*)scratch;
    unsigned* tiles = (unsigned*)(hw + N);
    unsigned* flags = tiles + 2 * ntiles;
    unsigned host_flags[FILL_BATCH + 1];
    const long long max_passes = N + 2;   // every pass that changes something completes at least one more step of some cell's flood path
    long long done = 0, converged_at = -1;
    hipLaunchKernelGGL(hydro_fill_init_kernel, dim3(blocks(N, HYDRO_THREADS)), dim3(HYDRO_THREADS), 0, st, h, H, W, conn8, has_nodata ? 1 : 0, nd, out, hw);
    hipError_t err = hipGetLastError();
    while (err == hipSuccess && converged_at < 0 && done < max_passes) {
        err = hipMemsetAsync(flags, 0, (FILL_BATCH + 1) * 4, st);
        for (int p = 0; p < FILL_BATCH && err == hipSuccess; ++p) {
            const long long g = done + p;
            hipLaunchKernelGGL(hydro_fill_pass_kernel, dim3(ntx, nty), dim3(HYDRO_THREADS), 0, st, out, (const float*)hw, H, W, eps, conn8,
                               g == 0 ? (const unsigned*)nullptr : (const unsigned*)(tiles + ((g - 1) & 1) * ntiles), tiles + (g & 1) * ntiles,
                               p == 0 ? (const unsigned*)nullptr : (const unsigned*)(flags + p - 1), flags + p);
            err = hipGetLastError();
        }
        if (err == hipSuccess) err = hipMemcpyAsync(host_flags, flags, FILL_BATCH * 4, hipMemcpyDeviceToHost, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        if (err == hipSuccess) {
            for (int p = 0; p < FILL_BATCH; ++p)
                if (host_flags[p] == 0u) { converged_at = done + p + 1; break; }
            done += FILL_BATCH;
        }
    }
    if (err == hipSuccess && converged_at >= 0) {
        hipLaunchKernelGGL(hydro_fill_out_kernel, dim3(blocks(N, HYDRO_THREADS)), dim3(HYDRO_THREADS), 0, st, h, (size_t)N, has_nodata ? 1 : 0, nd, out);
        err = hipGetLastError();
    }
    if (const int rc = finish(st, scratch, err, 1)) return rc;   // always synchronises: converged_at and *passes are read on the host
    if (converged_at < 0) return fail(ERR_CONVERGE, "td_hydro_fill: no convergence within H * W + 2 passes");
    if (passes) *passes = (int)(converged_at > 0x7fffffff ? 0x7fffffff : converged_at);
    return OK;
}

}  // extern "C"
