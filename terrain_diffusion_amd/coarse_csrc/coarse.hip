// libtd_coarse.so: the C-ABI of include/td_coarse.h over the kernels of coarse_kernels.hip.
#include "../side_csrc/td_side_host.h"
#include "../../include/td_coarse.h"
#include "coarse_kernels.hip"
#include <initializer_list>

using namespace td;

static_assert(CO_MAX_TILE == TD_COARSE_MAX_TILE, "one block holds a whole tile or crop");
static_assert(TD_COARSE_MAX_FACTOR <= CO_MAX_TILE, "a thread of the block mean holds one row of a block");
static_assert((long long)TD_COARSE_MAX_SIDE * TD_COARSE_MAX_SIDE <= (1LL << 26), "the solver indexes its planes with int");

namespace {
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}
size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }

// the largest iteration limit a level of N pixels can have: n <= N unknowns
int host_limit(int maxiter, long long N) {
    if (maxiter > 0) return maxiter;
    const int dflt = (int)(10.0 * sqrt((double)N));
    return dflt > 50 ? dflt : 50;
}

struct CgBuffers {
    unsigned char* code;
    double *x, *r, *z, *p[2], *q, *part[4];
};

// One level: the system of `a` (H, W), the CG loop from x (null: zeros; else the plane bufs.x already holds), the finish into `out`.
// Two launches per iteration; with `synchronize` the stop flag is read every `chunk` iterations and the loop left once it is set.
hipError_t solve_level(hipStream_t st, const double* a, int H, int W, bool have_x0, double tol, int maxiter, int chunk, int synchronize,
                       const CgBuffers& b, CoState* state, double* out, int32_t* info) {
    const int N = H * W;
    const unsigned nb = blocks(N, CO_THREADS);
    const int B = (int)(nb < (unsigned)CO_CG_BLOCKS ? nb : (unsigned)CO_CG_BLOCKS);       // a function of the shape alone
    hipError_t err = hipSuccess;
    if (!have_x0) err = hipMemsetAsync(b.x, 0, (size_t)N * sizeof(double), st);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(co_cg_setup_kernel, dim3(B), dim3(CO_THREADS), 0, st, a, have_x0 ? (const double*)b.x : (const double*)nullptr, H, W, b.code,
                       b.r, b.z, b.part[0], b.part[1], b.part[2], b.part[3]);
    hipLaunchKernelGGL(co_cg_begin_kernel, dim3(1), dim3(CO_THREADS), 0, st, (const double*)b.part[0], (const double*)b.part[3], B, tol, maxiter, state);
    const int limit = host_limit(maxiter, N);
    for (int it = 0; it < limit; ++it) {
        hipLaunchKernelGGL(co_cg_pass1_kernel, dim3(B), dim3(CO_THREADS), 0, st, it, H, W, (const unsigned char*)b.code, (const double*)b.z,
                           (const double*)b.p[(it + 1) & 1], b.p[it & 1], b.q, (const double*)b.part[1], (const double*)b.part[2], b.part[0], B, state);
        hipLaunchKernelGGL(co_cg_pass2_kernel, dim3(B), dim3(CO_THREADS), 0, st, it, N, (const unsigned char*)b.code, (const double*)b.p[it & 1],
                           (const double*)b.q, b.x, b.r, b.z, (const double*)b.part[0], b.part[1], b.part[2], B, state);
        if (synchronize && (it + 1) % chunk == 0 && it + 1 < limit) {
            int flag = 0;
            if ((err = hipGetLastError()) != hipSuccess) return err;
            if ((err = hipMemcpyAsync(&flag, &state->flag, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return err;
            if ((err = hipStreamSynchronize(st)) != hipSuccess) return err;
            if (flag) break;
        }
    }
    hipLaunchKernelGGL(co_cg_far_kernel, dim3(B), dim3(CO_THREADS), 0, st, N, (const unsigned char*)b.code, (const double*)b.x, (const CoState*)state,
                       b.part[3]);
    hipLaunchKernelGGL(co_cg_finish_kernel, dim3(B), dim3(CO_THREADS), 0, st, N, (const unsigned char*)b.code, (const double*)b.x, a,
                       (const CoState*)state, (const double*)b.part[3], B, out, info);
    return hipGetLastError();
}
}  // namespace

extern "C" {

const char* td_coarse_last_error(void) { return g_err.c_str(); }

int td_coarse_area_resize_w(void* hip_stream, const float* x, int H, int W_in, int W_out, int load_rule, float* out, int synchronize) {
    if (H < 1 || W_in < 1 || W_in > TD_COARSE_MAX_WIDTH || W_out < 1 || W_out > W_in || (long long)H * W_in >= (1LL << 31))
        return fail(ERR_ARG, "td_coarse_area_resize_w: needs H >= 1, 1 <= W_out <= W_in <= 65536 and H * W_in < 2^31");
    if (load_rule < 0 || load_rule > 3) return fail(ERR_ARG, "td_coarse_area_resize_w: load_rule must be 0, 1, 2 or 3");
    if (!x || !out) return fail(ERR_ARG, "td_coarse_area_resize_w: null buffer");
    if (!is_device_ptr(x) || !is_device_ptr(out)) return fail(ERR_ARG, "td_coarse_area_resize_w: device buffers only");
    if (overlap(x, (size_t)H * W_in * sizeof(float), out, (size_t)H * W_out * sizeof(float))) return fail(ERR_ARG, "td_coarse_area_resize_w: out overlaps x");
    hipStream_t st = (hipStream_t)hip_stream;
    const long long total = (long long)H * W_out;
    hipLaunchKernelGGL(co_area_resize_kernel, dim3(blocks(total, CO_THREADS)), dim3(CO_THREADS), 0, st, x, total, W_in, W_out, load_rule, out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_coarse_tile_stats(void* hip_stream, const float* x, int Hs, int Ws, int t, double q, float* out_mean, float* out_nanmean,
                         float* out_quantile, int synchronize) {
    if (Hs < 1 || Ws < 1 || Hs > TD_COARSE_MAX_WIDTH || Ws > TD_COARSE_MAX_WIDTH || (long long)Hs * Ws >= (1LL << 31))
        return fail(ERR_ARG, "td_coarse_tile_stats: needs 1 <= Hs, Ws <= 65536 and Hs * Ws < 2^31");
    if (t < 1 || t > TD_COARSE_MAX_TILE || t > Hs || t > Ws) return fail(ERR_ARG, "td_coarse_tile_stats: needs 1 <= t <= min(32, Hs, Ws)");
    if (!(q >= 0.0 && q <= 1.0)) return fail(ERR_ARG, "td_coarse_tile_stats: needs 0 <= q <= 1");
    if (!x) return fail(ERR_ARG, "td_coarse_tile_stats: null buffer");
    if (!out_mean && !out_nanmean && !out_quantile) return fail(ERR_ARG, "td_coarse_tile_stats: no output asked for");
    if (!is_device_ptr(x)) return fail(ERR_ARG, "td_coarse_tile_stats: device buffers only");
    const int Ht = Hs / t, Wt = Ws / t;
    const size_t in_bytes = (size_t)Hs * Ws * sizeof(float), out_bytes = (size_t)Ht * Wt * sizeof(float);
    for (const float* o : {out_mean, out_nanmean, out_quantile}) {
        if (!o) continue;
        if (!is_device_ptr(o)) return fail(ERR_ARG, "td_coarse_tile_stats: device buffers only");
        if (overlap(x, in_bytes, o, out_bytes)) return fail(ERR_ARG, "td_coarse_tile_stats: an output overlaps x");
    }
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(co_tile_stats_kernel, dim3((unsigned)((long long)Ht * Wt)), dim3(CO_THREADS), 0, st, x, Ws, t, Wt, q, out_mean, out_nanmean,
                       out_quantile);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_coarse_crop_scores(void* hip_stream, const float* plane, int H, int W, float mean0, float std0, const int32_t* offsets, int N, int c,
                          float* out, int synchronize) {
    if (H < 1 || W < 1 || H > TD_COARSE_MAX_WIDTH || W > TD_COARSE_MAX_WIDTH || (long long)H * W >= (1LL << 31))
        return fail(ERR_ARG, "td_coarse_crop_scores: needs 1 <= H, W <= 65536 and H * W < 2^31");
    if (c < 3 || c > TD_COARSE_MAX_TILE || c > H || c > W) return fail(ERR_ARG, "td_coarse_crop_scores: needs 3 <= c <= min(32, H, W)");
    if (N < 1 || N > (1 << 20)) return fail(ERR_ARG, "td_coarse_crop_scores: needs 1 <= N <= 2^20");
    if (!plane || !offsets || !out) return fail(ERR_ARG, "td_coarse_crop_scores: null buffer");
    if (!is_device_ptr(plane) || !is_device_ptr(offsets) || !is_device_ptr(out)) return fail(ERR_ARG, "td_coarse_crop_scores: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(co_crop_scores_kernel, dim3((unsigned)N), dim3(CO_THREADS), 0, st, plane, H, W, mean0, std0, (const int*)offsets, c, out);
    return finish(st, nullptr, hipGetLastError(), synchronize);
}

int td_coarse_fill_oceans_chunked(void* hip_stream, const double* a, int H, int W, double tol, int maxiter, int multires_factor, int chunk,
                                  double* out, int32_t* info, int synchronize) {
    if (H < 1 || W < 1 || H > TD_COARSE_MAX_SIDE || W > TD_COARSE_MAX_SIDE) return fail(ERR_ARG, "td_coarse_fill_oceans: needs 1 <= H, W <= 8192");
    if (multires_factor < 1 || multires_factor > TD_COARSE_MAX_FACTOR) return fail(ERR_ARG, "td_coarse_fill_oceans: needs 1 <= multires_factor <= 32");
    if (!(tol >= 0.0)) return fail(ERR_ARG, "td_coarse_fill_oceans: tol must not be negative");
    if (maxiter < 0) return fail(ERR_ARG, "td_coarse_fill_oceans: maxiter must not be negative (0: the default per level)");
    if (chunk < 1) return fail(ERR_ARG, "td_coarse_fill_oceans: chunk must be at least 1");
    if (!a || !out || !info) return fail(ERR_ARG, "td_coarse_fill_oceans: null buffer");
    if (!is_device_ptr(a) || !is_device_ptr(out) || !is_device_ptr(info)) return fail(ERR_ARG, "td_coarse_fill_oceans: device buffers only");
    const size_t N = (size_t)H * W, bytes = N * sizeof(double);
    if (out != a && overlap(a, bytes, out, bytes)) return fail(ERR_ARG, "td_coarse_fill_oceans: out overlaps a without being a");
    if (((uintptr_t)a | (uintptr_t)out) & 7) return fail(ERR_ARG, "td_coarse_fill_oceans: a and out need 8-byte alignment");
    hipStream_t st = (hipStream_t)hip_stream;
    const int f = multires_factor, Hc = (H + f - 1) / f, Wc = (W + f - 1) / f;
    const size_t Nc = (size_t)Hc * Wc;
    // scratch: six float64 planes (x, r, z, p, p', q: the coarse level uses their heads), the coarse plane and its filled form, the code bytes,
    // four rows of partials, the two states
    const size_t plane = round256(bytes), cplane = round256(Nc * sizeof(double)), parts = round256(CO_CG_BLOCKS * sizeof(double));
    const size_t total = 6 * plane + 2 * cplane + round256(N) + 4 * parts + round256(2 * sizeof(CoState));
    void* scratch = nullptr;
    TD_HIP_TRY(hipMallocAsync(&scratch, total, st));
    char* at = (char*)scratch;
    CgBuffers b;
    b.x = (double*)at; at += plane;
    b.r = (double*)at; at += plane;
    b.z = (double*)at; at += plane;
    b.p[0] = (double*)at; at += plane;
    b.p[1] = (double*)at; at += plane;
    b.q = (double*)at; at += plane;
    double* coarse = (double*)at; at += cplane;
    double* coarse_filled = (double*)at; at += cplane;
    b.code = (unsigned char*)at; at += round256(N);
    for (int k = 0; k < 4; ++k) { b.part[k] = (double*)at; at += parts; }
    CoState* states = (CoState*)at;
    hipLaunchKernelGGL(co_block_nanmean_kernel, dim3(blocks((long long)Nc, CO_THREADS)), dim3(CO_THREADS), 0, st, a, H, W, f, Hc, Wc, coarse);
    hipError_t err = solve_level(st, coarse, Hc, Wc, false, tol, maxiter, chunk, synchronize, b, states, coarse_filled, info);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(co_zoom_kernel, dim3(blocks((long long)N, CO_THREADS)), dim3(CO_THREADS), 0, st, (const double*)coarse_filled, Hc, Wc, a, H, W,
                           b.x);
        err = solve_level(st, a, H, W, true, tol, maxiter, chunk, synchronize, b, states + 1, out, info + 2);
    }
    return finish(st, scratch, err, synchronize);
}

int td_coarse_fill_oceans(void* hip_stream, const double* a, int H, int W, double tol, int maxiter, int multires_factor, double* out,
                          int32_t* info, int synchronize) {
    return td_coarse_fill_oceans_chunked(hip_stream, a, H, W, tol, maxiter, multires_factor, TD_COARSE_DEFAULT_CHUNK, out, info, synchronize);
}

}  // extern "C"
