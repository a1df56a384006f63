// libtd_spectrum.so: the C-ABI of include/td_spectrum.h over the kernels of spectrum_kernels.hip.
#include "../side_csrc/td_side_host.h"
#include "../../include/td_spectrum.h"
#include "spectrum_kernels.hip"

#include <mutex>

using namespace td;

static_assert(SP_MAX_N == TD_SPECTRUM_MAX_SIDE, "the row pass holds one transform of the longest side in LDS");
static_assert(SP_MAX_BINS == TD_SPECTRUM_MAX_BINS, "the bin counts of a block live in LDS");
static_assert(SP_TILE >= 2 * SP_MAX_N && SP_TILE * sizeof(float2) <= 64 * 1024, "a column tile holds two columns at least, in 64 KiB at most");
static_assert(SP_MAX_BINS * SP_BIN_THREADS * sizeof(double) <= 64 * 1024, "the bin slots of a block fit the LDS of a workgroup");

namespace {
enum { ERR_SIZE = TD_SPECTRUM_ERR_SIZE };
bool side_ok(int H, int W) { return H >= 1 && W >= 1 && H <= TD_SPECTRUM_MAX_SIDE && W <= TD_SPECTRUM_MAX_SIDE; }
bool batch_ok(int B) { return B >= 1 && B <= TD_SPECTRUM_MAX_BATCH; }
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}
size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }
int log2_of(int n) {                                       // the exponent of a power of two in 8 .. 4096, -1 for anything else
    for (int b = 3; b <= 12; ++b)
        if (n == 1 << b) return b;
    return -1;
}
unsigned sum_blocks(size_t n, int threads) {                // a function of n alone: the tree of a sum is fixed by the sizes
    const size_t all = (n + threads - 1) / threads;
    return (unsigned)(all < (size_t)SP_SUM_BLOCKS ? all : (size_t)SP_SUM_BLOCKS);
}

// exp(-2 pi i k / 4096), k = 0 .. 2047: cos and sin in float64, rounded once; the quarter points are exact
const float2* twiddles() {
    static float2 table[SP_TW];
    static std::once_flag once;
    std::call_once(once, [] {
        const double step = 2.0 * 3.14159265358979323846 / (double)SP_MAX_N;
        for (int k = 0; k < SP_TW; ++k) table[k] = make_float2((float)cos(step * k), (float)-sin(step * k));
        table[0] = make_float2(1.f, 0.f);
        table[SP_TW / 2] = make_float2(0.f, -1.f);
    });
    return table;
}
}  // namespace

extern "C" {

const char* td_spectrum_last_error(void) { return g_err.c_str(); }

int td_spectrum_decode(void* hip_stream, const float* lowfreq, const float* residual, int B, int H, int W, int h, int w, float* out,
                       int32_t* out_nonpos, double* out_mean, double* out_m2, float* out_std, int synchronize) {
    if (!batch_ok(B)) return fail(ERR_ARG, "td_spectrum_decode: needs 1 <= B <= 1024");
    if (!side_ok(H, W) || !side_ok(h, w) || (size_t)H * W < 2) return fail(ERR_ARG, "td_spectrum_decode: needs 1 <= H, W, h, w <= 4096 and H W >= 2");
    if (!lowfreq || !residual || !out || !out_nonpos || !out_mean || !out_m2 || !out_std) return fail(ERR_ARG, "td_spectrum_decode: null buffer");
    if (!is_device_ptr(lowfreq) || !is_device_ptr(residual) || !is_device_ptr(out) || !is_device_ptr(out_nonpos) || !is_device_ptr(out_mean) ||
        !is_device_ptr(out_m2) || !is_device_ptr(out_std))
        return fail(ERR_ARG, "td_spectrum_decode: device buffers only");
    const size_t n = (size_t)H * W, bytes = (size_t)B * n * sizeof(float);
    if (overlap(residual, bytes, out, bytes) || overlap(lowfreq, (size_t)B * h * w * sizeof(float), out, bytes))
        return fail(ERR_ARG, "td_spectrum_decode: out overlaps an input");
    hipStream_t st = (hipStream_t)hip_stream;
    const unsigned nb = sum_blocks(n, SP_THREADS);
    void* scratch = nullptr;                              // the partial sums, B x nb float64
    TD_HIP_TRY(hipMallocAsync(&scratch, (size_t)B * nb * sizeof(double), st));
    double* part = (double*)scratch;
    hipError_t err = hipMemsetAsync(out_nonpos, 0, (size_t)B * sizeof(int32_t), st);
    if (err == hipSuccess) {
        const float sy = (float)h / (float)H, sx = (float)w / (float)W;
        hipLaunchKernelGGL(sp_decode_kernel, dim3(nb, (unsigned)B), dim3(SP_THREADS), 0, st, lowfreq, residual, H, W, h, w, sy, sx, out,
                           (int*)out_nonpos, part);
        hipLaunchKernelGGL(sp_moments_final_kernel, dim3((unsigned)B), dim3(SP_THREADS), 0, st, (const double*)part, (int)nb, (double)n, 0, out_mean,
                           out_m2, out_std);
        hipLaunchKernelGGL(sp_centred_kernel, dim3(nb, (unsigned)B), dim3(SP_THREADS), 0, st, (const float*)out, n, (const double*)out_mean, part);
        hipLaunchKernelGGL(sp_moments_final_kernel, dim3((unsigned)B), dim3(SP_THREADS), 0, st, (const double*)part, (int)nb, (double)n, 1, out_mean,
                           out_m2, out_std);
        err = hipGetLastError();
    }
    return finish(st, scratch, err, synchronize);
}

int td_spectrum_fft2(void* hip_stream, const float* x, int B, int H, int W, float* out_half, float* out_logabs, int synchronize) {
    if (!batch_ok(B)) return fail(ERR_ARG, "td_spectrum_fft2: needs 1 <= B <= 1024");
    const int hbits = log2_of(H), wbits = log2_of(W);
    if (hbits < 0 || wbits < 0) return fail(ERR_SIZE, "td_spectrum_fft2: H and W must each be a power of two in 8 .. 4096");
    if (!x || (!out_half && !out_logabs)) return fail(ERR_ARG, "td_spectrum_fft2: null input, or neither output asked for");
    if (!is_device_ptr(x) || (out_half && !is_device_ptr(out_half)) || (out_logabs && !is_device_ptr(out_logabs)))
        return fail(ERR_ARG, "td_spectrum_fft2: device buffers only");
    const int Wh = W / 2 + 1;
    const size_t in_bytes = (size_t)B * H * W * sizeof(float), half_bytes = (size_t)B * H * Wh * sizeof(float2);
    if ((out_half && overlap(x, in_bytes, out_half, half_bytes)) || (out_logabs && overlap(x, in_bytes, out_logabs, in_bytes)) ||
        (out_half && out_logabs && overlap(out_half, half_bytes, out_logabs, in_bytes)))
        return fail(ERR_ARG, "td_spectrum_fft2: an output overlaps x or the other output");
    hipStream_t st = (hipStream_t)hip_stream;
    // scratch: the twiddle table, and the row spectra where the caller has no use for the half spectrum
    const size_t tw_bytes = round16(SP_TW * sizeof(float2));
    void* scratch = nullptr;
    TD_HIP_TRY(hipMallocAsync(&scratch, tw_bytes + (out_half ? 0 : half_bytes), st));
    float2* tw = (float2*)scratch;
    float2* rows = out_half ? (float2*)out_half : (float2*)((char*)scratch + tw_bytes);
    hipError_t err = hipMemcpyAsync(tw, twiddles(), SP_TW * sizeof(float2), hipMemcpyHostToDevice, st);   // pageable and static: staged before return
    if (err == hipSuccess) {
        int cols = SP_TILE / H;
        cols = cols > SP_MAX_COLS ? SP_MAX_COLS : cols;
        hipLaunchKernelGGL(sp_fft_rows_kernel, dim3((unsigned)(H / 2), (unsigned)B), dim3(SP_THREADS), 0, st, x, H, W, wbits, (const float2*)tw, rows);
        hipLaunchKernelGGL(sp_fft_cols_kernel, dim3(blocks(Wh, cols), (unsigned)B), dim3(SP_THREADS), 0, st, (const float2*)rows, H, W, hbits, cols,
                           (const float2*)tw, out_half ? rows : (float2*)nullptr, out_logabs);
        err = hipGetLastError();
    }
    return finish(st, scratch, err, synchronize);
}

int td_spectrum_radial_bins(void* hip_stream, const float* logabs, const uint8_t* bin_map, int B, int H, int W, int bins,
                            int32_t* out_counts, float* out_means, int synchronize) {
    if (!batch_ok(B)) return fail(ERR_ARG, "td_spectrum_radial_bins: needs 1 <= B <= 1024");
    if (!side_ok(H, W)) return fail(ERR_ARG, "td_spectrum_radial_bins: needs 1 <= H, W <= 4096");
    if (bins < 1 || bins > TD_SPECTRUM_MAX_BINS) return fail(ERR_ARG, "td_spectrum_radial_bins: needs 1 <= bins <= 64");
    if (!logabs || !bin_map || !out_counts || !out_means) return fail(ERR_ARG, "td_spectrum_radial_bins: null buffer");
    if (!is_device_ptr(logabs) || !is_device_ptr(bin_map) || !is_device_ptr(out_counts) || !is_device_ptr(out_means))
        return fail(ERR_ARG, "td_spectrum_radial_bins: device buffers only");
    hipStream_t st = (hipStream_t)hip_stream;
    const int n = H * W;                                  // <= 2^24
    const unsigned nb = sum_blocks((size_t)n, SP_BIN_THREADS * 8);        // about 8 positions per thread
    void* scratch = nullptr;                              // the partial sums, B x nb x bins float64
    TD_HIP_TRY(hipMallocAsync(&scratch, (size_t)B * nb * bins * sizeof(double), st));
    double* part = (double*)scratch;
    hipError_t err = hipMemsetAsync(out_counts, 0, (size_t)B * bins * sizeof(int32_t), st);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(sp_bins_partial_kernel, dim3(nb, (unsigned)B), dim3(SP_BIN_THREADS), (size_t)bins * SP_BIN_THREADS * sizeof(double), st,
                           logabs, (const unsigned char*)bin_map, n, bins, part, (int*)out_counts);
        hipLaunchKernelGGL(sp_bins_final_kernel, dim3((unsigned)B), dim3(SP_BIN_THREADS), 0, st, (const double*)part, (int)nb, bins,
                           (const int*)out_counts, out_means);
        err = hipGetLastError();
    }
    return finish(st, scratch, err, synchronize);
}

}  // extern "C"
