/*
 * td_spectrum.h — C-ABI of the spectrum library (libtd_spectrum.so): the device half of the reference's beauty score,
 *   calculate_beauty_score      terrain_diffusion/data/preprocessing/beauty_score.py:52-87: laplacian_decode, sign(d) d^2, the share of
 *                               pixels <= 0, the clamp at 0, torch.std,
 *   analyze_terrain_frequency   beauty_score.py:9-50: the 2-D FFT of a real plane, log|F|, its mean over radial bins.
 * terrain_diffusion_amd/beauty.py holds the host halves (the bin map, built once per shape with the reference's own expressions, the seven
 * features, the linear model, the class rule of h5_latents_dataset.py:107).  HDF5 and the plots stay with the caller.
 *
 * Conventions as in td_dataset.h: a library of its own beside libtd_engine.so, plain C, a CALLER-SUPPLIED HIP stream (pass td_engine_stream),
 * device buffers only, per-call scratch from the stream-ordered pool (hipMallocAsync / hipFreeAsync), synchronize = 0 only enqueues,
 * synchronize = 1 completes on return; 0 on success / negative code with a message in td_spectrum_last_error().  No rocFFT / hipFFT: the
 * transform is the library's own.
 *
 * Every entry point takes B planes (B, H, W) of fp32.  Every result is independent of the order the device visits pixels in: counts are
 * integers, float64 sums go through a fixed tree, and there is no floating-point atomic, so two calls on the same inputs give the same bits.
 */
#ifndef TD_SPECTRUM_H
#define TD_SPECTRUM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TD_SPECTRUM_MIN_SIDE 8            /* td_spectrum_fft2: H and W are powers of two in 8 .. 4096 */
#define TD_SPECTRUM_MAX_SIDE 4096         /* every entry point: 1 <= H, W <= 4096 */
#define TD_SPECTRUM_MAX_BATCH 1024        /* 1 <= B <= 1024 */
#define TD_SPECTRUM_MAX_BINS 64           /* td_spectrum_radial_bins: 1 <= bins <= 64 */
#define TD_SPECTRUM_NO_BIN 255            /* a position of the bin map that belongs to no bin */
#define TD_SPECTRUM_ERR_SIZE -3           /* td_spectrum_fft2: H or W is not a power of two in 8 .. 4096 */

const char* td_spectrum_last_error(void);

/* The head of calculate_beauty_score for B chunks: d = residual + up(lowfreq), up torch's upsample_bilinear2d of lowfreq (h, w) to (H, W)
 * with align_corners=False, evaluated per pixel in fp32 without contraction exactly as td_dataset_residual states it (td_dataset.h); then
 * v = sign(d) * fp32(d * d).  out_nonpos[b] (int32) = the number of v <= 0 (exact).  out (B, H, W) = v with negatives replaced by 0.
 * out_mean[b], out_m2[b] (float64) = the mean of out's plane b and its sum of (out - mean)^2, float64 sums in two passes through a fixed
 * tree; out_std[b] (fp32) = sqrt(m2 / (H W - 1)) in float64, rounded once: torch.std's unbiased estimate.  A NaN stays a NaN throughout
 * and counts as positive.  1 <= h, w, H, W <= 4096, H W >= 2.
 * lowfreq (B, h, w), residual and out (B, H, W), out_nonpos, out_mean, out_m2, out_std (B): device buffers; out must not overlap the inputs. */
int td_spectrum_decode(void* hip_stream, const float* lowfreq, const float* residual, int B, int H, int W, int h, int w, float* out,
                       int32_t* out_nonpos, double* out_mean, double* out_m2, float* out_std, int synchronize);

/* The 2-D DFT of B real planes, unnormalised, F[u, v] = sum x[r, c] exp(-2 pi i (u r / H + v c / W)) (torch.fft.fft2).  H and W are each a
 * power of two in 8 .. 4096, not necessarily equal; any other size returns TD_SPECTRUM_ERR_SIZE.  Both outputs are optional (NULL = not
 * written), at least one is needed:
 *   out_half (B, H, W / 2 + 1) interleaved complex fp32 (re, im): the half spectrum, torch.fft.rfft2's layout;
 *   out_logabs (B, H, W) fp32: log|F| at every position in torch's unshifted index order, the columns beyond W / 2 by Hermitian symmetry.
 *     |F| is taken in float64 (no overflow, no flush), the logarithm too, and the result is rounded once; an exact zero gives -inf.
 * Radix-2 butterflies in fp32 with twiddles whose cos and sin are computed in float64 and rounded once; no fast-math function anywhere.
 * x, out_half, out_logabs: device buffers; the outputs must not overlap x. */
int td_spectrum_fft2(void* hip_stream, const float* x, int B, int H, int W, float* out_half, float* out_logabs, int synchronize);

/* The bin means of analyze_terrain_frequency: logabs (B, H, W) fp32 and bin_map (H, W) uint8, the bin of every position or
 * TD_SPECTRUM_NO_BIN (shared by the planes; values >= bins belong to no bin).  out_counts[b * bins + k] (int32) = the number of positions
 * of bin k, out_means[b * bins + k] (fp32) = their mean, the sum in float64 through a fixed tree, divided in float64 and rounded once;
 * +-inf and NaN propagate as IEEE arithmetic has them; an empty bin gives 0.0 (beauty_score.py:47-48).  1 <= bins <= 64.
 * logabs, bin_map, out_counts, out_means: device buffers. */
int td_spectrum_radial_bins(void* hip_stream, const float* logabs, const uint8_t* bin_map, int B, int H, int W, int bins,
                            int32_t* out_counts, float* out_means, int synchronize);

#ifdef __cplusplus
}
#endif
#endif
