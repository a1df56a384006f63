/*
 * td_dataset.h — C-ABI of the dataset-preparation library (libtd_dataset.so): the device half of what the reference does to a DEM before
 * its autoencoder sees it,
 *   process_single_file_base   terrain_diffusion/data/preprocessing/elevation_dataset.py:231-301: voids blended towards a low-resolution
 *                              base by Euclidean distance, the signed square root, the r x r block median (lowres_exact), the residual of
 *                              laplacian_encode (data/laplacian_encoder.py:63-91), the land share per sub-chunk,
 *   calculate_stats_welford    data/preprocessing/calculate_stds.py:7-71: the per-chunk summary its running mean / M2 update consumes.
 * terrain_diffusion_amd/dataset.py holds the host halves (the margin crop, the chunk list, the running statistics) and takes the low band
 * of laplacian_encode from the engine's resampler (td_resample2d).  Reading rasters, HDF5 and skimage's resize / gaussian stay with the
 * caller.
 *
 * Conventions as in td_relief.h: a library of its own beside libtd_engine.so, plain C, a CALLER-SUPPLIED HIP stream (pass td_engine_stream),
 * device buffers only, per-call scratch from the stream-ordered pool (hipMallocAsync / hipFreeAsync), synchronize = 0 only enqueues,
 * synchronize = 1 completes on return; 0 on success / negative code with a message in td_dataset_last_error().
 *
 * Every result is independent of the order the device visits pixels in: two calls on the same inputs give the same bits.
 */
#ifndef TD_DATASET_H
#define TD_DATASET_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TD_DATASET_MAX_SIDE 16384         /* 1 <= H, W <= 16384: flat indices stay below 2^31 */
#define TD_DATASET_MAX_RADIUS 64          /* td_dataset_fill_voids: 1 <= radius <= 64 */
#define TD_DATASET_MAX_BLOCK 32           /* td_dataset_block_median: 1 <= r <= 32 */
#define TD_DATASET_MAX_CHUNKS 64          /* td_dataset_land_counts: 1 <= num_chunks <= 64 */
#define TD_DATASET_MAX_PLANES 1024        /* td_dataset_moments: 1 <= C <= 1024 */
#define TD_DATASET_MAX_ELEMENTS (1 << 30) /* td_dataset_moments: 1 <= n <= 2^30 and C * n <= 2^32 */

const char* td_dataset_last_error(void);

/* out (H, W) fp32 = dem with its voids blended towards base (elevation_dataset.py:231-240, and :269 with signed_sqrt).  A void is a NaN
 * of dem.  A valid pixel keeps its bits.  A void p takes fp32((double)base[p] * min(1.0, d / radius)), d the exact Euclidean distance from
 * p to the nearest valid pixel -- the float64 sqrt of the integer squared distance, what scipy.ndimage.distance_transform_edt returns --;
 * the reference's radius is 32.  Only d < radius matters, so the search is capped at radius in both directions; an image without a valid
 * pixel comes out equal to base bit for bit.  signed_sqrt = 1 stores sign(v) * sqrtf(|v|) of every value v above (correctly rounded).
 * out_void_count (1 int32) receives the number of voids.  1 <= radius <= 64.  out must not overlap dem.
 * dem, base, out (H, W fp32), out_void_count: device buffers. */
int td_dataset_fill_voids(void* hip_stream, const float* dem, const float* base, int H, int W, int radius, int signed_sqrt, float* out,
                          int32_t* out_void_count, int synchronize);

/* out (H / r, W / r) fp32 = skimage.measure.block_reduce(x, (r, r), np.median) for H % r == W % r == 0, 1 <= r <= 32: the median of the
 * r^2 values of each block -- the middle value for odd r^2, fp32(a + b) * 0.5f of the two middle values for even r^2 (np.median of
 * float32; a median of zero is +0 whatever the zeros' signs, as np.median's mean gives it) --; a block that holds a NaN gives NaN.
 * x (H, W), out: device buffers; out must not overlap x. */
int td_dataset_block_median(void* hip_stream, const float* x, int H, int W, int r, float* out, int synchronize);

/* out (H, W) fp32 = x - up(low): the residual of laplacian_encode.  up is torch's upsample_bilinear2d of low (h, w) to (H, W) with
 * align_corners=False, evaluated per pixel in fp32 without contraction: per axis scale = fp32(n_in) / fp32(n_out),
 * src = max(scale * (dst + 0.5f) - 0.5f, 0), i0 = min(int(src), n_in - 1), i1 = i0 + (i0 < n_in - 1), w1 = src - i0, w0 = 1 - w1, and
 * up = wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * d) over the taps a = low[i0, j0], b = low[i0, j1], c = low[i1, j0],
 * d = low[i1, j1].  The upsampled plane is never written.  out may be x itself.  1 <= h, w <= 16384.
 * x, out (H, W), low (h, w): device buffers. */
int td_dataset_residual(void* hip_stream, const float* x, const float* low, int H, int W, int h, int w, float* out, int synchronize);

/* counts[ch * num_chunks + cw] (int32) = the number of low > 0 (false for NaN) in sub-chunk (ch, cw): rows ch * sh .. ch * sh + sh - 1
 * and columns cw * sw .. cw * sw + sw - 1 of low (h, w), sh = h / num_chunks, sw = w / num_chunks (integer division; what is left over at
 * the far edges belongs to no sub-chunk, elevation_dataset.py:273-289).  1 <= num_chunks <= min(64, h, w).
 * low (h, w fp32), counts (num_chunks^2 int32): device buffers. */
int td_dataset_land_counts(void* hip_stream, const float* low, int h, int w, int num_chunks, int32_t* counts, int synchronize);

/* The chunk summary of calculate_stats_welford: x is C planes of n fp32 values; a position counts where NO plane holds a NaN
 * (calculate_stds.py:49; for C = 1 simply the non-NaN values).  out_count (1 int64) = the number of such positions, out_mean (C float64)
 * their mean per plane, out_m2 (C float64) the sum of (x - mean)^2 per plane.  All sums in float64, in two device passes (the sum, then
 * the centred squares) without a host synchronisation between them, through a fixed reduction tree.  count = 0 leaves mean and m2 at 0.
 * 1 <= C <= 1024, 1 <= n <= 2^30, C * n <= 2^32.  x, out_count, out_mean, out_m2: device buffers. */
int td_dataset_moments(void* hip_stream, const float* x, int C, int64_t n, int64_t* out_count, double* out_mean, double* out_m2,
                       int synchronize);

#ifdef __cplusplus
}
#endif
#endif
