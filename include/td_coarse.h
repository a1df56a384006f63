/*
 * td_coarse.h — C-ABI of the coarse-dataset library (libtd_coarse.so): the device half of what the reference does to build the data of its
 * coarse model (terrain_diffusion/training/datasets/coarse_dataset.py),
 *   CoarseDataset.__init__   :253-347: latitude bands shrunk in width by F.interpolate(mode='area'), 26 x 26 tiles reduced to a mean, a 5 %
 *                            quantile or a NaN-ignoring mean, the oceans of the climate layers filled by fill_oceans (:17-220), a Laplace
 *                            inpainting solved by Jacobi-preconditioned CG from a coarse-grid start,
 *   CoarseDataset.__getitem__ :396-403: the score of a candidate crop, a 0.9 quantile of its squared 3 x 3 blur residual.
 * terrain_diffusion_amd/coarse_dataset.py holds the host halves (the band rows, the assembly of the bands, the moments).  Reading rasters and
 * HDF5, the CoarseDataset class and its host RNG calls stay with the caller.
 *
 * Conventions as in td_dataset.h: a library of its own beside libtd_engine.so, plain C, a CALLER-SUPPLIED HIP stream (pass td_engine_stream),
 * device buffers only, per-call scratch from the stream-ordered pool (hipMallocAsync / hipFreeAsync), synchronize = 0 only enqueues,
 * synchronize = 1 completes on return; 0 on success / negative code with a message in td_coarse_last_error().
 *
 * Every result is independent of the order the device visits elements in: two calls on the same inputs give the same bits.  Floating sums use
 * no atomics: partial sums go through a fixed tree.
 */
#ifndef TD_COARSE_H
#define TD_COARSE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TD_COARSE_MAX_WIDTH 65536         /* td_coarse_area_resize_w: 1 <= W_out <= W_in <= 65536, H * W_in < 2^31 */
#define TD_COARSE_MAX_TILE 32             /* td_coarse_tile_stats: 1 <= t <= 32; td_coarse_crop_scores: 3 <= c <= 32 */
#define TD_COARSE_MAX_SIDE 8192           /* td_coarse_fill_oceans: 1 <= H, W <= 8192 */
#define TD_COARSE_MAX_FACTOR 32           /* td_coarse_fill_oceans: 1 <= multires_factor <= 32 */
#define TD_COARSE_DEFAULT_CHUNK 32        /* td_coarse_fill_oceans: CG iterations enqueued between two reads of the stop flag */

const char* td_coarse_last_error(void);

/* out (H, W_out) fp32 = F.interpolate(x[None, None], size=(H, W_out), mode='area') of x (H, W_in): the mean of the window
 * [floor(j W_in / W_out), ceil((j + 1) W_in / W_out)) of its row for output column j (64-bit integer arithmetic), summed from the left in fp32
 * and divided by the fp32 window length; a NaN in the window gives NaN.  load_rule is applied to every value as it is read: 0 none;
 * 1 |x - 32768| < 1e-6 -> NaN (the int16 no-data value, coarse_dataset.py:305-307); 2 |x| > 1e6 -> NaN (:309); 3 sign(x) sqrtf(|x|),
 * correctly rounded (:266).  1 <= W_out <= W_in <= 65536, H >= 1, H * W_in < 2^31.  x, out: device buffers; out must not overlap x. */
int td_coarse_area_resize_w(void* hip_stream, const float* x, int H, int W_in, int W_out, int load_rule, float* out, int synchronize);

/* Statistics of the (Hs / t) x (Ws / t) whole t x t tiles of x (Hs, Ws) fp32 (integer division; rows and columns beyond the last whole tile
 * belong to none, :284-285), n = t^2 values each.  Each output is (Hs / t, Ws / t) fp32 and may be null:
 *   out_mean      the float64 sum in a fixed order divided by n, rounded once to fp32; a NaN in the tile gives NaN;
 *   out_nanmean   the same over the non-NaN values; a tile without one gives NaN;
 *   out_quantile  numpy's `linear` quantile: r = q (n - 1) in float64, k = floor(r), the order statistics k and min(k + 1, n - 1) -- found exactly,
 *                 by counted ranks with an index tie-break -- interpolated in float64, a + (b - a) (r - k), and rounded once; a NaN in the tile
 *                 gives NaN.  0 <= q <= 1.
 * 1 <= t <= min(32, Hs, Ws), Hs, Ws <= 65536.  x and the outputs: device buffers; the outputs must not overlap x. */
int td_coarse_tile_stats(void* hip_stream, const float* x, int Hs, int Ws, int t, double q, float* out_mean, float* out_nanmean,
                         float* out_quantile, int synchronize);

/* out[n] (fp32) = the crop score of coarse_dataset.py:396-403 for the c x c crop at row offsets[2 n], column offsets[2 n + 1] of the normalised
 * channel-0 plane (H, W), all in fp32 without contraction: s = v std0 + mean0; e = s^2 where s > 0, 0 where s <= 0 (sign(s) s^2 with its
 * negatives set to 0), NaN for NaN; d = e - (the sum of the up to nine e of the 3 x 3 neighbourhood inside the crop, row-major) / 9;
 * the 0.9 quantile of d^2 with torch.quantile's rank fp32(fp32(0.9) fp32(c^2 - 1)), its fraction g in fp32 and torch's lerp
 * (g < 0.5: a + g (b - a), else b - (b - a) (1 - g)); a NaN in the crop gives NaN.  3 <= c <= min(32, H, W), 1 <= N <= 2^20; the offsets are
 * device data and are not read back: a crop that leaves the plane reads nothing and gives NaN.
 * plane (H, W fp32; H, W <= 65536, H * W < 2^31), offsets (N x 2 int32), out (N fp32): device buffers. */
int td_coarse_crop_scores(void* hip_stream, const float* plane, int H, int W, float mean0, float std0, const int32_t* offsets, int N, int c,
                          float* out, int synchronize);

/* out (H, W) float64 = fill_oceans(a, tol=tol, maxiter=maxiter or None, multires_factor=multires_factor) of coarse_dataset.py:17-220 without
 * anchors, the whole of it on the device: the NaN mask; the NaN-aware block mean of means (:176-184) with NaN padding to a multiple of the
 * factor; the coarse solve from x0 = 0; scipy.ndimage.zoom(order=1, mode='nearest') of the coarse result back to (H, W) as the start of the
 * fine solve; the fine solve; the np.allclose(., 0) -> 1e-9 rule (:160-161) on both levels.  The operator is matrix-free: the diagonal is the
 * count of in-image neighbours, ocean neighbours contribute -1, land neighbours go to b, off-image neighbours are omitted.  CG is scipy's:
 * the stop test |r|_2 < max(tol, 1e-5 |b|_2), strict, at the top of every iteration; b = 0 returns zeros; the Jacobi preconditioner; the
 * iteration limit ends the loop without a final test.  maxiter = 0 is the reference's default per level, max(50, int(10 sqrt(n))) for n
 * unknowns.  Land pixels keep their bits; an input without NaN comes out unchanged.  All ocean gives 1e-9 everywhere; a coarse level without
 * ocean is solved in no iteration (the reference does the same).
 * info (4 int32): coarse iterations, coarse scipy `info`, fine iterations, fine `info` -- `info` is 0, or the iteration limit when the limit
 * ended the loop.  Two plain launches per iteration; the iteration limit and the stop flag live in device memory and every kernel returns at
 * once when the flag is set.  With synchronize = 1 the host enqueues TD_COARSE_DEFAULT_CHUNK iterations at a time and reads the flag between
 * chunks; with synchronize = 0 it enqueues up to the largest limit the shape allows without reading anything back.  Result and counts do not
 * depend on the chunk length.  tol >= 0, maxiter >= 0, 1 <= H, W <= 8192, 1 <= multires_factor <= 32.
 * a, out (H, W float64), info: device buffers; out may be a itself. */
int td_coarse_fill_oceans(void* hip_stream, const double* a, int H, int W, double tol, int maxiter, int multires_factor, double* out,
                          int32_t* info, int synchronize);

/* td_coarse_fill_oceans with the chunk length given: chunk >= 1 iterations between two reads of the stop flag. */
int td_coarse_fill_oceans_chunked(void* hip_stream, const double* a, int H, int W, double tol, int maxiter, int multires_factor, int chunk,
                                  double* out, int32_t* info, int synchronize);

#ifdef __cplusplus
}
#endif
#endif
