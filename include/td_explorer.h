/*
 * td_explorer.h — C-ABI of the explorer views (libtd_explorer.so): what the reference's terrain explorer (terrain_diffusion/inference/
 * explorer/server.py: /api/coarse.png, /api/coarse_stats, /api/coarse_data.json, /api/detail.png, /api/detail_raw) and its random sampler
 * (inference/random_sampler.py: sample_land_tiles, get_coarse_climate_info) compute after WorldPipeline.coarse[...] / WorldPipeline.get(...).
 *
 * A library of its own, like td_relief.h, td_hydro.h and td_mc.h: the engine's sources stay the ones its committed profiles were collected
 * from (td_build_id).  Every call works on a CALLER-SUPPLIED HIP stream -- pass the engine's stream (td_engine_stream) to order it with the
 * engine's other work.  All buffers are device memory unless a parameter says "host".  With synchronize = 0 a call only enqueues (per-call
 * scratch comes from the stream-ordered pool, hipMallocAsync / hipFreeAsync, and goes back to it in stream order); with synchronize = 1 the
 * results are complete on return.
 * Conventions as in td_engine.h: plain C, 0 on success / negative code (TD_ERR_* values) on failure with a message in td_explorer_last_error().
 * Sizes: 1 <= H, W <= 2^16 and H W <= 2^26 pixels per call (TD_EXPLORER_MAX_PIXELS); flat pixel indices are int32.
 * Every result is bit-reproducible: minima and maxima are integer atomics on order-preserving keys, the tile list is an ordered compaction,
 * there are no floating-point atomics.  Arithmetic is IEEE fp32 without contraction unless a line below says float64.
 */
#ifndef TD_EXPLORER_H
#define TD_EXPLORER_H
#include <stdint.h>

#define TD_EXPLORER_MAX_SIDE (1 << 16)
#define TD_EXPLORER_MAX_PIXELS (1 << 26)
#define TD_EXPLORER_MAX_CHANNELS 8
#define TD_EXPLORER_MAX_FILTERS 8
#define TD_EXPLORER_MAX_HALF 2047   /* 4 half^2 < 2^24: the window count is exact in fp32 */

#ifdef __cplusplus
extern "C" {
#endif

const char* td_explorer_last_error(void);

/* sums (C + 1, H, W): the coarse stage's weighted sums with the weight plane last, 1 <= C <= 8.
 * out (C, H, W): v = sums[c] / (sums[C] + eps) -- eps = 1e-8 is the explorer's _coarse_channel, eps = 0 (nothing is added) the sampler's
 * normalize_tensor -- then v <- sign(v) v^2 (np.sign: 0 for +-0, NaN for NaN) for the channels c < n_signed_sq (0 <= n_signed_sq <= C; the
 * explorer's signed-sqrt elevation and p5: 2).  The division is the correctly rounded fp32 quotient, so out equals torch's on the CPU bit
 * for bit.
 * minmax (C, 2) or null: NaN-ignoring minimum and maximum of each out plane, from the same pass (np.nanmin / np.nanmax; NaN when a plane is
 * all NaN; a plane that holds -0.0 and +0.0 as extremes reports either zero). */
int td_explorer_channels(void* hip_stream, const float* sums, int C, int H, int W, int n_signed_sq, double eps, float* out, float* minmax,
                         int synchronize);

/* out (H, W, 4) uint8 RGBA of one field (H, W), as matplotlib colours it and plt.imsave quantises it:
 *   display    d = field, or log1pf(max(field, 0)) when log1p (evaluated as the float64 log1p rounded once to fp32);
 *   range      has_range: (vmin, vmax), finite with vmin < vmax.  Otherwise resolved on the device and consumed there without a host round
 *              trip: the NaN-ignoring minimum and maximum of d, vmax = vmin + 1 (in float64) when they are equal.
 *              range_out (2 floats, or null) receives the minimum and the maximum as found -- equal values mean that the + 1 rule applied --
 *              or (float)vmin, (float)vmax when has_range;
 *   normalise  matplotlib.colors.Normalize on an fp32 array: t = (float)((double)d - vmin), x = (float)((double)t / (vmax - vmin));
 *   lookup     lut: 256 x 3 fp32 rows; xa = x * 256.0f, xa == 256 -> 255, xa < 0 -> 0, xa >= 256 -> 255, else (int)xa; NaN -> RGBA (0, 0, 0, 0),
 *              every other pixel alpha 1;
 *   dimming    n_filters <= 8 planes (H, W): planes, lo, hi, use_lo, use_hi are HOST arrays of n_filters entries (planes: device pointers).  A
 *              pixel with !(plane >= (float)lo) for a used lower bound or !(plane <= (float)hi) for a used upper bound -- NaN fails, bounds
 *              rounded to fp32 as NumPy compares an fp32 array with a Python float -- gets rgb <- rgb * 0.3f; alpha is untouched;
 *   quantise   clip to [0, 1], (uint8)(c * 255.0f), truncating. */
int td_explorer_colorize(void* hip_stream, const float* field, int H, int W, int log1p, int has_range, double vmin, double vmax, const float* lut,
                         int n_filters, const float* const* planes, const double* lo, const double* hi, const int* use_lo, const int* use_hi,
                         uint8_t* out, float* range_out, int synchronize);

/* out (H, W, 4) uint8 = the same clip and truncation of rgb (H, W, 3) fp32 (a td_relief_map result), alpha 255.  A NaN channel is written
 * as 0: the reference's NumPy cast of NaN to uint8 is undefined. */
int td_explorer_quantize(void* hip_stream, const float* rgb, int H, int W, uint8_t* out, int synchronize);

/* The body of /api/detail_raw: out[0 .. 2 H W) = clip(floor(elev), -32768, 32767) as little-endian int16 -- a NaN elevation is written as 0,
 * td_mc_payload's convention; the reference's NumPy cast leaves it undefined -- then, when temp is not null, out[2 H W .. 6 H W) = the bytes
 * of temp (H, W) fp32, little-endian (at a 2-byte-aligned offset: H W may be odd).  out needs 2-byte alignment. */
int td_explorer_raw(void* hip_stream, const float* elev, const float* temp, int H, int W, uint8_t* out, int synchronize);

/* sample_land_tiles' search over elev_m (H, W) fp32 metres.  For every position (i, j), half <= i < H - half, half <= j < W - half, in row-major
 * order: c = the number of cells with elev_m > 0 (NaN is not land) in the window [i - half, i + half) x [j - half, j + half);
 * m = (float)c / (float)(4 half^2); the position is valid when (double)m >= min_land_frac -- torch's fp32 .mean().item() compared with a
 * Python float, NOT an exact fraction (half 5, 70 cells: m = 0.699999988 < 0.7).  half == 0 yields no position (the mean of an empty slice
 * is NaN).  0 <= half <= 2047 and 2 half <= H, W.
 * out_idx: the flat indices i W + j of the valid positions in ascending order, capacity (H - 2 half)(W - 2 half) int32 (may be null when that
 * is 0); out_count: 1 int32, their number.  The window counts come from two separable passes. */
int td_explorer_land_tiles(void* hip_stream, const float* elev_m, int H, int W, int half, double min_land_frac, int32_t* out_idx,
                           int32_t* out_count, int synchronize);

#ifdef __cplusplus
}
#endif
#endif
