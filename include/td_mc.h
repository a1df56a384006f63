/*
 * td_mc.h — C-ABI of the Minecraft terrain library (libtd_mc.so): the per-request tail of the reference's Minecraft terrain server
 * (terrain_diffusion/inference/minecraft_api.py: _get_upsampled, _compute_climate_vars, _classify_biome, _binary_response) and of its REST
 * server's scaled path (api.py: _get_terrain), on fp32 data that WorldPipeline.get returned.
 *
 * A library of its own, like td_relief.h and td_hydro.h: the engine's sources stay the ones its committed profiles were collected from
 * (td_build_id).  Every call works on a CALLER-SUPPLIED HIP stream -- pass the engine's stream (td_engine_stream) to order it with the engine's
 * other work.  All buffers are device memory.  With synchronize = 0 a call only enqueues; with synchronize = 1 the results are complete on
 * return.  No call allocates scratch.
 * Conventions as in td_engine.h: plain C, 0 on success / negative code (TD_ERR_* values) on failure with a message in td_mc_last_error().
 * Sizes: 1 <= H, W <= 2^16 and H W <= 2^26 output pixels per call (TD_MC_MAX_PIXELS).
 */
#ifndef TD_MC_H
#define TD_MC_H
#include <stdint.h>

#define TD_MC_MAX_SIDE (1 << 16)
#define TD_MC_MAX_PIXELS (1 << 26)

#ifdef __cplusplus
extern "C" {
#endif

const char* td_mc_last_error(void);

/* out (C, H, W) = rows [r0, r0 + H) x columns [c0, c0 + W) of F.interpolate(src (C, Hn, Wn), scale_factor=scale, mode="bilinear",
 * align_corners=False), i.e. of the (C, Hn scale, Wn scale) image, which is never materialised: 0 <= r0, r0 + H <= Hn scale, likewise for
 * columns; 1 <= scale <= 1024, 1 <= C <= 64.  Per output pixel, torch's source index fma(fl32(1 / scale), u + 0.5, -0.5) clamped below at 0,
 * the index clamped to Hn - 1 and no +1 neighbour on the last row / column; the weighted sum is taken in float64 and rounded once.  scale 1
 * copies.  Covers the elevation crop, its 1-pixel padded copy, the climate crop and api.py's 1-pixel-padded variant. */
int td_mc_upsample(void* hip_stream, const float* src, int C, int Hn, int Wn, int scale, long long r0, long long c0, int H, int W, float* out,
                   int synchronize);

/* One fused pass over an H x W box whose first pixel sits at absolute (row i0, column j0):
 *   elev (H, W) at row pitch elev_ld (>= W): the classifier's elevation and the detail noise's elev_smooth;
 *   elev_padded (H + 2, W + 2): its Sobel (3 x 3, weights / 8) gives the detail noise's slope factor and the classifier's slope;
 *   climate (n_climate, H, W) or null: fewer than 4 channels (or null) make every pixel plains (id 1);
 *   noise_planes (7, H, W) or null: the noise values of the reference's seven generators in its order (_TEMP_NOISE, _TEMP_NOISE_FINE,
 *   _PRECIP_NOISE, _SNOW_NOISE, _SNOW_NOISE_FINE, _ELEV_NOISE_COARSE, _ELEV_NOISE_FINE); null evaluates the built-in FBm Perlin noise at
 *   x = j0 + column, y = i0 + row (fp32), whose values are this library's own.
 * elev_out (H, W) or null: elev + (n_coarse amp_coarse + n_fine amp_fine) * (elev >= 0) when noise_scale > 0, else elev, with
 *   slope_factor = clamp(|Sobel| / fl32(40 detail_pixel_size_m / 90), 0, 1)^1.5, amp = slope_factor * fl32(noise_scale * 100 | 70)
 *   * fl32(detail_pixel_size_m) / fl32(native_resolution) (_get_upsampled);
 * biome_out (H, W) int16 or null: _classify_biome with pixel_size_m = biome_pixel_size_m.
 * Every mask is evaluated as the reference writes it, so NaN inputs give the reference's ids. */
int td_mc_finish(void* hip_stream, const float* elev, long long elev_ld, const float* elev_padded, const float* climate, int n_climate, int H,
                 int W, long long i0, long long j0, const float* noise_planes, double noise_scale, double detail_pixel_size_m,
                 double native_resolution, double biome_pixel_size_m, float* elev_out, int16_t* biome_out, int synchronize);

/* out (7, H, W) = the built-in noise planes of the box at absolute (i0, j0), in the generator order of td_mc_finish: the values td_mc_finish
 * uses when it is given no planes. */
int td_mc_noise(void* hip_stream, int H, int W, long long i0, long long j0, float* out, int synchronize);

/* The body of _binary_response: out[0 .. H W) = clip(floor(elev), -32768, 32767) as int16 (a NaN elevation is written as 0; the reference's
 * NumPy cast leaves it undefined), then, when biome is not null, out[H W .. 2 H W) = biome.  Little-endian on the device and the host. */
int td_mc_payload(void* hip_stream, const float* elev, const int16_t* biome, int H, int W, int16_t* out, int synchronize);

#ifdef __cplusplus
}
#endif
#endif
