/*
 * td_rivers.h — C-ABI of the river-map library (libtd_rivers.so): the two pieces of the reference that draw a map with its rivers on it,
 *   get_relief_map WITH its biome, flow and rgb inputs (terrain_diffusion/inference/relief_map.py:64-199), and
 *   smooth_river_bumps (terrain_diffusion/inference/postprocessing.py:87-135).
 * The relief picture is rendered by the kernels of libtd_relief.so (relief_csrc/relief_kernels.hip is compiled into both libraries; the
 * shade kernel is one template, and with rgb, biome and flow all null td_rivers_relief gives td_relief_map's bits).
 *
 * Like td_relief.h and td_hydro.h: a library of its own, on a CALLER-SUPPLIED HIP stream (pass the engine's, td_engine_stream), all buffers
 * device memory, per-call scratch from the stream-ordered pool (hipMallocAsync / hipFreeAsync).  With synchronize = 0 a call only enqueues;
 * with synchronize = 1 the results are complete on return.  Plain C, 0 on success / negative code (TD_ERR_* values) on failure with a message
 * in td_rivers_last_error(); null buffers, host pointers and shapes out of range are refused, never dereferenced.
 */
#ifndef TD_RIVERS_H
#define TD_RIVERS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* td_rivers_last_error(void);

/* out (H, W, 3) fp32 = the reference's relief picture of elev (H, W) fp32 with its overlays.  elev ... fill are td_relief_map's arguments
 * (td_relief.h) with the same meaning and limits (2 <= H, W <= 2^20, 0 <= rl, rs <= 64).  The overlays, each left out when its pointer is null:
 *   rgb      (H, W, 3) fp32: the base colour in place of the terrain colormap.  The colormap, its range reduction and has_range / vmin / vmax
 *            are then skipped entirely;
 *   biome    (H, W) int32 with palette 31 x 3 fp32: where clip(biome, 0, 30) > 0 the base colour is palette[clip(biome, 0, 30)], on top of
 *            rgb too (palette may be null when biome is);
 *   shading  as td_relief_map: clip(base * (relief * (0.35 + 0.65 hs) + 1 - relief), 0, 1); pixels whose elevation is NaN become NaN;
 *   flow     (H, W) fp32: where flow > fl32(flow_threshold) each channel becomes fl32(0.25) * shaded + fl32(0.75) * (0.100, 0.450, 0.850)
 *            (two rounded products and one add).  The threshold is ROUNDED TO fp32 before the comparison: that is how NumPy >= 2 compares
 *            a float32 array with a Python float.  A NaN flow draws nothing; a river on a NaN pixel stays NaN;
 *   ocean    the ocean ramp where the filled elevation is below 0, applied last: it overwrites rivers, as in the reference.
 * All arithmetic per pixel is fp32 in the reference's order, without contraction. */
int td_rivers_relief(void* hip_stream, const float* elev, int H, int W, const float* lut, const float* wl, int rl, const float* ws, int rs,
                     double azimuth_deg, double resolution, double relief, int has_range, double vmin, double vmax, int has_fill, double fill,
                     const float* rgb, const int32_t* biome, const float* palette, const float* flow, double flow_threshold, float* out,
                     int synchronize);

/* out (H, W) fp32 = smooth_river_bumps(h, slope_thresh, smooth_strength, iterations) of h (H, W) fp32; 2 <= H, W <= 2^20, H * W < 2^31,
 * 0 <= iterations <= 64 (0 copies h).  out must not overlap h.  Each iteration, all fp32 in the reference's order, no contraction,
 * correctly rounded division and square root, the precise device exp:
 *   hs = h with NaN -> 0;  gy, gx = np.gradient(hs) (central differences inside, one-sided at the image's edges, NOT wrapped);
 *   slope = sqrt(gx gx + gy gy);  the four neighbours WRAP around the image (np.roll) and count only where they are not NaN:
 *   lap = (((up + dn) + lf) + rt) - cnt * hs;  w = exp(-(slope / fl32(slope_thresh))^2);  h += (fl32(smooth_strength) * w) * lap.
 * NaN cells stay NaN and contribute 0.  One launch per iteration (8 bytes per pixel each) between out and one scratch plane. */
int td_rivers_smooth(void* hip_stream, const float* h, int H, int W, double slope_thresh, double smooth_strength, int iterations, float* out,
                     int synchronize);

#ifdef __cplusplus
}
#endif
#endif
