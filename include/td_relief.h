/*
 * td_relief.h — C-ABI of the shaded-relief renderer (libtd_relief.so): get_relief_map of the reference
 * (terrain_diffusion/inference/relief_map.py:64-199) with biome, flow and rgb None, the path every caller of it uses
 * (inference/explorer/server.py:203-227, inference/random_sampler.py:175, the evaluation scripts).
 *
 * The library is separate from libtd_engine.so: it needs none of the engine's state, and the engine's sources stay the ones its committed
 * profiles were collected from (td_build_id).  Like td_seam.h it works on a CALLER-SUPPLIED HIP stream -- pass the engine's stream
 * (td_engine_stream) and the render is ordered with the engine's other work by that stream.  All buffers are device memory.  With
 * synchronize = 0 the call only enqueues (per-call scratch comes from the stream-ordered pool, hipMallocAsync / hipFreeAsync, and goes back
 * to it in stream order); with synchronize = 1 the results are complete on return.
 * Conventions as in td_engine.h: plain C, 0 on success / negative code (TD_ERR_* values) on failure with a message in td_relief_last_error().
 */
#ifndef TD_RELIEF_H
#define TD_RELIEF_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* td_relief_last_error(void);

/* out (H, W, 3) fp32 = the reference's relief picture of elev (H, W) fp32, 2 <= H, W <= 2^20:
 *   NaN fill      has_fill: NaN -> fill (the caller's np.nanmedian, 0 when that is not finite), +-inf -> +-FLT_MAX (np.nan_to_num);
 *   blurs         scipy.ndimage.gaussian_filter of the filled image with the 1-D weights wl (2 rl + 1) and ws (2 rs + 1), mode 'reflect',
 *                 axis 0 then axis 1, fp32 between the axes; 0 <= rl, rs <= 64;
 *   hillshades    np.gradient of each blurred field divided by 15 * resolution / 90, sun at azimuth_deg and 45 degrees up, clipped to [0, 1];
 *                 hs = clip(0.75 hs_large + 0.25 hs_small, 0, 1) ** 0.85;
 *   base colour   the terrain colormap (lut: 256 x 3 rows) of max(0, elev) over [max(0, vmin), vmax] when has_range, else over the land's
 *                 nanmin / nanmax (resolved on the device; (0, 1) when not finite or equal); offset to [0.25, 1] when the lower end is 0;
 *   shading       clip(base * (relief * (0.35 + 0.65 hs) + 1 - relief), 0, 1); NaN pixels NaN; ocean ramp where the filled elevation < 0.
 * elev, lut, wl, ws, out: device buffers. */
int td_relief_map(void* hip_stream, const float* elev, int H, int W, const float* lut, const float* wl, int rl, const float* ws, int rs,
                  double azimuth_deg, double resolution, double relief, int has_range, double vmin, double vmax, int has_fill, double fill,
                  float* out, int synchronize);

#ifdef __cplusplus
}
#endif
#endif
