/*
 * td_custom.h — C-ABI of the custom-map import library (libtd_custom.so): the device halves of the reference's two commands that let a user
 * bring a world of their own,
 *   azgaar-to-tiff   terrain_diffusion/inference/utils/azgaar_to_tiff.py: rasterize_layer (polygonal cells -> a raster) and fill_nodata
 *                    (every hole takes the nearest valid pixel),
 *   tiff-export      terrain_diffusion/inference/tiff_export.py: the int16 elevation it writes.
 * terrain_diffusion_amd/custom_world.py holds the host halves (the Azgaar JSON, padding and installing the layers, the export's chunk loop).
 *
 * Conventions as in td_relief.h: a library of its own beside libtd_engine.so, plain C, a CALLER-SUPPLIED HIP stream (pass td_engine_stream),
 * device buffers only, per-call scratch from the stream-ordered pool (hipMallocAsync / hipFreeAsync), synchronize = 0 only enqueues,
 * synchronize = 1 completes on return; 0 on success / negative code with a message in td_custom_last_error().
 *
 * Two things this library states rather than reproduces:
 *   - The pixel-CENTRE rule of td_custom_rasterize is this project's statement of GDAL's all_touched=False.  It was not compared with GDAL;
 *     a difference is possible only for a pixel centre that lies on an edge to within rounding.
 *   - A layer without one valid pixel is REFUSED by the Python binding (fill_nearest raises) rather than reproduced: the reference's result
 *     for it is meaningless.  td_custom_fill_nearest itself leaves such a layer unchanged and reports 0 valid pixels.
 */
#ifndef TD_CUSTOM_H
#define TD_CUSTOM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TD_CUSTOM_MAX_SIDE 16384          /* 1 <= H, W <= 16384: flat indices and squared pixel distances stay below 2^31 */
#define TD_CUSTOM_MAX_ELEMENTS (1 << 30)  /* td_custom_elev_int16: 0 <= n <= 2^30 */

const char* td_custom_last_error(void);

/* out (H, W) fp32 = rasterize_layer with all_touched=False.  n polygons in CSR form: polygon p is the ring of the vertices
 * offsets[p] .. offsets[p + 1] - 1 of xy (n_xy (x, y) float64 pairs, already in pixel units: x along columns, y along rows), implicitly
 * closed; values[p] is what it burns.  Pixel (r, c) belongs to a polygon when its centre (px, py) = (c + 0.5, r + 0.5) is inside by the
 * crossing-number test: an edge (x0, y0) -> (x1, y1) counts when (y0 > py) != (y1 > py) and px < x0 + (py - y0) * (x1 - x0) / (y1 - y0),
 * in float64, in that order, without contraction; an odd count is inside.  Where polygons overlap the one LATER in the list wins (the
 * painter's order, as GDAL burns shapes in sequence); the result does not depend on the order the device visits them in.  A ring with fewer
 * than 3 vertices burns nothing, neither does one whose offsets leave [0, n_xy] or decrease.  Pixels no polygon covers get `fill` (NaN is a
 * valid fill).  The vertex count of a polygon is unbounded.  n = 0 is allowed (xy, offsets and values may then be null): all fill.
 * xy, offsets (n + 1 int32), values (n fp32), out: device buffers. */
int td_custom_rasterize(void* hip_stream, const double* xy, int64_t n_xy, const int32_t* offsets, const float* values, int n, int H, int W,
                        double fill, float* out, int synchronize);

/* out (H, W) fp32 = fill_nodata(in, nodata): every invalid pixel of in takes the value of the nearest valid pixel in exact Euclidean
 * distance; a valid pixel keeps its bits.  Invalid = NaN, or equal to (float)nodata (pass NaN for "NaN only").  Among the valid pixels at
 * the minimum squared distance the one in the SMALLEST COLUMN wins, and within that column the one in the smallest row: the choice of
 * scipy.ndimage.distance_transform_edt(return_indices=True), which the reference calls.
 * out_valid (1 int32) receives the number of valid pixels; with 0 valid pixels out = in.  out_index, when not null, (H, W) int32 receives
 * the flat index r * W + c of the pixel each output pixel was taken from (its own for a valid one).  out must not overlap in.
 * Work: one pass over the columns, then for every invalid pixel a scan of its row of column distances (O(W) each, cut to the columns no
 * further away than the nearest valid pixel of its own column).  in, out, out_index, out_valid: device buffers. */
int td_custom_fill_nearest(void* hip_stream, const float* in, int H, int W, double nodata, float* out, int32_t* out_index,
                           int32_t* out_valid, int synchronize);

/* out (n) int16, little-endian = np.clip(elev, -32768, 32767).astype(np.int16) of the export: clip, then TRUNCATE toward zero (-0.999 -> 0;
 * td_explorer_raw floors instead).  NaN is written as 0, the convention of td_mc_payload and td_explorer_raw (the reference's cast of NaN is
 * undefined).  elev (n fp32), out: device buffers; out needs 2-byte alignment. */
int td_custom_elev_int16(void* hip_stream, const float* elev, int64_t n, int16_t* out, int synchronize);

#ifdef __cplusplus
}
#endif
#endif
