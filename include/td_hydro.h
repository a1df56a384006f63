/*
 * td_hydro.h — C-ABI of the hydrology library (libtd_hydro.so): the reference's d8_flow, flow_accumulation, plot_flow_indicator and
 * fill_depressions_priority_flood with max_raise = None (terrain_diffusion/inference/postprocessing.py), on fp32 elevation.
 *
 * A library of its own, like td_relief.h: the engine's sources stay the ones its committed profiles were collected from (td_build_id).  Every
 * call works on a CALLER-SUPPLIED HIP stream -- pass the engine's stream (td_engine_stream) to order it with the engine's other work.  All
 * buffers are device memory.  With synchronize = 0 a call only enqueues (per-call scratch comes from the stream-ordered pool, hipMallocAsync /
 * hipFreeAsync, and goes back to it in stream order); with synchronize = 1 the results are complete on return.  td_hydro_fill always
 * synchronises: it reads its convergence flags on the host.
 * Conventions as in td_engine.h: plain C, 0 on success / negative code (TD_ERR_* values) on failure with a message in td_hydro_last_error().
 * Invalid (ocean) cells are NaN or <= 0 everywhere; the fill also treats cells equal to nodata as invalid.
 */
#ifndef TD_HYDRO_H
#define TD_HYDRO_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* td_hydro_last_error(void);

/* D8 steepest descent of z (H, W), 1 <= H, W <= 2^20, H W < 2^31.  Neighbour k = 0..7 is N, S, W, E, NW, NE, SW, SE; outside the image a
 * neighbour takes the edge value.  slope = (z_c - z_n) / dist in fp32 (dist 1, or fl32(sqrt 2) on the diagonals), -inf below fl32(tol); an
 * ocean centre has every slope -inf, an ocean neighbour of a land centre +inf.  kmax = the first maximum (0 when all are -inf);
 * receiver = clamp(i + dy[kmax]) * W + clamp(j + dx[kmax]) (int32, flat); is_sink = 1 for an ocean centre, or a centre with no ocean
 * neighbour and no finite slope once ocean is ignored. */
int td_hydro_d8(void* hip_stream, const float* z, int H, int W, double tol, int32_t* receiver, uint8_t* kmax, uint8_t* is_sink, int synchronize);

/* Upstream cell count acc (H, W) fp32, 1 <= H, W, H W <= 2^24: acc = 1 + the sum over donors on valid cells, 0 on invalid ones.  A counted
 * edge runs from a valid, non-sink cell c to receiver[c] when that receiver is valid.  *bad_edges (device, uint32) = the number of counted edges
 * that do not go strictly downhill or whose receiver lies outside [0, H W): where it is not 0 the reference's result depends on the order its
 * sort gives to equal elevations, and acc is not meaningful. */
int td_hydro_accumulate(void* hip_stream, const float* z, int H, int W, const int32_t* receiver, const uint8_t* is_sink, float* acc,
                        uint32_t* bad_edges, int synchronize);

/* out (H / k, W / k) fp32 = log1p of the maximum of acc (H, W) over each non-overlapping k x k block (rows and columns past a multiple of k
 * are dropped); 1 <= k <= min(H, W), H W <= 2^24.  log1p is evaluated in fp64 and rounded once. */
int td_hydro_indicator(void* hip_stream, const float* acc, int H, int W, int k, float* out, int synchronize);

/* Priority-Flood+epsilon depression fill of h (H, W), 1 <= H, W <= 2^20, H W < 2^31, into out (not aliasing h); connectivity 4, anything else
 * means 8; epsilon >= 0, added in fp32; has_nodata: cells equal to fl32(nodata) are invalid too.  Invalid cells keep h.  Seeds (valid border
 * cells, valid cells with an invalid neighbour) keep h; every other valid cell c takes d(c) = h(c) > m(c) ? h(c) : m(c) + epsilon, m(c) the
 * minimum of d over its valid neighbours -- the greatest solution, which is the reference's heap result.  *passes (host, may be null) = the
 * number of relaxation passes until one changed nothing.  ALWAYS synchronises the stream before returning. */
int td_hydro_fill(void* hip_stream, const float* h, int H, int W, double epsilon, int connectivity, int has_nodata, double nodata, float* out,
                  int* passes);

#ifdef __cplusplus
}
#endif
#endif
