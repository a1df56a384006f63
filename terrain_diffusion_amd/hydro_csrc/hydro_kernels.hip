// Hydrology of an elevation image: the reference's d8_flow, flow_accumulation, plot_flow_indicator and fill_depressions_priority_flood
// (terrain_diffusion/inference/postprocessing.py) as parallel kernels with the reference's results, bit for bit (the indicator's log1p to 1 ulp).
//   hydro_d8_kernel             one thread per cell: the eight slopes in the reference's neighbour order, ocean handling, first-maximum argmax
//   hydro_acc_*_kernel          upstream cell counts over the strictly-downhill receiver forest: donors counted with atomics, then one walker
//                               per source cell that carries its running count downstream; only the last donor to arrive at a cell continues
//   hydro_indicator_kernel      non-overlapping k x k max-pool, log1p
//   hydro_fill_*_kernel         Priority-Flood+epsilon as the greatest fixed point of d(c) = h(c) > m(c) ? h(c) : m(c) + eps, m(c) the minimum
//                               of d over the valid neighbours, relaxed downwards from +inf in LDS tiles
// Arithmetic is fp32 in the reference's order; no contraction (numpy does not fuse), correctly rounded division (hipcc's default).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace td {

constexpr int HYDRO_THREADS = 256;
constexpr int FILL_TILE = 64;                    // fill: 64 x 64 cells per workgroup, one column strip of 16 cells per thread
constexpr int FILL_STRIP = FILL_TILE * FILL_TILE / HYDRO_THREADS;
constexpr int FILL_LDS = FILL_TILE + 2;          // + 1 cell of halo on each side
constexpr int FILL_MAX_SWEEPS = 128;             // in-tile sweeps per pass; a tile that needs more continues in the next pass

// k = 0..7: N, S, W, E, NW, NE, SW, SE (the reference's dy / dx)
__constant__ int HYDRO_DY[8] = {-1, 1, 0, 0, -1, -1, 1, 1};
__constant__ int HYDRO_DX[8] = {0, 0, -1, 1, -1, 1, -1, 1};

__device__ __forceinline__ int hydro_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
// ocean / invalid: NaN or <= 0
__device__ __forceinline__ bool hydro_ocean(float v) { return !(v > 0.f); }

// ---------------------------------------------------------------------------------------------------------------------------------------------
// D8.  Neighbours outside the image take the edge value (np.pad mode 'edge'): z[clamp(i + dy), clamp(j + dx)].  slope = (zc - zn) / dist in
// fp32, dist = fl32(sqrt 2) on the diagonals; a slope below tol is -inf (a NaN slope is not below it and stays NaN).  prefer: -inf for an ocean
// centre, +inf into an ocean neighbour of a land centre; ignore: -inf for both.  argmax is numpy's: the first maximum, a NaN wins at once.
// receiver = clamp(i + dy[kmax]) * W + clamp(j + dx[kmax]); is_sink = ocean centre, or no ocean neighbour and no finite maximum of ignore.
__global__ __launch_bounds__(HYDRO_THREADS) void hydro_d8_kernel(const float* __restrict__ z, int H, int W, float tol, int32_t* __restrict__ receiver,
                                                                  uint8_t* __restrict__ kmax_out, uint8_t* __restrict__ sink_out) {
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= (int64_t)H * W) return;
    const int i = (int)(cell / W), j = (int)(cell % W);
    const float dist_diag = __uint_as_float(0x3FB504F3u);   // fl32(sqrt(2))
    const float zc = z[(size_t)i * W + j];
    const bool center_ocean = hydro_ocean(zc);
    float best_p = 0.f, best_i = 0.f;
    int kp = 0;
    bool ocean_nbr = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float zn = z[(size_t)hydro_clamp(i + HYDRO_DY[k], H) * W + hydro_clamp(j + HYDRO_DX[k], W)];
        float s = (zc - zn) / (k < 4 ? 1.0f : dist_diag);
        if (s < tol) s = -INFINITY;
        const bool no = hydro_ocean(zn);
        ocean_nbr |= no;
        const float p = center_ocean ? -INFINITY : (no ? INFINITY : s);
        const float g = (center_ocean || no) ? -INFINITY : s;
        if (k == 0) {
            best_p = p;
            best_i = g;
        } else {
            if (!isnan(best_p) && !(p <= best_p)) { best_p = p; kp = k; }
            if (!isnan(best_i) && !(g <= best_i)) best_i = g;
        }
    }
    const size_t c = (size_t)i * W + j;
    receiver[c] = hydro_clamp(i + HYDRO_DY[kp], H) * W + hydro_clamp(j + HYDRO_DX[kp], W);
    kmax_out[c] = (uint8_t)kp;
    sink_out[c] = (center_ocean || (!ocean_nbr && !isfinite(best_i))) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Accumulation.  A counted edge c -> r: c valid, not a sink, r valid (the reference's loop).  Each cell holds one 64-bit word,
//   word = (count << 32) | pending donors,
// so one agent-scope atomic add of (total << 32) - 1 both delivers a donor's total and retires it: the donor that sees pending == 1 in the old
// word arrived last, and the old word's count plus its own total is the receiver's complete count -- no second location, so no ordering
// between two atomics to rely on across the non-coherent per-XCD L2s.  No workgroup ever waits for another.

// word = valid ? 1 << 32 : 0; next = receiver of a counted edge, or -1; a counted edge that is not strictly downhill (or a receiver outside
// the image) counts in *bad.  Then one atomic per counted edge counts the receiver's donors.
__global__ __launch_bounds__(HYDRO_THREADS) void hydro_acc_init_kernel(const float* __restrict__ z, int N, unsigned long long* __restrict__ word) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < N) word[c] = hydro_ocean(z[c]) ? 0ull : (1ull << 32);
}

__global__ __launch_bounds__(HYDRO_THREADS) void hydro_acc_edges_kernel(const float* __restrict__ z, int N, const int32_t* __restrict__ receiver,
                                                                         const uint8_t* __restrict__ is_sink, int32_t* __restrict__ next,
                                                                         unsigned long long* __restrict__ word, unsigned* __restrict__ bad) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const float zc = z[c];
    int nx = -1;
    if (!hydro_ocean(zc) && !is_sink[c]) {
        const int r = receiver[c];
        if (r < 0 || r >= N) {
            __hip_atomic_fetch_add(bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const float zr = z[r];
            if (!hydro_ocean(zr)) {
                if (!(zr < zc)) __hip_atomic_fetch_add(bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                nx = r;
                __hip_atomic_fetch_add(&word[r], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    next[c] = nx;
}

// One thread per cell; a source (valid, no donors: word == 1 << 32, a value no cell with donors ever holds) walks downstream.  Every step
// retires one counted edge, so the walks end whatever the edges are (a cycle of bad edges is never entered: its cells keep pending > 0).
__global__ __launch_bounds__(HYDRO_THREADS) void hydro_acc_walk_kernel(int N, const int32_t* __restrict__ next, unsigned long long* __restrict__ word) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    if (__hip_atomic_load(&word[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (1ull << 32)) return;
    unsigned long long total = 1;
    int cur = c;
    for (;;) {
        const int t = next[cur];
        if (t < 0) break;
        const unsigned long long old = __hip_atomic_fetch_add(&word[t], (total << 32) - 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((old & 0xFFFFFFFFull) != 1ull) break;   // donors still to come: the last of them carries on
        total += old >> 32;
        cur = t;
    }
}

__global__ __launch_bounds__(HYDRO_THREADS) void hydro_acc_out_kernel(int N, const unsigned long long* __restrict__ word, float* __restrict__ acc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < N) acc[c] = (float)(unsigned)(word[c] >> 32);   // <= 2^24: exact in fp32
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Indicator: out (H / k, W / k) = log1p(max of acc over the k x k block), numpy's max (a NaN wins); log1p in fp64, rounded once to fp32.
__global__ __launch_bounds__(HYDRO_THREADS) void hydro_indicator_kernel(const float* __restrict__ acc, int W, int k, int Ho, int Wo, float* __restrict__ out) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;   // Ho * Wo <= 2^24
    if (o >= Ho * Wo) return;
    const int y = o / Wo, x = o % Wo;
    float m = acc[(size_t)y * k * W + (size_t)x * k];
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) {
            const float v = acc[(size_t)(y * k + a) * W + (size_t)x * k + b];
            if (!isnan(m) && !(v <= m)) m = v;
        }
    out[(size_t)y * Wo + x] = (float)log1p((double)m);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Fill.  Working image d (the output buffer): invalid cells +inf (never a neighbour's minimum), seeds h, other valid cells +inf at the start.
// hw: h of the cells that relax, NaN for the fixed ones (invalid cells and seeds).  Seeds: valid border cells and valid cells with an invalid
// neighbour in the connectivity.  Invalid: NaN, <= 0, or == nodata.
__device__ __forceinline__ bool hydro_invalid(float v, int has_nodata, float nodata) { return !(v > 0.f) || (has_nodata && v == nodata); }

__global__ __launch_bounds__(HYDRO_THREADS) void hydro_fill_init_kernel(const float* __restrict__ h, int H, int W, int conn8, int has_nodata, float nodata,
                                                                         float* __restrict__ d, float* __restrict__ hw) {
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= (int64_t)H * W) return;
    const int i = (int)(cell / W), j = (int)(cell % W);
    const size_t c = (size_t)i * W + j;
    const float v = h[c];
    if (hydro_invalid(v, has_nodata, nodata)) {
        d[c] = INFINITY;
        hw[c] = NAN;
        return;
    }
    bool seed = i == 0 || i == H - 1 || j == 0 || j == W - 1;
    for (int k = 0; k < (conn8 ? 8 : 4) && !seed; ++k) {
        const int y = i + HYDRO_DY[k], x = j + HYDRO_DX[k];
        seed = hydro_invalid(h[(size_t)y * W + x], has_nodata, nodata);   // interior cell: every neighbour is inside
    }
    d[c] = seed ? v : INFINITY;
    hw[c] = seed ? NAN : v;
}

// One relaxation pass: d = min(d, G(d)) swept in the LDS tile (Gauss-Seidel, alternating direction) until the tile stops changing or
// FILL_MAX_SWEEPS, halo read at the start.  Values only fall and every value read, stale or not, bounds the result from above, so concurrent
// tiles need no ordering.  A tile runs only when it or one of its 8 neighbour tiles changed in the previous pass (tile_prev; null: all run),
// and not at all once the previous pass changed nothing (*prev_flag == 0; null: first pass of a batch).  tile_cur and *flag record this pass.
__global__ __launch_bounds__(HYDRO_THREADS) void hydro_fill_pass_kernel(float* __restrict__ d, const float* __restrict__ hw, int H, int W, float eps, int conn8,
                                                                         const unsigned* __restrict__ tile_prev, unsigned* __restrict__ tile_cur,
                                                                         const unsigned* __restrict__ prev_flag, unsigned* __restrict__ flag) {
    __shared__ float s[FILL_LDS * FILL_LDS];
    const int tx = blockIdx.x, ty = blockIdx.y, ntx = gridDim.x, nty = gridDim.y;
    const int tid = threadIdx.x;
    bool active = prev_flag == nullptr || *prev_flag != 0u;
    if (active && tile_prev) {
        active = false;
        for (int a = ty - 1; a <= ty + 1; ++a)
            for (int b = tx - 1; b <= tx + 1; ++b)
                if (a >= 0 && a < nty && b >= 0 && b < ntx && tile_prev[a * ntx + b]) active = true;
    }
    if (!active) {   // block-uniform
        if (tid == 0) tile_cur[ty * ntx + tx] = 0u;
        return;
    }
    const int y0 = ty * FILL_TILE, x0 = tx * FILL_TILE;
    for (int q = tid; q < FILL_LDS * FILL_LDS; q += HYDRO_THREADS) {
        const int y = y0 - 1 + q / FILL_LDS, x = x0 - 1 + q % FILL_LDS;
        s[q] = (y >= 0 && y < H && x >= 0 && x < W) ? d[(size_t)y * W + x] : INFINITY;
    }
    const int col = tid % FILL_TILE, r0 = (tid / FILL_TILE) * FILL_STRIP;
    float hv[FILL_STRIP];
#pragma unroll
    for (int k = 0; k < FILL_STRIP; ++k) {
        const int y = y0 + r0 + k, x = x0 + col;
        hv[k] = (y < H && x < W) ? hw[(size_t)y * W + x] : NAN;
    }
    __syncthreads();
    bool any = false;
    for (int sweep = 0; sweep < FILL_MAX_SWEEPS; ++sweep) {
        bool ch = false;
#pragma unroll
        for (int kk = 0; kk < FILL_STRIP; ++kk) {
            const int k = (sweep & 1) ? FILL_STRIP - 1 - kk : kk;
            if (isnan(hv[k])) continue;
            const int q = (r0 + k + 1) * FILL_LDS + col + 1;
            float m = fminf(fminf(s[q - FILL_LDS], s[q + FILL_LDS]), fminf(s[q - 1], s[q + 1]));
            if (conn8) m = fminf(m, fminf(fminf(s[q - FILL_LDS - 1], s[q - FILL_LDS + 1]), fminf(s[q + FILL_LDS - 1], s[q + FILL_LDS + 1])));
            if (!(m < INFINITY)) continue;
            const float g = hv[k] > m ? hv[k] : m + eps;
            if (g < s[q]) {
                s[q] = g;
                ch = true;
            }
        }
        if (!__syncthreads_or(ch)) break;
        any = true;
    }
    if (any) {   // block-uniform (from __syncthreads_or)
#pragma unroll
        for (int k = 0; k < FILL_STRIP; ++k) {
            const int y = y0 + r0 + k, x = x0 + col;
            if (y < H && x < W && !isnan(hv[k])) d[(size_t)y * W + x] = s[(r0 + k + 1) * FILL_LDS + col + 1];
        }
        if (tid == 0) *flag = 1u;
    }
    if (tid == 0) tile_cur[ty * ntx + tx] = any ? 1u : 0u;
}

// out = d on valid cells, h (NaN included) elsewhere.
__global__ __launch_bounds__(HYDRO_THREADS) void hydro_fill_out_kernel(const float* __restrict__ h, size_t N, int has_nodata, float nodata, float* __restrict__ d) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < N && hydro_invalid(h[c], has_nodata, nodata)) d[c] = h[c];
}

}  // namespace td
