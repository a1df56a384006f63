// Kernels of libtd_custom.so (include/td_custom.h): the cell rasteriser and the nearest-valid fill of the reference's azgaar-to-tiff
// (inference/utils/azgaar_to_tiff.py: rasterize_layer, fill_nodata) and the int16 elevation of its tiff-export (inference/tiff_export.py).
//
// Arithmetic is restated in tests/_custom_twin.py; keep the two in step.  Contraction is off (and the library is built with
// -ffp-contract=off): the rasteriser's edge formula rounds every float64 product, quotient and sum on its own, as NumPy does.  The fill works
// on int32 squared distances only, so nothing in it rounds.  Every kernel is order-independent: the rasteriser resolves overlaps with an
// integer atomicMax of the polygon index, the fill reads planes that an earlier kernel completed.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace td {

constexpr int CW_THREADS = 256;
constexpr int CW_WAVES = CW_THREADS / 64;
constexpr int CW_MAX_SLICES = 64;            // waves that share one polygon's bounding box (grid.y of the owner kernel)
constexpr double CW_TAME = 1.0e9;            // |coordinate| up to here: the bounding box is trusted (see cw_owner_kernel)
constexpr int CW_NONE = 0x7fffffff;          // column plane: this column holds no valid pixel
constexpr unsigned CW_NONE_SQ = 0x7fffffffu; // its squared distance: above every real one (< 2^30), and + 2^28 does not wrap
constexpr int CW_FILL_CHUNK = 1024;          // columns of the column plane staged in LDS at a time by cw_fill_rows_kernel
constexpr int CW_UNROLL = 8;                 // rows a column sweep keeps in flight

// ------------------------------------------------------------------------------------------------------------------------------ rasteriser
// One wave per polygon and slice: the wave finds the ring's bounding box, clips it to the raster, and its lanes walk the box's pixels (slice
// s of S takes every S-th group of 64); each lane runs the crossing-number test of its pixel centre over the whole ring, read from global
// memory (every lane reads the same vertex: one broadcast load, served by the caches), so the vertex count is unbounded.  A covered pixel
// raises owner[r, c] (cleared to -1) to the polygon index: the later polygon wins whatever the order of the waves.
//
// The box is a shortcut and must not change the result.  Rows: an edge counts only when py lies in [min(y0, y1), max(y0, y1)), an exact
// comparison.  Columns: a centre left of every vertex is crossed by an even number of edges and one right of every vertex by none, up to the
// rounding of the intersection, which stays far below the one-pixel margin taken here while coordinates are at most CW_TAME in magnitude.  A
// ring with a larger or non-finite coordinate is tested against the whole raster instead.
__global__ void __launch_bounds__(CW_THREADS) cw_owner_kernel(const double2* __restrict__ xy, long long n_xy, const int* __restrict__ offsets,
                                                              int n, int H, int W, int* __restrict__ owner) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * CW_WAVES + (threadIdx.x >> 6);
    if (p >= n) return;                                   // wave-uniform
    const long long o0 = offsets[p], o1 = offsets[p + 1];
    if (o0 < 0 || o1 > n_xy || o1 - o0 < 3) return;       // wave-uniform; also o1 < o0
    const int nv = (int)(o1 - o0);
    const double2* __restrict__ v = xy + o0;
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    bool wild = false;
    for (int k = lane; k < nv; k += 64) {
        const double2 q = v[k];
        wild |= !(fabs(q.x) <= CW_TAME) || !(fabs(q.y) <= CW_TAME);     // NaN and inf included
        xmin = fmin(xmin, q.x); xmax = fmax(xmax, q.x);
        ymin = fmin(ymin, q.y); ymax = fmax(ymax, q.y);
    }
    for (int o = 32; o > 0; o >>= 1) {
        xmin = fmin(xmin, __shfl_xor(xmin, o, 64)); xmax = fmax(xmax, __shfl_xor(xmax, o, 64));
        ymin = fmin(ymin, __shfl_xor(ymin, o, 64)); ymax = fmax(ymax, __shfl_xor(ymax, o, 64));
    }
    int r0 = 0, r1 = H - 1, c0 = 0, c1 = W - 1;
    if (!__any(wild)) {
        r0 = max(0, (int)floor(ymin) - 1); r1 = min(H - 1, (int)floor(ymax) + 1);
        c0 = max(0, (int)floor(xmin) - 1); c1 = min(W - 1, (int)floor(xmax) + 1);
        if (r0 > r1 || c0 > c1) return;                   // wholly outside the raster
    }
    const int bw = c1 - c0 + 1;
    const long long npix = (long long)(r1 - r0 + 1) * bw;
    for (long long i = (long long)blockIdx.y * 64 + lane; i < npix; i += 64LL * gridDim.y) {
        const int r = r0 + (int)(i / bw), c = c0 + (int)(i % bw);
        const double px = c + 0.5, py = r + 0.5;
        bool inside = false;
        double2 a = v[nv - 1];                            // the closing edge first: the parity does not depend on the order of the edges
        for (int k = 0; k < nv; ++k) {
            const double2 b = v[k];
            if ((a.y > py) != (b.y > py)) {
                const double xi = a.x + (py - a.y) * (b.x - a.x) / (b.y - a.y);
                if (px < xi) inside = !inside;
            }
            a = b;
        }
        if (inside) atomicMax(&owner[(size_t)r * W + c], p);
    }
}

__global__ void __launch_bounds__(CW_THREADS) cw_paint_kernel(const int* __restrict__ owner, const float* __restrict__ values, float fill,
                                                              int npx, float* __restrict__ out) {
    const int i = blockIdx.x * CW_THREADS + threadIdx.x;
    if (i >= npx) return;
    const int p = owner[i];
    out[i] = p >= 0 ? values[p] : fill;
}

// ------------------------------------------------------------------------------------------------------------------------------ nearest fill
__device__ __forceinline__ bool cw_invalid(float v, float nodata) { return isnan(v) || v == nodata; }

// Pass 1, one thread per column (neighbouring threads read neighbouring columns of a row: coalesced): off[r, c] = row of the nearest valid
// pixel of column c minus r, the SMALLER row on a tie, CW_NONE when the column has no valid pixel.  Down sweep: the nearest valid row at or
// above; up sweep: the nearest below replaces it when strictly nearer.  CW_UNROLL rows are loaded before the carried row is updated, so the
// loads of a sweep overlap.  The number of valid pixels goes to *valid (zeroed by the caller), one atomic per wave.
__global__ void __launch_bounds__(CW_THREADS) cw_fill_columns_kernel(const float* __restrict__ in, int H, int W, float nodata,
                                                                     int* __restrict__ off, int* __restrict__ valid) {
    const int c = blockIdx.x * CW_THREADS + threadIdx.x;
    int count = 0;
    if (c < W) {
        int last = -1;
        for (int rb = 0; rb < H; rb += CW_UNROLL) {
            float v[CW_UNROLL];
#pragma unroll
            for (int k = 0; k < CW_UNROLL; ++k) v[k] = rb + k < H ? in[(size_t)(rb + k) * W + c] : 0.f;
#pragma unroll
            for (int k = 0; k < CW_UNROLL; ++k) {
                const int r = rb + k;
                if (r < H) {
                    if (!cw_invalid(v[k], nodata)) { last = r; ++count; }
                    off[(size_t)r * W + c] = last < 0 ? CW_NONE : last - r;
                }
            }
        }
        int next = -1;
        for (int rb = H - 1; rb >= 0; rb -= CW_UNROLL) {
            int up[CW_UNROLL];
#pragma unroll
            for (int k = 0; k < CW_UNROLL; ++k) up[k] = rb - k >= 0 ? off[(size_t)(rb - k) * W + c] : 0;
#pragma unroll
            for (int k = 0; k < CW_UNROLL; ++k) {
                const int r = rb - k;
                if (r >= 0) {
                    if (up[k] == 0) next = r;
                    if (next >= 0 && (up[k] == CW_NONE || next - r < -up[k])) off[(size_t)r * W + c] = next - r;
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(valid, count);
}

// Pass 2, one thread per pixel of a row segment of CW_THREADS columns: an invalid pixel (r, c) takes the minimum over the columns c' of
// (c - c')^2 + off[r, c']^2 in ascending c' with a strict <, so the smallest column wins a tie and pass 1 has settled the row within it.
// Its own column bounds the search: a column further than |off[r, c]| away cannot reach or tie the minimum, so only the columns within
// that radius are scanned, the whole row when the own column has no valid pixel.  The squared column distances of the
// row are staged through LDS in chunks of CW_FILL_CHUNK columns; the block visits the chunks its threads' ranges touch.  Squared distances
// are below 2^30 (H, W <= 16384); CW_NONE_SQ marks an empty column and stays above them with any (c - c')^2 added, without wrapping.
__global__ void __launch_bounds__(CW_THREADS) cw_fill_rows_kernel(const float* __restrict__ in, const int* __restrict__ off, int H, int W,
                                                                  float nodata, float* __restrict__ out, int* __restrict__ out_index) {
    __shared__ unsigned sq[CW_FILL_CHUNK];
    __shared__ int span[2];
    const int tid = threadIdx.x;
    const int r = blockIdx.y, c = blockIdx.x * CW_THREADS + tid;
    const size_t row = (size_t)r * W;
    float v = 0.f;
    bool hole = false;
    if (c < W) {
        v = in[row + c];
        hole = cw_invalid(v, nodata);
        if (!hole) {
            out[row + c] = v;
            if (out_index) out_index[row + c] = (int)(row + c);
        }
    }
    if (tid == 0) { span[0] = W; span[1] = -1; }
    if (!__syncthreads_or(hole)) return;                  // block-uniform
    int lo = 0, hi = -1;
    if (hole) {
        const int own = off[row + c];
        int rad = W;
        if (own != CW_NONE) rad = own < 0 ? -own : own;
        lo = max(0, c - rad);
        hi = min(W - 1, c + rad);
        atomicMin(&span[0], lo);
        atomicMax(&span[1], hi);
    }
    __syncthreads();
    const int blo = span[0], bhi = span[1];
    unsigned best = 0xffffffffu;
    int bestc = -1;
    for (int k0 = (blo / CW_FILL_CHUNK) * CW_FILL_CHUNK; k0 <= bhi; k0 += CW_FILL_CHUNK) {
        __syncthreads();                                  // the previous chunk has been read
        for (int k = tid; k < CW_FILL_CHUNK; k += CW_THREADS) {
            unsigned q = CW_NONE_SQ;
            if (k0 + k < W) {
                const int o = off[row + k0 + k];
                if (o != CW_NONE) q = (unsigned)(o * o);
            }
            sq[k] = q;
        }
        __syncthreads();
        if (hole) {
            const int a = max(lo, k0), b = min(hi, k0 + CW_FILL_CHUNK - 1);
            for (int cc = a; cc <= b; ++cc) {
                const int dx = c - cc;
                const unsigned d = (unsigned)(dx * dx) + sq[cc - k0];
                if (d < best) { best = d; bestc = cc; }
            }
        }
    }
    if (hole) {
        size_t src = row + c;                             // no valid pixel anywhere: unchanged
        if (best < CW_NONE_SQ) src = (size_t)(r + off[row + bestc]) * W + bestc;
        out[row + c] = in[src];
        if (out_index) out_index[row + c] = (int)src;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ int16 export
// np.clip(v, -32768, 32767).astype(np.int16): clip, then truncate toward zero; NaN -> 0
__device__ __forceinline__ short cw_int16(float v) {
    if (isnan(v)) return 0;
    return (short)(int)fminf(fmaxf(v, -32768.f), 32767.f);
}

// four elements per thread: one 16-byte load and one 8-byte store where `vec` (both buffers aligned for them), element-wise otherwise and in the tail
__global__ void __launch_bounds__(CW_THREADS) cw_elev_int16_kernel(const float* __restrict__ elev, long long n, int vec, short* __restrict__ out) {
    const long long i = 4 * ((long long)blockIdx.x * CW_THREADS + threadIdx.x);
    if (i >= n) return;
    if (vec && i + 4 <= n) {
        const float4 v = *reinterpret_cast<const float4*>(elev + i);
        short4 q;
        q.x = cw_int16(v.x); q.y = cw_int16(v.y); q.z = cw_int16(v.z); q.w = cw_int16(v.w);
        *reinterpret_cast<short4*>(out + i) = q;
    } else {
        for (long long k = i; k < n && k < i + 4; ++k) out[k] = cw_int16(elev[k]);
    }
}

}  // namespace td
