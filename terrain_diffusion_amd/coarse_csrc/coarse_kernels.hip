// Kernels of libtd_coarse.so (include/td_coarse.h): the device half of the reference's coarse-dataset preparation
// (terrain_diffusion/training/datasets/coarse_dataset.py) -- the width-only area resize of a latitude band, the statistics of its t x t tiles,
// the crop score of __getitem__ and fill_oceans, a Laplace inpainting solved by Jacobi-preconditioned CG from a coarse-grid start.
//
// Arithmetic is restated in tests/_coarse_twin.py; keep the two in step.  Contraction is off (and the library is built with
// -ffp-contract=off): every product and sum rounds on its own, as NumPy's and scipy's do.  Every kernel is order-independent: order
// statistics are found by counting with an index tie-break, integer counts are exact, and every floating sum goes thread by thread in
// ascending order and then through a fixed tree (no floating-point atomic anywhere), so two runs give the same bits.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace td {

constexpr int CO_THREADS = 256;
constexpr int CO_WAVES = CO_THREADS / 64;
constexpr int CO_MAX_TILE = 32;                          // td_coarse.h TD_COARSE_MAX_TILE
constexpr int CO_ITEMS = CO_MAX_TILE * CO_MAX_TILE;      // values one block of the tile statistics / crop scores holds
constexpr int CO_CG_BLOCKS = 1024;                       // workgroups of a solver pass at most: the width of its reduction tree

// the fixed tree of a block: xor-shuffles inside a wave (every lane ends with the same bits), then the waves' sums pairwise; every thread
// must call it and every thread receives the sum
__device__ __forceinline__ double co_block_sum(double v, double* wave_sums) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3]);
    __syncthreads();
    return s;
}
static_assert(CO_WAVES == 4, "co_block_sum adds four wave sums");

// ------------------------------------------------------------------------------------------------------------------------------ area resize
__device__ __forceinline__ float co_load(float v, int rule) {
    if (rule == 1) return fabsf(v - 32768.f) < 1e-6f ? __builtin_nanf("") : v;
    if (rule == 2) return fabsf(v) > 1e6f ? __builtin_nanf("") : v;
    if (rule == 3) return copysignf(sqrtf(fabsf(v)), v);
    return v;
}

// One thread per output element: the window [floor(j Win / Wout), ceil((j + 1) Win / Wout)) of its row, summed from the left in fp32.
__global__ void __launch_bounds__(CO_THREADS) co_area_resize_kernel(const float* __restrict__ x, long long total, int W_in, int W_out, int rule,
                                                                    float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * CO_THREADS + threadIdx.x;
    if (i >= total) return;
    const long long y = i / W_out, j = i - y * W_out;
    const long long a = (j * W_in) / W_out, b = ((j + 1) * W_in + W_out - 1) / W_out;     // b <= W_in, b > a
    const float* __restrict__ row = x + y * W_in;
    float acc = co_load(row[a], rule);
    for (long long k = a + 1; k < b; ++k) acc = acc + co_load(row[k], rule);
    out[i] = acc / (float)(b - a);
}

// ------------------------------------------------------------------------------------------------------------------------------ order statistics
// The values val[0 .. n) of one block in LDS, none of them NaN: the rank of a value is the number of values that are smaller, or equal and
// earlier -- a permutation of 0 .. n - 1 whatever the order of the visits.  The values of ranks k0 and k1 go to pick[0], pick[1].
__device__ __forceinline__ void co_select(const float* val, int n, int k0, int k1, float* pick) {
    for (int i = threadIdx.x; i < n; i += CO_THREADS) {
        const float v = val[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (val[j] < v) || (val[j] == v && j < i);
        if (rank == k0) pick[0] = v;
        if (rank == k1) pick[1] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ tile statistics
// One block per tile.  The float64 sum of the non-NaN values: thread i adds the values i, i + 256, ... in ascending order, then the block's
// tree; their number likewise (exact).  mean = sum / n where no value is NaN; nanmean = sum / count; quantile: numpy's `linear` on the two
// order statistics k, min(k + 1, n - 1) of r = q (n - 1), interpolated in float64 and rounded once.
__global__ void __launch_bounds__(CO_THREADS) co_tile_stats_kernel(const float* __restrict__ x, int Ws, int t, int Wt, double q,
                                                                   float* __restrict__ out_mean, float* __restrict__ out_nanmean,
                                                                   float* __restrict__ out_quantile) {
    __shared__ float val[CO_ITEMS];
    __shared__ float pick[2];
    __shared__ double wave_sums[CO_WAVES];
    const int tid = threadIdx.x;
    const int n = t * t;
    const long long tile = blockIdx.x;
    const long long ty = tile / Wt, tx = tile - ty * Wt;
    const float* __restrict__ src = x + (size_t)(ty * t) * Ws + (size_t)tx * t;
    double acc = 0.0, cnt = 0.0;
    for (int i = tid; i < n; i += CO_THREADS) {
        const int r = i / t, c = i - r * t;
        const float v = src[(size_t)r * Ws + c];
        val[i] = v;
        if (!isnan(v)) { acc += (double)v; cnt += 1.0; }
    }
    if (tid < 2) pick[tid] = 0.f;
    const double sum = co_block_sum(acc, wave_sums);      // also the barrier after the stores to val and pick
    const double count = co_block_sum(cnt, wave_sums);
    const bool whole = count == (double)n;
    const float nan = __builtin_nanf("");
    if (tid == 0) {
        if (out_mean) out_mean[tile] = whole ? (float)(sum / (double)n) : nan;
        if (out_nanmean) out_nanmean[tile] = count > 0.0 ? (float)(sum / count) : nan;
    }
    if (!out_quantile) return;                            // block-uniform
    const double r = q * (double)(n - 1);
    const int k0 = (int)floor(r), k1 = min(k0 + 1, n - 1);
    if (whole) co_select(val, n, k0, k1, pick);
    __syncthreads();
    if (tid == 0) {
        const double a = (double)pick[0], b = (double)pick[1];
        out_quantile[tile] = whole ? (float)(a + (b - a) * (r - (double)k0)) : nan;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ crop scores
// One block per crop: e in LDS inside a frame of zeros (avg_pool2d pads with zeros and always divides by 9), d^2 in LDS, then the two order
// statistics of torch.quantile's rank.  A crop that leaves the plane, or holds a NaN, gives NaN.
__global__ void __launch_bounds__(CO_THREADS) co_crop_scores_kernel(const float* __restrict__ plane, int H, int W, float mean0, float std0,
                                                                    const int* __restrict__ offsets, int c, float* __restrict__ out) {
    __shared__ float e[(CO_MAX_TILE + 2) * (CO_MAX_TILE + 2)];
    __shared__ float d2[CO_ITEMS];
    __shared__ float pick[2];
    __shared__ int has_nan;
    const int tid = threadIdx.x;
    const int n = c * c, ew = c + 2;
    const int oi = offsets[2 * blockIdx.x], oj = offsets[2 * blockIdx.x + 1];
    const float nan = __builtin_nanf("");
    if (oi < 0 || oj < 0 || oi > H - c || oj > W - c) {   // block-uniform
        if (tid == 0) out[blockIdx.x] = nan;
        return;
    }
    for (int i = tid; i < ew * ew; i += CO_THREADS) e[i] = 0.f;
    if (tid == 0) { has_nan = 0; pick[0] = 0.f; pick[1] = 0.f; }
    __syncthreads();
    for (int i = tid; i < n; i += CO_THREADS) {
        const int r = i / c, col = i - r * c;
        const float v = plane[(size_t)(oi + r) * W + oj + col];
        const float s = v * std0 + mean0;
        e[(r + 1) * ew + col + 1] = s > 0.f ? s * s : (s <= 0.f ? 0.f : nan);
    }
    __syncthreads();
    for (int i = tid; i < n; i += CO_THREADS) {
        const int r = i / c, col = i - r * c;
        const float* __restrict__ w = e + r * ew + col;   // the top-left corner of the 3 x 3 window
        float sum = w[0];
        sum = sum + w[1]; sum = sum + w[2];
        sum = sum + w[ew]; sum = sum + w[ew + 1]; sum = sum + w[ew + 2];
        sum = sum + w[2 * ew]; sum = sum + w[2 * ew + 1]; sum = sum + w[2 * ew + 2];
        const float d = w[ew + 1] - sum / 9.f;
        const float v = d * d;
        d2[i] = v;
        if (isnan(v)) has_nan = 1;                        // every writer stores the same 1
    }
    __syncthreads();
    const float rank = 0.9f * (float)(n - 1);
    const int k0 = (int)floorf(rank), k1 = min(k0 + 1, n - 1);
    const float g = rank - (float)k0;
    const bool whole = has_nan == 0;
    if (whole) co_select(d2, n, k0, k1, pick);
    __syncthreads();
    if (tid == 0) {
        const float a = pick[0], b = pick[1];
        const float v = g < 0.5f ? a + g * (b - a) : b - (b - a) * (1.f - g);
        out[blockIdx.x] = whole ? v : nan;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ fill_oceans
// The state of one CG solve, in device memory: the host never needs it to enqueue an iteration.
struct CoState {
    int flag;            // set: the loop has ended (converged, b = 0, no unknowns, or the limit); every solver kernel returns at once
    int info;            // scipy's info: 0, or the limit when the limit ended the loop
    int iters;           // completed iterations (scipy's callback count)
    int limit;           // maxiter, or max(50, int(10 sqrt(n)))
    int zero_x;          // b = 0: scipy returns zeros whatever x0 was
    int pad;
    long long n;         // unknowns
    double thr;          // max(tol, 1e-5 |b|_2)
    double rho[2];       // r . z of the even / odd iterations
};

// numpy's add.reduce over a contiguous axis of n <= 32 float64 values: sequential below 8, else eight running sums combined pairwise and the
// rest added one by one (np.nanmean of coarse_dataset.py:183 on the inner axis)
__device__ __forceinline__ double co_numpy_sum(const double* v, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += v[i];
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = v[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += v[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += v[i];
    return res;
}

// One thread per coarse cell: the NaN-ignoring mean of the NaN-ignoring row means of its f x f block, NaN outside the image (:165-184).
__global__ void __launch_bounds__(CO_THREADS) co_block_nanmean_kernel(const double* __restrict__ a, int H, int W, int f, int Hc, int Wc,
                                                                      double* __restrict__ coarse) {
    const int i = blockIdx.x * CO_THREADS + threadIdx.x;
    if (i >= Hc * Wc) return;
    const int cy = i / Wc, cx = i - cy * Wc;
    double rows = 0.0;
    int n_rows = 0;
    for (int dy = 0; dy < f; ++dy) {
        const int y = cy * f + dy;
        if (y >= H) break;                                // padded rows hold NaN only
        double v[CO_MAX_TILE];
        int cnt = 0;
        for (int dx = 0; dx < f; ++dx) {
            const int x = cx * f + dx;
            const double t = x < W ? a[(size_t)y * W + x] : __builtin_nan("");
            const bool ok = !isnan(t);
            v[dx] = ok ? t : 0.0;
            cnt += ok;
        }
        if (cnt) { rows += co_numpy_sum(v, f) / (double)cnt; ++n_rows; }
    }
    coarse[i] = n_rows ? rows / (double)n_rows : __builtin_nan("");
}

// scipy.ndimage.zoom(order=1, mode='nearest'): output index o reads coordinate o (n_in - 1) / (n_out - 1) (1 where n_out = 1)
__device__ __forceinline__ void co_zoom_taps(int o, int n_in, int n_out, int& i0, int& i1, double& w0, double& w1) {
    const double z = n_out > 1 ? (double)(n_in - 1) / (double)(n_out - 1) : 1.0;
    const double cc = (double)o * z;
    const int s = (int)floor(cc);
    w1 = cc - (double)s;
    w0 = 1.0 - w1;
    i0 = min(max(s, 0), n_in - 1);
    i1 = min(max(s + 1, 0), n_in - 1);
}

// x0 of the fine solve: the zoomed coarse result on the ocean pixels, 0 on land
__global__ void __launch_bounds__(CO_THREADS) co_zoom_kernel(const double* __restrict__ cf, int Hc, int Wc, const double* __restrict__ a, int H,
                                                             int W, double* __restrict__ x) {
    const int i = blockIdx.x * CO_THREADS + threadIdx.x;
    if (i >= H * W) return;
    double v = 0.0;
    if (isnan(a[i])) {
        const int y = i / W, xx = i - y * W;
        int i0, i1, j0, j1;
        double wy0, wy1, wx0, wx1;
        co_zoom_taps(y, Hc, H, i0, i1, wy0, wy1);
        co_zoom_taps(xx, Wc, W, j0, j1, wx0, wx1);
        v = cf[(size_t)i0 * Wc + j0] * wy0 * wx0;
        v = v + cf[(size_t)i0 * Wc + j1] * wy0 * wx1;
        v = v + cf[(size_t)i1 * Wc + j0] * wy1 * wx0;
        v = v + cf[(size_t)i1 * Wc + j1] * wy1 * wx1;
    }
    x[i] = v;
}

// The system of one level on its plane a (H, W), NaN = unknown.  code = 0 on land, 0x80 | (number of in-image neighbours) on an unknown;
// b = the sum of the land neighbours (up, down, left, right, the reference's order); r = b - A x0 (x0 null: zeros), z = r / diag; one
// partial of b . b, r . r and r . z and one count of unknowns per block.
__global__ void __launch_bounds__(CO_THREADS) co_cg_setup_kernel(const double* __restrict__ a, const double* __restrict__ x0, int H, int W,
                                                                 unsigned char* __restrict__ code, double* __restrict__ r, double* __restrict__ z,
                                                                 double* __restrict__ part_bb, double* __restrict__ part_rr,
                                                                 double* __restrict__ part_rz, double* __restrict__ part_n) {
    __shared__ double wave_sums[CO_WAVES];
    const int N = H * W;
    double bb = 0.0, rr = 0.0, rz = 0.0, cnt = 0.0;
    for (int i = blockIdx.x * CO_THREADS + threadIdx.x; i < N; i += gridDim.x * CO_THREADS) {
        unsigned char cd = 0;
        double rv = 0.0, zv = 0.0;
        if (isnan(a[i])) {
            const int y = i / W, x = i - y * W;
            int diag = 0;
            double b = 0.0, ax = 0.0;
            const int nb[4] = {y > 0 ? i - W : -1, y < H - 1 ? i + W : -1, x > 0 ? i - 1 : -1, x < W - 1 ? i + 1 : -1};
            for (int k = 0; k < 4; ++k) {
                if (nb[k] < 0) continue;
                ++diag;
                const double t = a[nb[k]];
                if (!isnan(t)) b += t;
            }
            if (x0) {                                     // A x0: diag x0 minus the in-image neighbours up, left, right, down (x0 is 0 on land)
                ax = (double)diag * x0[i];
                if (nb[0] >= 0) ax -= x0[nb[0]];
                if (nb[2] >= 0) ax -= x0[nb[2]];
                if (nb[3] >= 0) ax -= x0[nb[3]];
                if (nb[1] >= 0) ax -= x0[nb[1]];
            }
            cd = (unsigned char)(0x80 | diag);
            rv = b - ax;
            zv = rv * (diag > 0 ? 1.0 / (double)diag : 1.0);
            bb += b * b; rr += rv * rv; rz += rv * zv; cnt += 1.0;
        }
        code[i] = cd; r[i] = rv; z[i] = zv;
    }
    const double s0 = co_block_sum(bb, wave_sums), s1 = co_block_sum(rr, wave_sums), s2 = co_block_sum(rz, wave_sums), s3 = co_block_sum(cnt, wave_sums);
    if (threadIdx.x == 0) { part_bb[blockIdx.x] = s0; part_rr[blockIdx.x] = s1; part_rz[blockIdx.x] = s2; part_n[blockIdx.x] = s3; }
}

// the B <= CO_CG_BLOCKS partials of a pass through one tree, the same in every block: thread t adds t, t + 256, ... in ascending order
__device__ __forceinline__ double co_reduce_partials(const double* __restrict__ part, int B, double* wave_sums) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < B; b += CO_THREADS) acc += part[b];
    return co_block_sum(acc, wave_sums);
}

// One block: |b|, the threshold, the unknowns, the limit; the loop is over before it starts when there is no unknown or b = 0.
__global__ void __launch_bounds__(CO_THREADS) co_cg_begin_kernel(const double* __restrict__ part_bb, const double* __restrict__ part_n, int B,
                                                                 double tol, int maxiter, CoState* __restrict__ st) {
    __shared__ double wave_sums[CO_WAVES];
    const double bb = co_reduce_partials(part_bb, B, wave_sums);
    const double n = co_reduce_partials(part_n, B, wave_sums);        // exact: far below 2^53
    if (threadIdx.x == 0) {
        const int dflt = (int)(10.0 * sqrt(n));
        st->n = (long long)n;
        st->limit = maxiter > 0 ? maxiter : (dflt > 50 ? dflt : 50);
        st->thr = fmax(tol, 1e-5 * sqrt(bb));
        st->zero_x = (n > 0.0 && bb == 0.0) ? 1 : 0;
        st->flag = (n == 0.0 || bb == 0.0) ? 1 : 0;
        st->info = 0;
        st->iters = 0;
        st->rho[0] = 0.0; st->rho[1] = 0.0;
    }
}

__device__ __forceinline__ bool co_stopped(const CoState* st, int* s_flag) {
    if (threadIdx.x == 0) *s_flag = st->flag;             // one read per block: its waves must agree
    __syncthreads();
    return *s_flag != 0;
}

// Pass 1 of iteration `it`.  Finishes the reduction of r . r and r . z (from the setup or from pass 2 of it - 1), tests the limit and the
// stop rule -- every block comes to the same decision from the same partials; block 0 records it --, then p' = z + beta p and q = A p' by the
// 5-point stencil: a thread recomputes p' of its neighbours from p and z (p is double-buffered: no block waits for another), and leaves
// one partial of p' . q per block.  Land pixels hold 0 in every vector.
__global__ void __launch_bounds__(CO_THREADS) co_cg_pass1_kernel(int it, int H, int W, const unsigned char* __restrict__ code,
                                                                 const double* __restrict__ z, const double* __restrict__ p_old,
                                                                 double* __restrict__ p_new, double* __restrict__ q,
                                                                 const double* __restrict__ part_rr, const double* __restrict__ part_rz,
                                                                 double* __restrict__ part_pq, int B, CoState* __restrict__ st) {
    __shared__ double wave_sums[CO_WAVES];
    __shared__ int s_flag;
    if (co_stopped(st, &s_flag)) return;
    const double rr = co_reduce_partials(part_rr, B, wave_sums);
    const double rho = co_reduce_partials(part_rz, B, wave_sums);
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (it >= st->limit) {                                // block-uniform: the loop is exhausted, no final test
        if (first) { st->info = st->limit; st->flag = 1; }
        return;
    }
    if (sqrt(rr) < st->thr) {
        if (first) { st->info = 0; st->flag = 1; }
        return;
    }
    const bool start = it == 0;
    const double beta = start ? 0.0 : rho / st->rho[(it - 1) & 1];
    if (first) st->rho[it & 1] = rho;
    const int N = H * W;
    double pq = 0.0;
    for (int i = blockIdx.x * CO_THREADS + threadIdx.x; i < N; i += gridDim.x * CO_THREADS) {
        const unsigned char cd = code[i];
        double pn = 0.0, qv = 0.0;
        if (cd & 0x80) {
            const int y = i / W, x = i - y * W;
#define CO_NEWP(j) (start ? z[j] : beta * p_old[j] + z[j])
            pn = CO_NEWP(i);
            qv = (double)(cd & 7) * pn;
            if (y > 0) qv -= CO_NEWP(i - W);
            if (x > 0) qv -= CO_NEWP(i - 1);
            if (x < W - 1) qv -= CO_NEWP(i + 1);
            if (y < H - 1) qv -= CO_NEWP(i + W);
#undef CO_NEWP
            pq += pn * qv;
        }
        p_new[i] = pn; q[i] = qv;
    }
    const double s = co_block_sum(pq, wave_sums);
    if (threadIdx.x == 0) part_pq[blockIdx.x] = s;
}

// Pass 2 of iteration `it`: reduces the partials of p . q, alpha = rho / (p . q), x += alpha p, r -= alpha q, z = r / diag, and leaves one
// partial of r . r and of r . z per block.  Block 0 counts the iteration.
__global__ void __launch_bounds__(CO_THREADS) co_cg_pass2_kernel(int it, int N, const unsigned char* __restrict__ code,
                                                                 const double* __restrict__ p, const double* __restrict__ q,
                                                                 double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                                 const double* __restrict__ part_pq, double* __restrict__ part_rr,
                                                                 double* __restrict__ part_rz, int B, CoState* __restrict__ st) {
    __shared__ double wave_sums[CO_WAVES];
    __shared__ int s_flag;
    if (co_stopped(st, &s_flag)) return;
    const double pq = co_reduce_partials(part_pq, B, wave_sums);
    const double alpha = st->rho[it & 1] / pq;
    double rr = 0.0, rz = 0.0;
    for (int i = blockIdx.x * CO_THREADS + threadIdx.x; i < N; i += gridDim.x * CO_THREADS) {
        const unsigned char cd = code[i];
        if (!(cd & 0x80)) continue;
        const int diag = cd & 7;
        x[i] = x[i] + alpha * p[i];
        const double rv = r[i] - alpha * q[i];
        const double zv = rv * (diag > 0 ? 1.0 / (double)diag : 1.0);
        r[i] = rv; z[i] = zv;
        rr += rv * rv; rz += rv * zv;
    }
    const double s0 = co_block_sum(rr, wave_sums), s1 = co_block_sum(rz, wave_sums);
    if (threadIdx.x == 0) {
        part_rr[blockIdx.x] = s0; part_rz[blockIdx.x] = s1;
        if (blockIdx.x == 0) st->iters = it + 1;
    }
}

// np.allclose(x, 0): every |x| <= 1e-8.  One count per block of the unknowns that are not (NaN and infinities are not).
__global__ void __launch_bounds__(CO_THREADS) co_cg_far_kernel(int N, const unsigned char* __restrict__ code, const double* __restrict__ x,
                                                               const CoState* __restrict__ st, double* __restrict__ part_far) {
    __shared__ double wave_sums[CO_WAVES];
    const bool zero_x = st->zero_x != 0;
    double far = 0.0;
    for (int i = blockIdx.x * CO_THREADS + threadIdx.x; i < N; i += gridDim.x * CO_THREADS)
        if ((code[i] & 0x80) && !zero_x && !(fabs(x[i]) <= 1e-8)) far += 1.0;
    const double s = co_block_sum(far, wave_sums);
    if (threadIdx.x == 0) part_far[blockIdx.x] = s;
}

// out = the solution on the unknowns (1e-9 on all of them where all are close to 0, :160-161), a's own bits elsewhere; out may be a itself.
// Block 0 writes the level's two entries of info: the iterations, and scipy's info (the limit where the enqueued loop ran out unflagged).
__global__ void __launch_bounds__(CO_THREADS) co_cg_finish_kernel(int N, const unsigned char* __restrict__ code, const double* __restrict__ x,
                                                                  const double* a, const CoState* __restrict__ st,
                                                                  const double* __restrict__ part_far, int B, double* out, int* __restrict__ info) {
    __shared__ double wave_sums[CO_WAVES];
    const bool all_close = co_reduce_partials(part_far, B, wave_sums) == 0.0;
    const bool zero_x = st->zero_x != 0;
    for (int i = blockIdx.x * CO_THREADS + threadIdx.x; i < N; i += gridDim.x * CO_THREADS) {
        const double v = a[i];
        out[i] = (code[i] & 0x80) ? (all_close ? 1e-9 : (zero_x ? 0.0 : x[i])) : v;
    }
    if (info && blockIdx.x == 0 && threadIdx.x == 0) {
        info[0] = st->iters;
        info[1] = st->flag ? st->info : st->limit;
    }
}

}  // namespace td
