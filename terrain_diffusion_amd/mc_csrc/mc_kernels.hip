// Kernels of libtd_mc.so (include/td_mc.h): the reference's Minecraft terrain path (terrain_diffusion/inference/minecraft_api.py:
// _get_upsampled, _compute_climate_vars, _classify_biome, _binary_response; api.py: _get_terrain).
//
// Arithmetic is restated in tests/_mc_twin.py, which reproduces these kernels bit for bit; keep the two in step.  Contraction is off (and
// the library is built with -ffp-contract=off): every a * b + c below rounds twice, as NumPy does, unless written as fmaf.  Divisions and
// square roots that feed a decision are taken in float64 and rounded once (the correctly rounded fp32 result, whatever the fp32 flags).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace td {

constexpr int MC_TILE = 16;        // finish: 16 x 16 output pixels per workgroup, an 18 x 18 LDS tile of elev_padded
constexpr int MC_THREADS = 256;    // upsample, payload: threads per workgroup

// ---- noise: FastNoiseLite's Perlin / FBm structure (hash primes, quintic fade, 1.4247691104677813 gain, fractal bounding, weighted strength
// 0, seed + 1 per octave, lacunarity 2) with a 128-entry gradient table: unit vectors at angles (k + 1/2) 2 pi / 128, computed in float64 and
// rounded to fp32 (the angles of compose_kernels.hip's pn_grad).  The values are this package's own, not FastNoiseLite's.
__constant__ float2 MC_GRAD[128] = {
    {0x1.ffd8860000000p-1f, 0x1.9215600000000p-6f}, {0x1.fe9cda0000000p-1f, 0x1.2d520a0000000p-4f}, {0x1.fc26480000000p-1f, 0x1.f564e60000000p-4f}, {0x1.f876500000000p-1f, 0x1.5e21440000000p-3f},
    {0x1.f38f3a0000000p-1f, 0x1.c0b8260000000p-3f}, {0x1.ed740e0000000p-1f, 0x1.111d260000000p-2f}, {0x1.e6288e0000000p-1f, 0x1.4135ca0000000p-2f}, {0x1.ddb13c0000000p-1f, 0x1.7088540000000p-2f},
    {0x1.d4134e0000000p-1f, 0x1.9ef7940000000p-2f}, {0x1.c954b20000000p-1f, 0x1.cc66ea0000000p-2f}, {0x1.bd7c0a0000000p-1f, 0x1.f8ba4e0000000p-2f}, {0x1.b090a60000000p-1f, 0x1.11eb360000000p-1f},
    {0x1.a29a7a0000000p-1f, 0x1.26d0540000000p-1f}, {0x1.93a2240000000p-1f, 0x1.3affa20000000p-1f}, {0x1.83b0e00000000p-1f, 0x1.4e6cac0000000p-1f}, {0x1.72d0840000000p-1f, 0x1.610b760000000p-1f},
    {0x1.610b760000000p-1f, 0x1.72d0840000000p-1f}, {0x1.4e6cac0000000p-1f, 0x1.83b0e00000000p-1f}, {0x1.3affa20000000p-1f, 0x1.93a2240000000p-1f}, {0x1.26d0540000000p-1f, 0x1.a29a7a0000000p-1f},
    {0x1.11eb360000000p-1f, 0x1.b090a60000000p-1f}, {0x1.f8ba4e0000000p-2f, 0x1.bd7c0a0000000p-1f}, {0x1.cc66ea0000000p-2f, 0x1.c954b20000000p-1f}, {0x1.9ef7940000000p-2f, 0x1.d4134e0000000p-1f},
    {0x1.7088540000000p-2f, 0x1.ddb13c0000000p-1f}, {0x1.4135ca0000000p-2f, 0x1.e6288e0000000p-1f}, {0x1.111d260000000p-2f, 0x1.ed740e0000000p-1f}, {0x1.c0b8260000000p-3f, 0x1.f38f3a0000000p-1f},
    {0x1.5e21440000000p-3f, 0x1.f876500000000p-1f}, {0x1.f564e60000000p-4f, 0x1.fc26480000000p-1f}, {0x1.2d520a0000000p-4f, 0x1.fe9cda0000000p-1f}, {0x1.9215600000000p-6f, 0x1.ffd8860000000p-1f},
    {-0x1.9215600000000p-6f, 0x1.ffd8860000000p-1f}, {-0x1.2d520a0000000p-4f, 0x1.fe9cda0000000p-1f}, {-0x1.f564e60000000p-4f, 0x1.fc26480000000p-1f}, {-0x1.5e21440000000p-3f, 0x1.f876500000000p-1f},
    {-0x1.c0b8260000000p-3f, 0x1.f38f3a0000000p-1f}, {-0x1.111d260000000p-2f, 0x1.ed740e0000000p-1f}, {-0x1.4135ca0000000p-2f, 0x1.e6288e0000000p-1f}, {-0x1.7088540000000p-2f, 0x1.ddb13c0000000p-1f},
    {-0x1.9ef7940000000p-2f, 0x1.d4134e0000000p-1f}, {-0x1.cc66ea0000000p-2f, 0x1.c954b20000000p-1f}, {-0x1.f8ba4e0000000p-2f, 0x1.bd7c0a0000000p-1f}, {-0x1.11eb360000000p-1f, 0x1.b090a60000000p-1f},
    {-0x1.26d0540000000p-1f, 0x1.a29a7a0000000p-1f}, {-0x1.3affa20000000p-1f, 0x1.93a2240000000p-1f}, {-0x1.4e6cac0000000p-1f, 0x1.83b0e00000000p-1f}, {-0x1.610b760000000p-1f, 0x1.72d0840000000p-1f},
    {-0x1.72d0840000000p-1f, 0x1.610b760000000p-1f}, {-0x1.83b0e00000000p-1f, 0x1.4e6cac0000000p-1f}, {-0x1.93a2240000000p-1f, 0x1.3affa20000000p-1f}, {-0x1.a29a7a0000000p-1f, 0x1.26d0540000000p-1f},
    {-0x1.b090a60000000p-1f, 0x1.11eb360000000p-1f}, {-0x1.bd7c0a0000000p-1f, 0x1.f8ba4e0000000p-2f}, {-0x1.c954b20000000p-1f, 0x1.cc66ea0000000p-2f}, {-0x1.d4134e0000000p-1f, 0x1.9ef7940000000p-2f},
    {-0x1.ddb13c0000000p-1f, 0x1.7088540000000p-2f}, {-0x1.e6288e0000000p-1f, 0x1.4135ca0000000p-2f}, {-0x1.ed740e0000000p-1f, 0x1.111d260000000p-2f}, {-0x1.f38f3a0000000p-1f, 0x1.c0b8260000000p-3f},
    {-0x1.f876500000000p-1f, 0x1.5e21440000000p-3f}, {-0x1.fc26480000000p-1f, 0x1.f564e60000000p-4f}, {-0x1.fe9cda0000000p-1f, 0x1.2d520a0000000p-4f}, {-0x1.ffd8860000000p-1f, 0x1.9215600000000p-6f},
    {-0x1.ffd8860000000p-1f, -0x1.9215600000000p-6f}, {-0x1.fe9cda0000000p-1f, -0x1.2d520a0000000p-4f}, {-0x1.fc26480000000p-1f, -0x1.f564e60000000p-4f}, {-0x1.f876500000000p-1f, -0x1.5e21440000000p-3f},
    {-0x1.f38f3a0000000p-1f, -0x1.c0b8260000000p-3f}, {-0x1.ed740e0000000p-1f, -0x1.111d260000000p-2f}, {-0x1.e6288e0000000p-1f, -0x1.4135ca0000000p-2f}, {-0x1.ddb13c0000000p-1f, -0x1.7088540000000p-2f},
    {-0x1.d4134e0000000p-1f, -0x1.9ef7940000000p-2f}, {-0x1.c954b20000000p-1f, -0x1.cc66ea0000000p-2f}, {-0x1.bd7c0a0000000p-1f, -0x1.f8ba4e0000000p-2f}, {-0x1.b090a60000000p-1f, -0x1.11eb360000000p-1f},
    {-0x1.a29a7a0000000p-1f, -0x1.26d0540000000p-1f}, {-0x1.93a2240000000p-1f, -0x1.3affa20000000p-1f}, {-0x1.83b0e00000000p-1f, -0x1.4e6cac0000000p-1f}, {-0x1.72d0840000000p-1f, -0x1.610b760000000p-1f},
    {-0x1.610b760000000p-1f, -0x1.72d0840000000p-1f}, {-0x1.4e6cac0000000p-1f, -0x1.83b0e00000000p-1f}, {-0x1.3affa20000000p-1f, -0x1.93a2240000000p-1f}, {-0x1.26d0540000000p-1f, -0x1.a29a7a0000000p-1f},
    {-0x1.11eb360000000p-1f, -0x1.b090a60000000p-1f}, {-0x1.f8ba4e0000000p-2f, -0x1.bd7c0a0000000p-1f}, {-0x1.cc66ea0000000p-2f, -0x1.c954b20000000p-1f}, {-0x1.9ef7940000000p-2f, -0x1.d4134e0000000p-1f},
    {-0x1.7088540000000p-2f, -0x1.ddb13c0000000p-1f}, {-0x1.4135ca0000000p-2f, -0x1.e6288e0000000p-1f}, {-0x1.111d260000000p-2f, -0x1.ed740e0000000p-1f}, {-0x1.c0b8260000000p-3f, -0x1.f38f3a0000000p-1f},
    {-0x1.5e21440000000p-3f, -0x1.f876500000000p-1f}, {-0x1.f564e60000000p-4f, -0x1.fc26480000000p-1f}, {-0x1.2d520a0000000p-4f, -0x1.fe9cda0000000p-1f}, {-0x1.9215600000000p-6f, -0x1.ffd8860000000p-1f},
    {0x1.9215600000000p-6f, -0x1.ffd8860000000p-1f}, {0x1.2d520a0000000p-4f, -0x1.fe9cda0000000p-1f}, {0x1.f564e60000000p-4f, -0x1.fc26480000000p-1f}, {0x1.5e21440000000p-3f, -0x1.f876500000000p-1f},
    {0x1.c0b8260000000p-3f, -0x1.f38f3a0000000p-1f}, {0x1.111d260000000p-2f, -0x1.ed740e0000000p-1f}, {0x1.4135ca0000000p-2f, -0x1.e6288e0000000p-1f}, {0x1.7088540000000p-2f, -0x1.ddb13c0000000p-1f},
    {0x1.9ef7940000000p-2f, -0x1.d4134e0000000p-1f}, {0x1.cc66ea0000000p-2f, -0x1.c954b20000000p-1f}, {0x1.f8ba4e0000000p-2f, -0x1.bd7c0a0000000p-1f}, {0x1.11eb360000000p-1f, -0x1.b090a60000000p-1f},
    {0x1.26d0540000000p-1f, -0x1.a29a7a0000000p-1f}, {0x1.3affa20000000p-1f, -0x1.93a2240000000p-1f}, {0x1.4e6cac0000000p-1f, -0x1.83b0e00000000p-1f}, {0x1.610b760000000p-1f, -0x1.72d0840000000p-1f},
    {0x1.72d0840000000p-1f, -0x1.610b760000000p-1f}, {0x1.83b0e00000000p-1f, -0x1.4e6cac0000000p-1f}, {0x1.93a2240000000p-1f, -0x1.3affa20000000p-1f}, {0x1.a29a7a0000000p-1f, -0x1.26d0540000000p-1f},
    {0x1.b090a60000000p-1f, -0x1.11eb360000000p-1f}, {0x1.bd7c0a0000000p-1f, -0x1.f8ba4e0000000p-2f}, {0x1.c954b20000000p-1f, -0x1.cc66ea0000000p-2f}, {0x1.d4134e0000000p-1f, -0x1.9ef7940000000p-2f},
    {0x1.ddb13c0000000p-1f, -0x1.7088540000000p-2f}, {0x1.e6288e0000000p-1f, -0x1.4135ca0000000p-2f}, {0x1.ed740e0000000p-1f, -0x1.111d260000000p-2f}, {0x1.f38f3a0000000p-1f, -0x1.c0b8260000000p-3f},
    {0x1.f876500000000p-1f, -0x1.5e21440000000p-3f}, {0x1.fc26480000000p-1f, -0x1.f564e60000000p-4f}, {0x1.fe9cda0000000p-1f, -0x1.2d520a0000000p-4f}, {0x1.ffd8860000000p-1f, -0x1.9215600000000p-6f},};

__device__ __forceinline__ float mc_div(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float mc_sqrt(float a) { return (float)sqrt((double)a); }

__device__ __forceinline__ float mc_grad(const float2* g, uint32_t seed, uint32_t xp, uint32_t yp, float xd, float yd) {
    uint32_t h = (seed ^ xp ^ yp) * 0x27d4eb2du;
    const float2 v = g[(h ^ (h >> 15)) & 127u];
    return xd * v.x + yd * v.y;
}

// one octave at fp32 coordinates already multiplied by the frequency
__device__ __forceinline__ float mc_perlin(const float2* g, uint32_t seed, float x, float y) {
    const float fx = floorf(x), fy = floorf(y);
    const float xd0 = x - fx, yd0 = y - fy, xd1 = xd0 - 1.f, yd1 = yd0 - 1.f;
    const float xs = xd0 * xd0 * xd0 * (xd0 * (xd0 * 6.f - 15.f) + 10.f);
    const float ys = yd0 * yd0 * yd0 * (yd0 * (yd0 * 6.f - 15.f) + 10.f);
    const uint32_t x0 = (uint32_t)(int)fx * 501125321u, y0 = (uint32_t)(int)fy * 1136930381u;
    const uint32_t x1 = x0 + 501125321u, y1 = y0 + 1136930381u;
    const float a = mc_grad(g, seed, x0, y0, xd0, yd0), b = mc_grad(g, seed, x1, y0, xd1, yd0);
    const float c = mc_grad(g, seed, x0, y1, xd0, yd1), d = mc_grad(g, seed, x1, y1, xd1, yd1);
    const float xf0 = a + xs * (b - a), xf1 = c + xs * (d - c);
    return (xf0 + ys * (xf1 - xf0)) * 1.4247691104677813f;
}

// the single octaves n[0 .. octs) of a generator: seed + o at (x, y) * 2^o
template <int OCTS>
__device__ __forceinline__ void mc_octaves(const float2* g, uint32_t seed, float freq, float cx, float cy, float* n) {
    float x = cx * freq, y = cy * freq;
#pragma unroll
    for (int o = 0; o < OCTS; ++o) {
        n[o] = mc_perlin(g, seed + o, x, y);
        x *= 2.f; y *= 2.f;
    }
}

__device__ __forceinline__ float mc_bounding(int octs, float gain) {
    const float g = fabsf(gain);
    float amp = g, total = 1.f;
    for (int o = 1; o < octs; ++o) { total += amp; amp *= g; }
    return 1.f / total;
}

// FBm sum over precomputed octaves: total += n[o] * amp, amp *= gain, from amp = the fractal bounding
__device__ __forceinline__ float mc_fbm(const float* n, int octs, float gain) {
    float amp = mc_bounding(octs, gain), total = 0.f;
    for (int o = 0; o < octs; ++o) { total += n[o] * amp; amp *= gain; }
    return total;
}

// ---- upsample: rows [r0, r0 + H) x columns [c0, c0 + W) of F.interpolate(src, scale_factor=s, mode="bilinear", align_corners=False) for C
// channels.  torch's index and weight formula per axis (the source index as fmaf, which is how torch's CPU build evaluates it), both edge
// clamps; the weighted sum in float64 (products of floats are exact there), rounded once.  s == 1 copies, as torch does.
struct McAxis { long long i0, i1; double l0, l1; };

__device__ __forceinline__ McAxis mc_axis(long long u, int n_in, int s, float ratio) {
    McAxis a;
    if (s == 1) { a.i0 = a.i1 = u; a.l0 = 1.0; a.l1 = 0.0; return a; }
    float real = fmaf(ratio, (float)u + 0.5f, -0.5f);
    if (real < 0.f) real = 0.f;
    long long i0 = (long long)floorf(real);
    if (i0 > n_in - 1) i0 = n_in - 1;
    const float l1 = fminf(fmaxf(real - (float)i0, 0.f), 1.f);
    a.i0 = i0; a.i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    a.l1 = (double)l1; a.l0 = (double)(1.f - l1);
    return a;
}

__global__ void __launch_bounds__(MC_THREADS) mc_upsample_kernel(const float* __restrict__ src, int C, int Hn, int Wn, int s, float ratio,
                                                                 long long r0, long long c0, int H, int W, float* __restrict__ out) {
    // grid: (pixels / MC_THREADS, C); H W <= 2^26, so the pixel index and its division stay in 32 bits
    const unsigned hw = (unsigned)H * (unsigned)W;
    const unsigned p = blockIdx.x * MC_THREADS + threadIdx.x;
    if (p >= hw) return;
    const int ch = blockIdx.y;
    const size_t idx = (size_t)ch * hw + p;
    const int r = (int)(p / (unsigned)W), c = (int)(p - (unsigned)r * (unsigned)W);
    const McAxis ay = mc_axis(r0 + r, Hn, s, ratio), ax = mc_axis(c0 + c, Wn, s, ratio);
    const float* x = src + (size_t)ch * Hn * Wn;
    if (s == 1) { out[idx] = x[(size_t)ay.i0 * Wn + ax.i0]; return; }
    const double x00 = x[(size_t)ay.i0 * Wn + ax.i0], x01 = x[(size_t)ay.i0 * Wn + ax.i1];
    const double x10 = x[(size_t)ay.i1 * Wn + ax.i0], x11 = x[(size_t)ay.i1 * Wn + ax.i1];
    const double top = ax.l0 * x00 + ax.l1 * x01, bot = ax.l0 * x10 + ax.l1 * x11;
    out[idx] = (float)(ay.l0 * top + ay.l1 * bot);
}

// ---- finish: per pixel, the Sobel of elev_padded once, then the detail noise of _get_upsampled and / or _classify_biome.
struct McFinishArgs {
    const float* elev; long long elev_ld;       // the classifier's elevation and the detail's elev_smooth, row pitch elev_ld
    const float* padded;                        // (H + 2, W + 2)
    const float* climate; int has_climate;      // (>= 4, H, W) when has_climate
    const float* planes;                        // (7, H, W) in the reference's generator order, or null: built-in noise
    int H, W; long long i0, j0;                 // box and its absolute origin (noise coordinates: x = j0 + col, y = i0 + row)
    float detail_div, amp_c, amp_f, px_m, nr;   // fl32(40 P / 90), fl32(noise_scale 100), fl32(noise_scale 70), fl32(P), fl32(native res)
    int detail_on;                              // noise_scale > 0
    float biome_px;                             // fl32(pixel_size_m) of the classifier
    float bare_span;                            // fl32(1.19 - 0.7)
    float* elev_out; int16_t* biome_out;        // either may be null
};

__device__ __forceinline__ float mc_clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }   // NaN stays NaN, as torch.clamp

__device__ int16_t mc_classify(float e, float temp, float t_season, float precip, float p_cv, const float* n, float sr, float bare_span) {
    // noise perturbation (numpy fp32: temp_noise = 0.4 c + 0.2 f; precip * (1 + 0.2 p); snow = 3 c + 2 f)
    precip = precip < 0.f ? 0.f : precip;
    temp = temp + (0.4f * n[0] + 0.2f * n[1]);
    precip = precip * (1.0f + 0.2f * n[2]);
    const float snow_noise = 3.0f * n[3] + 2.0f * n[4];
    // _compute_climate_vars
    const float t_std = mc_div(t_season, 100.f);
    float t_eff = temp + 0.5f * t_std;
    t_eff = t_eff < 0.f ? 0.f : t_eff;
    float pet = 250.f + 25.f * t_eff + 0.7f * (t_eff * t_eff);
    pet = pet < 250.f ? 250.f : pet;
    const float pet1 = pet < 1.f ? 1.f : pet;
    const float aridity = mc_div(precip, pet1);
    float pc = mc_div(p_cv, 100.f);
    pc = pc > 1.f ? 1.f : pc;
    const float tm = aridity * (1.f - 0.35f * pc);
    float amplitude = t_std * 1.414f;
    amplitude = amplitude < 0.1f ? 0.1f : amplitude;
    const float x = mc_div(5.f - temp, amplitude);
    const float xc = x < -1.f ? -1.f : (x > 1.f ? 1.f : x);
    const float as = (float)asin((double)xc);
    float gs = 365.f * (0.5f - mc_div(as, 3.14159f));
    gs = x <= -1.f ? 365.f : (x >= 1.f ? 0.f : gs);
    const bool tropical = (temp >= 18.f) & (t_std < 5.f);
    // slope, tree classes
    const bool is_steep = sr > 0.78f;
    const float gsf = mc_clamp01(mc_div(gs - 60.f, 90.f));
    const float eff = tm * gsf;
    const float mf = mc_clamp01(mc_div(tm - 0.35f, 0.45f));
    const float bt = 0.7f + bare_span * mf;
    bool none = eff < 0.2f;
    const bool barren = (tm < 0.05f) | (gs < 60.f);
    bool sparse = !none & (eff < 0.5f);
    bool forest = !none & (eff >= 0.5f) & (eff < 0.8f);
    bool dense = !none & (eff >= 0.8f) & (eff < 1.3f);
    bool rain = !none & (eff >= 1.3f);
    const bool medium = (sr >= 0.62f) & (sr < bt);
    const bool bare = sr >= bt;
    const bool had = forest | dense | rain;
    sparse = sparse | (medium & had);
    forest = forest & !medium; dense = dense & !medium; rain = rain & !medium;
    none = none | bare;
    sparse = sparse & !bare; forest = forest & !bare; dense = dense & !bare; rain = rain & !bare;
    const bool snow = ((temp + snow_noise) < 0.f) & (precip > 150.f) & !is_steep;
    const float alt = e < 0.f ? 0.f : e;     // torch.clamp(min=0): NaN stays NaN
    const bool ocean = e < 0.f, mountains = alt > 2500.f, lowland = alt < 200.f;
    const bool frozen = temp < -5.f;
    const bool cold = (temp >= -5.f) & (temp < 5.f);
    const bool cool = (temp >= 5.f) & (temp < 12.f);
    const bool temperate = (temp >= 12.f) & (temp < 20.f);
    const bool warm = (temp >= 20.f) & (temp < 26.f);
    const bool hot = temp >= 26.f;
    const bool steppe_dry = (tm < 0.35f) | (precip < 350.f);
    // the decision tree: the reference's masks in its order, later writes winning
    int out = 1;
    if (ocean) {
        const bool of = frozen, oc = cold & !frozen, ow = warm | hot;
        if (of) out = 48;
        if (oc) out = 46;
        if (ow) out = 41;
        if (!of & !oc & !ow) out = 44;
    } else if (mountains) {
        if (bare & snow) out = 33;
        if (bare & !snow) out = 35;
        if (!bare) {
            if (snow & none) out = 32;
            if (snow & (sparse | forest)) out = 116;
            if (snow & (dense | rain)) out = 16;
            if (!snow & none & barren) out = 19;
            const bool mcs = !snow & none & !barren & steppe_dry;
            if (mcs) out = 31;
            if (!snow & none & !barren & !mcs) out = 1;
            if (!snow & (sparse | forest)) out = 115;
            if (!snow & (dense | rain)) out = 15;
        }
    } else {
        bool land = true;
        if (snow & none) { out = 3; land = false; }
        if (land & snow & (sparse | forest)) { out = 116; land = false; }
        else if (land & snow & (dense | rain)) { out = 16; land = false; }
        if (land & !snow & none) {
            const bool desert = warm | hot;
            const bool ws = (cold | cool | temperate) & !lowland & barren;
            const bool cs = steppe_dry & !barren;
            if (desert) out = 5;
            if (ws) out = 31;
            if (cs) out = 31;
            if (!desert & !ws & !cs) out = 1;
            land = false;
        }
        if (land & !snow & (sparse | forest)) {
            if (hot) out = 23;
            if (warm & sparse & !medium) out = 17;
            if (warm & forest) out = 108;
            if (temperate) out = 108;
            if (cool | cold) out = 115;
            land = false;
        }
        if (land & !snow & dense) {
            const bool jd = hot, sw = warm & lowland, tdn = (cool | cold) & !jd & !sw;
            if (jd) out = 23;
            if (sw) out = 6;
            if (tdn) out = 15;
            if (!jd & !sw & !tdn) out = 8;
            land = false;
        }
        if (land & !snow & rain) {
            const bool jr = hot | (warm & tropical), swr = !jr & lowland, tr = (cool | cold) & !jr & !swr;
            if (jr) out = 23;
            if (swr) out = 6;
            if (tr) out = 15;
            if (!jr & !swr & !tr) out = 8;
            land = false;
        }
        if (land) out = 1;
    }
    if (bare & !ocean & !mountains) out = snow ? 33 : 35;
    return (int16_t)out;
}

__global__ void __launch_bounds__(MC_TILE * MC_TILE) mc_finish_kernel(McFinishArgs a) {
    __shared__ float tile[MC_TILE + 2][MC_TILE + 3];
    __shared__ float2 grad[128];
    const int tx = threadIdx.x % MC_TILE, ty = threadIdx.x / MC_TILE;
    const int bc = blockIdx.x * MC_TILE, br = blockIdx.y * MC_TILE;
    const int PW = a.W + 2, PH = a.H + 2;
    for (int k = threadIdx.x; k < (MC_TILE + 2) * (MC_TILE + 2); k += MC_TILE * MC_TILE) {
        const int r = k / (MC_TILE + 2), c = k % (MC_TILE + 2);
        const int gr = br + r, gc = bc + c;
        tile[r][c] = (gr < PH && gc < PW) ? a.padded[(size_t)gr * PW + gc] : 0.f;
    }
    if (threadIdx.x < 128) grad[threadIdx.x] = MC_GRAD[threadIdx.x];
    __syncthreads();
    const int row = br + ty, col = bc + tx;
    if (row >= a.H || col >= a.W) return;
    const size_t pix = (size_t)row * a.W + col, hw = (size_t)a.H * a.W;
    // Sobel / 8 of the 3 x 3 window (tile rows ty .. ty + 2), the centre tap only propagating NaN as the reference's zero weights do
    const float a00 = tile[ty][tx], a01 = tile[ty][tx + 1], a02 = tile[ty][tx + 2];
    const float a10 = tile[ty + 1][tx], a11 = tile[ty + 1][tx + 1], a12 = tile[ty + 1][tx + 2];
    const float a20 = tile[ty + 2][tx], a21 = tile[ty + 2][tx + 1], a22 = tile[ty + 2][tx + 2];
    const float gx = ((a02 - a00) + (a12 - a10) * 2.f) + (a22 - a20);
    const float gy = ((a20 - a00) + (a21 - a01) * 2.f) + (a22 - a02);
    const float dx = gx * 0.125f, dy = gy * 0.125f;
    const float g = mc_sqrt(dx * dx + dy * dy) + 0.f * a11;
    const float e = a.elev[(size_t)row * a.elev_ld + col];
    const float cx = (float)(a.j0 + col), cy = (float)(a.i0 + row);
    if (a.elev_out) {
        float out = e;
        if (a.detail_on) {
            float nc, nf;
            if (a.planes) {
                nc = a.planes[5 * hw + pix]; nf = a.planes[6 * hw + pix];
            } else {
                float o[3];
                mc_octaves<3>(grad, 99999u, (float)(1.0 / 24.0), cx, cy, o);
                nc = mc_fbm(o, 3, 0.5f);
                mc_octaves<2>(grad, 88888u, (float)(1.0 / 6.0), cx, cy, o);
                nf = mc_fbm(o, 2, 0.6f);
            }
            const float sd = (float)mc_clamp01(mc_div(g, a.detail_div));
            const double sdd = (double)sd;
            const float sf = (float)(sdd * sqrt(sdd));                 // pow(1.5), rounded once
            const float ac = mc_div(sf * a.amp_c * a.px_m, a.nr);
            const float af = mc_div(sf * a.amp_f * a.px_m, a.nr);
            const float land = e >= 0.f ? 1.f : 0.f;
            out = e + (nc * ac + nf * af) * land;
        }
        a.elev_out[pix] = out;
    }
    if (a.biome_out) {
        int16_t b = 1;
        if (a.has_climate) {
            float n[5];
            if (a.planes) {
#pragma unroll
                for (int k = 0; k < 5; ++k) n[k] = a.planes[k * hw + pix];
            } else {
                // _TEMP_NOISE, _SNOW_NOISE and the first three octaves of _PRECIP_NOISE are the same singles; so are the two fine ones
                float o[5], f[2];
                mc_octaves<5>(grad, 12345u, (float)(1.0 / 500.0), cx, cy, o);
                mc_octaves<2>(grad, 54321u, (float)(1.0 / 128.0), cx, cy, f);
                n[0] = n[3] = mc_fbm(o, 3, 0.5f);
                n[1] = n[4] = mc_fbm(f, 2, 0.5f);
                n[2] = mc_fbm(o, 5, 0.5f);
            }
            const float sr = mc_div(g, a.biome_px);
            b = mc_classify(e, a.climate[pix], a.climate[hw + pix], a.climate[2 * hw + pix], a.climate[3 * hw + pix], n, sr, a.bare_span);
        }
        a.biome_out[pix] = b;
    }
}

// ---- the seven built-in noise planes (7, H, W) of the box at absolute (i0, j0), in the reference's generator order: what td_mc_finish
// evaluates when it is given no planes
__global__ void __launch_bounds__(MC_THREADS) mc_noise_kernel(int H, int W, long long i0, long long j0, float* __restrict__ out) {
    __shared__ float2 grad[128];
    if (threadIdx.x < 128) grad[threadIdx.x] = MC_GRAD[threadIdx.x];
    __syncthreads();
    const long long hw = (long long)H * W;
    const long long p = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (p >= hw) return;
    const int r = (int)(p / W), c = (int)(p - (long long)r * W);
    const float cx = (float)(j0 + c), cy = (float)(i0 + r);
    float o[5], f[2];
    mc_octaves<5>(grad, 12345u, (float)(1.0 / 500.0), cx, cy, o);
    mc_octaves<2>(grad, 54321u, (float)(1.0 / 128.0), cx, cy, f);
    out[p] = out[3 * hw + p] = mc_fbm(o, 3, 0.5f);
    out[hw + p] = out[4 * hw + p] = mc_fbm(f, 2, 0.5f);
    out[2 * hw + p] = mc_fbm(o, 5, 0.5f);
    mc_octaves<3>(grad, 99999u, (float)(1.0 / 24.0), cx, cy, o);
    out[5 * hw + p] = mc_fbm(o, 3, 0.5f);
    mc_octaves<2>(grad, 88888u, (float)(1.0 / 6.0), cx, cy, f);
    out[6 * hw + p] = mc_fbm(f, 2, 0.6f);
}

// ---- payload: clip(floor(elev), -32768, 32767) as int16 (NaN written as 0), then the biome ids; one buffer, copied to the host in one piece
__global__ void __launch_bounds__(MC_THREADS) mc_payload_kernel(const float* __restrict__ elev, const int16_t* __restrict__ biome, long long n,
                                                                int16_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= n) return;
    const float f = floorf(elev[i]);
    out[i] = (int16_t)(f != f ? 0.f : (f < -32768.f ? -32768.f : (f > 32767.f ? 32767.f : f)));
    if (biome) out[n + i] = biome[i];
}

}  // namespace td
