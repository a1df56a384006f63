// Host runtime behind the C-ABI of include/td_engine.h: weight folding/packing, the EDMUnet2D execution plan
// (which fused conv op consumes which tensor), the sampler loops, hipGraph capture.  gfx950 only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>
#include <unordered_map>

#include "../../include/td_engine.h"
#include "td_device.h"
#include "conv_select.h"
#include "model_graph.h"

// single translation unit: kernels are compiled together with the host runtime
#include "conv_igemm.hip"
#include "conv_glds.hip"
#include "conv_glds_wide.hip"
#include "conv_glds_wide16.hip"
#include "conv_sb.hip"
#include "conv_s16.hip"
#include "conv_fewcout.hip"
#include "small_kernels.hip"
#include "compose_kernels.hip"
#include "attn_mfma.hip"
#include "ae_kernels.hip"

using namespace td;

// element-type dispatch for the kernels that exist in fp32 / bf16 / fp16 form (T_ is the storage type of the model `U`)
#define TD_DISPATCH_T(U, ...)                                                       \
    do {                                                                             \
        if ((U)->dt == TD_DTYPE_BF16) { typedef __bf16 T_; __VA_ARGS__; }            \
        else if ((U)->dt == TD_DTYPE_F16) { typedef _Float16 T_; __VA_ARGS__; }      \
        else { typedef float T_; __VA_ARGS__; }                                      \
    } while (0)

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess) return fail(TD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// ------------------------------------------------------------------------------------------------ helpers
static inline uint16_t f2h(float f) {  // IEEE binary16, round-to-nearest-even (the host compiler's _Float16 conversion)
    _Float16 h = (_Float16)f;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
static inline uint16_t f2bf(float f) {  // round-to-nearest-even, NaN-preserving
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// Every C-ABI entry point runs on its engine's device and leaves the caller's current device as it found it.
struct DevGuard {
    int prev = -1, cur = -1;
    explicit DevGuard(int dev) : cur(dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); }
    ~DevGuard() { if (prev >= 0 && prev != cur) (void)hipSetDevice(prev); }
    DevGuard(const DevGuard&) = delete;
    DevGuard& operator=(const DevGuard&) = delete;
};

// Per-call device scratch (I/O staging, descriptor tables, intermediate planes).  hipMalloc / hipFree cost tens of microseconds and hipFree
// waits for the device, so scratch is recycled: a buffer handed back at the end of a call may be given to the next call at once, because all of
// an engine's work is enqueued on ONE stream and the stream orders the two uses (td_engine_set_stream drains the stream before it changes).
struct ScratchPool {
    std::vector<std::pair<void*, size_t>> idle;
    size_t idle_bytes = 0;
    ~ScratchPool() { for (auto& b : idle) (void)hipFree(b.first); }
    hipError_t take(size_t n, void** p, size_t* got) {
        int best = -1;
        for (int i = 0; i < (int)idle.size(); ++i)
            if (idle[i].second >= n && idle[i].second <= 4 * n + 4096 && (best < 0 || idle[i].second < idle[best].second)) best = i;
        if (best >= 0) { *p = idle[best].first; *got = idle[best].second; idle_bytes -= *got; idle[best] = idle.back(); idle.pop_back(); return hipSuccess; }
        *got = (n + 4095) / 4096 * 4096;
        return hipMalloc(p, *got);
    }
    void give(void* p, size_t n) {
        idle.emplace_back(p, n); idle_bytes += n;
        while (idle_bytes > ((size_t)1 << 30) || idle.size() > 64) {   // bounded: drop the oldest (hipFree waits for the device; rare)
            (void)hipFree(idle.front().first); idle_bytes -= idle.front().second; idle.erase(idle.begin());
        }
    }
};

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ScratchPool* pool = nullptr;   // set: p came from the pool and goes back to it
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    void release() { if (p) { if (pool) pool->give(p, bytes); else (void)hipFree(p); p = nullptr; pool = nullptr; } }
    ~DevBuf() { release(); }
    hipError_t scratch(ScratchPool& sp, size_t n) {   // uninitialised per-call scratch
        release();
        hipError_t e = sp.take(n ? n : 16, &p, &bytes);
        if (e == hipSuccess) pool = &sp; else p = nullptr;
        return e;
    }
    hipError_t alloc(size_t n, bool zero = true) {
        release();
        bytes = n ? n : 16;
        hipError_t e = hipMalloc(&p, bytes);
        // hipMemset on device memory is asynchronous and runs on the NULL stream, which the engine's non-blocking stream does not wait
        // for: without the synchronise a kernel launched right after could be overtaken by the zero fill (allocations are setup-time)
        if (e == hipSuccess && zero) { e = hipMemset(p, 0, bytes); if (e == hipSuccess) e = hipDeviceSynchronize(); }
        return e;
    }
};
typedef std::unique_ptr<DevBuf> Buf;

static bool is_device_ptr(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// Pinned host staging for the small uploads (timesteps, descriptor tables, tap tables) of calls that only enqueue (option "async"): the source
// of a hipMemcpyAsync has to stay valid until the copy has run, and the caller's arrays do not.  Two halves; leaving a half records an event
// behind everything enqueued from it, entering a half waits for its event (long past, in practice).
struct PinnedRing {
    static constexpr size_t HALF = (size_t)2 << 20;
    unsigned char* base = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
    int cur = 0;
    size_t used = 0;
    ~PinnedRing() { if (base) (void)hipHostFree(base); for (auto e : ev) if (e) (void)hipEventDestroy(e); }
    // copies `bytes` from src into the ring; nullptr when it cannot (too large / allocation failure): the caller then ends the call synchronously
    const void* stage(const void* src, size_t bytes, hipStream_t st) {
        const size_t need = (bytes + 63) / 64 * 64;
        if (need > HALF) return nullptr;
        if (!base) {
            if (hipHostMalloc((void**)&base, 2 * HALF, hipHostMallocDefault) != hipSuccess) { base = nullptr; (void)hipGetLastError(); return nullptr; }
            for (auto& e : ev) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        }
        if (used + need > HALF) {
            if (hipEventRecord(ev[cur], st) != hipSuccess) return nullptr;
            pending[cur] = true;
            cur ^= 1; used = 0;
            if (pending[cur]) { if (hipEventSynchronize(ev[cur]) != hipSuccess) return nullptr; pending[cur] = false; }
        }
        unsigned char* d = base + (size_t)cur * HALF + used;
        used += need;
        memcpy(d, src, bytes);
        return d;
    }
    void reset() { pending[0] = pending[1] = false; used = 0; }   // after a stream synchronise: nothing is in flight
};

struct td_engine {
    ScratchPool scratch;       // first member: destroyed last, after every buffer that came from it
    PinnedRing ring;
    bool call_host_src = false;   // this call copied from a caller-owned host array that could not be staged: it must end synchronously
    int device = 0;
    int n_cus = 256;
    void* zeros = nullptr;     // 4 KiB of zeros: a readable page of zeros for the kernels (ConvParams::zeros)
    hipStream_t stream = nullptr;   // the stream every call enqueues on: the engine's own, or the caller's (td_engine_set_stream)
    hipStream_t own_stream = nullptr;
    hipStream_t stream2 = nullptr;  // second lane of the batched EDM sampler (sample_edm_impl): two half-batches run concurrently
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;   // its ordering against the first lane's stream (which may be the caller's)
    std::vector<std::unique_ptr<struct DevBuf>> deferred;  // option "async": staging buffers of enqueued calls, released by td_engine_synchronize
    std::map<std::string, int64_t> opt;
    // scratch for I/O staging
    std::vector<Buf> keep;
    // "profile" option: HIP events around every conv launch (eager mode), accumulated here
    double prof_conv_ms = 0.0, prof_other_ms = 0.0;
    int64_t prof_conv_launches = 0, prof_other_launches = 0;
    std::map<std::string, std::pair<double, int64_t>> prof_ops;  // label -> (ms, launches)
    double prof_glds_ms = 0.0, prof_glds_flop = 0.0;             // the LDS-DMA conv kernel family alone
    int64_t prof_glds_launches = 0;
    std::map<int, std::unique_ptr<struct DevBuf>> wwin;   // linear weight window per tile size, uploaded once (td_gather_regions)
    int64_t option(const char* k, int64_t dflt) const { auto it = opt.find(k); return it == opt.end() ? dflt : it->second; }
};

// host array -> device memory on the engine's stream.  Option "async": through the pinned ring, so that the call may return before the copy has run
static int upload(td_engine* e, void* dst, const void* src, size_t bytes) {
    if (!bytes) return TD_OK;
    if (e->option("async", 0) != 0) {
        if (const void* pinned = e->ring.stage(src, bytes, e->stream)) { HIP_TRY(hipMemcpyAsync(dst, pinned, bytes, hipMemcpyHostToDevice, e->stream)); return TD_OK; }
        e->call_host_src = true;
    }
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream));
    return TD_OK;
}

// The scope of one C-ABI call: the device guard, the call's staging buffers, its host outputs and ONE flag -- "every caller buffer of this call is
// device memory" -- from which finish() decides how the call ends.  An entry point names each caller pointer once, by what it is:
//   in      a tensor that may be host or device            table    a small array the ABI defines as host (`*_host`, tap tables, descriptors)
//   out     a result that may be host or device            inout    a host-or-device buffer updated in place
//   direct  a pointer the entry point copies itself        scratch / keep   device memory that lives to the end of the call
// Host arrays that uploads read (the job structs below) are declared BEFORE the Call, so that they outlive it: a call that returns without
// finish() -- an error -- waits in the destructor for the uploads it enqueued before those arrays go.
struct Call {
    td_engine* const e;
    DevGuard dg;
    std::vector<Buf> hold;
    struct HostOut { void* host; const void* dev; size_t bytes; };
    std::vector<HostOut> outs;
    bool all_device = true;   // no caller buffer of this call is host memory
    bool uploaded = false;    // a copy from a host array has been enqueued
    bool finished = false;
    explicit Call(td_engine* e_) : e(e_), dg(e_->device) {}
    ~Call() {
        if (finished) return;
        e->call_host_src = false;
        if (uploaded) (void)hipStreamSynchronize(e->stream);
    }
    void keep(Buf b) { hold.push_back(std::move(b)); }
    template <typename T> int scratch(size_t bytes, T** p) {   // uninitialised
        Buf b(new DevBuf());
        HIP_TRY(b->scratch(e->scratch, bytes));
        *p = (T*)b->p;
        keep(std::move(b));
        return TD_OK;
    }
    int up(void* dst, const void* src, size_t bytes) { uploaded = true; return upload(e, dst, src, bytes); }
    // does not mark the call: through the pinned ring it may still end enqueue-only (upload's call_host_src says when it may not)
    template <typename T> int table(const T* src, size_t bytes, const T** dev) {
        T* p;
        int rc = scratch(bytes, &p);
        *dev = p;
        return rc ? rc : up(p, src, bytes);
    }
    template <typename T> int in(const T* src, size_t bytes, const T** dev) {
        *dev = src;
        if (direct(src)) return TD_OK;
        return table(src, bytes, dev);
    }
    template <typename T> int out(T* dst, size_t bytes, T** dev) { return inout(dst, bytes, false, dev); }
    // host: device scratch now (`read`: filled from the caller's buffer), copied back by finish
    template <typename T> int inout(T* ptr, size_t bytes, bool read, T** dev) {
        *dev = ptr;
        if (direct(ptr)) return TD_OK;
        int rc = scratch(bytes, dev);
        if (rc) return rc;
        outs.push_back({ptr, *dev, bytes});
        if (read) { uploaded = true; HIP_TRY(hipMemcpyAsync(*dev, ptr, bytes, hipMemcpyHostToDevice, e->stream)); }
        return TD_OK;
    }
    // residency of a caller pointer (NULL counts as device: nothing of the host is read through it)
    bool direct(const void* p) {
        const bool dev = !p || is_device_ptr(p);
        all_device = all_device && dev;
        return dev;
    }
    // End of the call: host outputs are copied back behind the work and the stream is waited for ONCE.  Default: the call is synchronous (results
    // complete on return).  With engine option "async" = 1 and only device pointers involved, the work stays enqueued on e->stream -- typically the
    // caller's own stream (td_engine_set_stream), so that it is ordered with the caller's other GPU work without a host synchronisation -- and the
    // call's staging buffers are parked until td_engine_synchronize.  `always_sync`: the entry points that never honoured "async".
    int finish(bool always_sync = false) {
        for (const HostOut& o : outs) HIP_TRY(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, e->stream));
        const bool host_src = e->call_host_src;
        if (!always_sync && all_device && !host_src && e->option("async", 0) != 0) {
            // pooled scratch goes straight back to the pool (the stream orders its next use behind this call's work); buffers that would be
            // hipFree'd -- which waits for the device -- are parked until the next synchronise
            if (e->deferred.size() > 256) { HIP_TRY(hipStreamSynchronize(e->stream)); e->deferred.clear(); e->ring.reset(); }
            for (auto& b : hold) if (b && !b->pool) e->deferred.push_back(std::move(b));
            hold.clear();
        } else {
            HIP_TRY(hipStreamSynchronize(e->stream));
            e->ring.reset();
        }
        e->call_host_src = false;
        finished = true;
        return TD_OK;
    }
};

// ------------------------------------------------------------------------------------------------ model description
struct Param : GraphParam {
    std::vector<float> data;
    bool set = false;
    int64_t numel() const { int64_t n = 1; for (int i = 0; i < ndim; ++i) n *= shape[i]; return n; }
};

// weights of one fused conv op: its K-segments' weight side with the folded tensor each slices (valid during finalize)
struct WSeg : GraphSeg {
    const std::vector<float>* w = nullptr;  // folded [cout][cin_tot][k][k]
};
struct ConvWeights {
    std::vector<WSeg> segs;
    int cout = 0, cout_pad = 0;
    Buf packed;
    int ksteps = 0;
    Buf packed_sb;             // 16-bit modes: the same weights in MFMA-fragment order for the small-batch flavour (conv_sb.hip); made the first
                               // time a plan puts this op on that flavour (ensure_packed_sb): never with option "sb" = 0 / "batch_invariant" = 1
    size_t packed_bytes = 0;   // bytes of weights in `packed` (without its tail padding)
    Buf packed_s16;            // the fragment order of the deep-level latency flavour (conv_s16.hip), likewise made on first use
    int sb_n3 = 0, sb_g1 = 0;  // its leading 3x3 K-groups / trailing 1x1 K-groups (sb_n3 < 0: segment order not supported by that flavour)
};

struct Tensor {
    void* ptr = nullptr;
    int C = 0, cstride = 0, H = 0, W = 0;
    float* sumsq = nullptr;
    int nparts = 0;
};

struct Op {
    enum Kind { CONV, ATTN } kind = CONV;
    ConvParams p;
    ConvSel sel;               // kernel, tile and split of this op (conv_select.h)
    int cvec_off = -1;         // EPI_EMB_SILU: offset of this block's c vector
    double k_alg = 0.0;        // sum over the K-segments of (real input channels x taps): the algorithmic K of the op (profile labels, roofline FLOP)
    int out_C = 0, out_H = 0, out_W = 0;  // output tensor geometry (debug read-back)
    // ATTN
    const void* qkv = nullptr; void* att = nullptr; int tokens = 0, C = 0;
    void* attn_ws = nullptr;   // bf16 mode: packed Qp | Kp | Vt operands of the MFMA attention kernel (attn_mfma.hip)
    std::string label;
};

// Everything a captured EDM sampler graph has baked into its kernel arguments: the plan's graph is replayed only for a call with an equal key.
struct GraphKey {
    std::vector<float> sigmas;
    float sigma_data = 0.f;
    int solver_order = 0;
    int lof = -1, fuse = -1, stop = -2;      // engine options "lower_order_final", "fuse_solver", "sampler_stop_after"
    const void* guide = nullptr;             // guide plan / its modulation buffer / scale (autoguidance)
    const void* guide_cvec = nullptr;
    float gscale = 0.f;
    float alpha = 1.f;                       // score-scaling factor and its (cos t_i, sin t_i) pairs
    std::vector<float> cs;
    bool operator==(const GraphKey& o) const {
        return std::tie(sigmas, sigma_data, solver_order, lof, fuse, stop, guide, guide_cvec, gscale, alpha, cs) ==
               std::tie(o.sigmas, o.sigma_data, o.solver_order, o.lof, o.fuse, o.stop, o.guide, o.guide_cvec, o.gscale, o.alpha, o.cs);
    }
};

struct Plan {
    int N = 0, H = 0, W = 0;
    std::vector<Op> ops;
    std::vector<Buf> bufs;
    void* xin = nullptr;       // NHWC input (T), cstride = chunk
    float* F = nullptr;        // NHWC fp32 model output, stride 8
    float* partial = nullptr;
    // sampler state
    Buf x, m1, m2, xt, cond, emb, cvec, tsteps;
    int cvec_rows = 0;         // rows emb / cvec are allocated for
    int cvec_written = 0;      // rows the last compute_cvecs wrote (read-back labels "@emb:rows" / "@cvec:rows")
    // graph cache for the EDM loop
    hipGraphExec_t graph = nullptr;
    GraphKey graph_key;        // what `graph` was captured under
    size_t bytes = 0;          // device memory owned by this plan (activations, partials, sampler state)
    uint64_t last_use = 0;     // LRU stamp (td_unet::use_clock)
    void drop_graph() { if (graph) { (void)hipGraphExecDestroy(graph); graph = nullptr; } }
    ~Plan() { drop_graph(); }
};

struct td_unet {
    td_engine* eng = nullptr;
    td_unet_config cfg;
    // Graph kind.  0: the EDMUnet2D (encoder + skip-concat decoder, modulated by an embedding).  The two stacks of the EDMAutoencoder have no embedding
    // (emb_channels = 0: a block's epilogue is mp_silu(y), unet_block.py:133-134 -- run as EPI_EMB_SILU on a modulation row of 1.0f, which is exact):
    // 1: encoder only, out_conv on the bottleneck (edm_unet.py:107-139 with encode_only); 2: skip-less decoder behind a 1x1 decoder_conv (edm_autoencoder.py:86-103)
    int kind = 0;
    ModelGraph g;              // blocks, parameters and fused ops (model_graph.h): finalize packs its weight side, build_plan wires its activation side
    Buf d_ones;                // kinds 1 and 2: the all-ones modulation row every block reads (cvec stride 0)
    bool bf16 = false;         // 16-bit storage (bf16 OR fp16): 64-channel K chunks, LDS-DMA / small-batch conv flavours available
    int dt = TD_DTYPE_F32;     // TD_DTYPE_*
    int chunk = 32;            // channels per 128-byte K chunk
    std::vector<Param> params;
    std::map<std::string, int> pindex;
    std::map<std::string, std::vector<float>> folded;
    std::vector<ConvWeights> convw;   // by index into g.ops (attention ops own none)
    bool finalized = false;
    bool prefolded = false;    // parameters already carry the MP normalisation and gains (host folded them)
    // embedding weights on device (fp32)
    Buf d_freqs, d_wnoise, d_wcond, d_fourier, d_wemb, d_blk_woff, d_blk_coff, d_blk_cout;
    EmbDesc embd;              // conditional-input layout of the embedding kernel
    int cond_row_len = 0;
    int n_blocks = 0;
    std::map<std::string, std::unique_ptr<Plan>> plans;
    uint64_t use_clock = 0;
    size_t esize() const { return bf16 ? 2 : 4; }
};

// the model's graph (model_graph.h) and a slot for every parameter it names
static int init_graph(td_unet* u, const int32_t* lpb_dec) {
    int rc = build_model_graph(u->cfg, u->kind, lpb_dec, u->chunk, u->g);
    if (rc) return fail(rc, u->g.err);
    for (const GraphParam& gp : u->g.params) {
        Param p;
        static_cast<GraphParam&>(p) = gp;
        u->pindex[p.name] = (int)u->params.size();
        u->params.push_back(std::move(p));
    }
    return TD_OK;
}

// mp_layers.py:203-213 (eval): W / (1e-4 + ||W||_2 / sqrt(numel)) * gain / sqrt(fan_in)
static void fold(const Param& p, float gain, std::vector<float>& out, bool prefolded) {
    const int64_t n = p.numel();
    if (prefolded) { out = p.data; return; }
    double ss = 0.0;
    for (int64_t i = 0; i < n; ++i) ss += (double)p.data[i] * p.data[i];
    const int64_t fan_in = n / p.shape[0];
    const double scale = (double)gain / ((1e-4 + sqrt(ss) / sqrt((double)n)) * sqrt((double)fan_in));
    out.resize(n);
    for (int64_t i = 0; i < n; ++i) out[i] = (float)(p.data[i] * scale);
}

static const Param& P(td_unet* u, const std::string& n) { return u->params[u->pindex.at(n)]; }

// packs one fused conv's weights into [kstep][cout_pad][128 B] with the 16-byte slots XOR-swizzled by (cout & 7)
static int pack_conv(td_unet* u, ConvWeights& cw) {
    const int chunk = u->chunk, per16 = chunk / 8;
    cw.cout_pad = (cw.cout + 63) / 64 * 64;
    int ksteps = 0;
    for (auto& s : cw.segs) ksteps += (s.c_pad / chunk) * s.taps;
    cw.ksteps = ksteps;
    const size_t row_elems = (size_t)chunk;
    const size_t total = (size_t)ksteps * cw.cout_pad * row_elems;
    std::vector<float> stage(u->bf16 ? 0 : total, 0.f);
    std::vector<uint16_t> stage16(u->bf16 ? total : 0, 0);
    int kstep = 0;
    for (auto& s : cw.segs) {
        const int k = s.taps == 9 ? 3 : 1;
        for (int ch = 0; ch < s.c_pad / chunk; ++ch)
            for (int tap = 0; tap < s.taps; ++tap, ++kstep)
                for (int co = 0; co < cw.cout; ++co)
                    for (int q = 0; q < 8; ++q) {
                        const size_t dst = ((size_t)kstep * cw.cout_pad + co) * row_elems + (size_t)((q ^ TD_SWZ(co)) * per16);
                        for (int e = 0; e < per16; ++e) {
                            int ci = ch * chunk + q * per16 + e;
                            float v = 0.f;
                            if (ci < s.c_real) v = (*s.w)[(((size_t)co * s.cin_tot + s.cin_off + ci) * k * k) + tap] * s.mul;
                            if (u->bf16) stage16[dst + e] = u->dt == TD_DTYPE_F16 ? f2h(v) : f2bf(v); else stage[dst + e] = v;
                        }
                    }
    }
    cw.packed.reset(new DevBuf());
    // tail padding: the LDS-DMA kernel over-reads 32 rows per tile and always fetches two K-steps past the end
    HIP_TRY(cw.packed->alloc(total * u->esize() + 2 * (size_t)cw.cout_pad * 128 + 16384, true));
    HIP_TRY(hipMemcpy(cw.packed->p, u->bf16 ? (const void*)stage16.data() : (const void*)stage.data(), total * u->esize(), hipMemcpyHostToDevice));
    // small-batch flavour: a second copy in MFMA-fragment order (0.5 GB more for the 30m base model; 288 GB of HBM).  Every 3x3 segment must
    // precede every 1x1 segment (true for every fused op of the U-Net); otherwise that flavour is simply not offered for this op
    cw.sb_n3 = 0; cw.sb_g1 = 0;
    if (u->bf16) {
        bool seen1 = false;
        for (auto& s : cw.segs) {
            if (s.taps == 9) { if (seen1) { cw.sb_n3 = -1; break; } cw.sb_n3 += s.c_pad / chunk; }
            else { seen1 = true; cw.sb_g1 += s.c_pad / chunk; }
        }
    }
    cw.packed_bytes = total * u->esize();
    return TD_OK;
}

// Fragment-order copy of an op's weights for the small-batch flavour, on first use (the planner calls this when it puts the op on conv_sb): +0.5 GB
// for the 30m base model when every conv of a single-tile forward runs on that flavour, nothing for models that never leave the throughput flavour.
static int ensure_packed_sb(td_unet* u, ConvWeights& cw) {
    if (cw.packed_sb || cw.sb_n3 < 0) return TD_OK;
    // Built into a local buffer and published only when allocation, launch AND completion succeeded (round-5 advisor): a failed repack must not leave a
    // zero-filled copy that the next plan would silently use, and the copy is read by launches on EITHER sampler lane's stream (dual_stream: the second
    // lane builds its plan after the stream swap, finds the copy present and launches on stream2 with no dependency on the stream that made it) --
    // so this setup-time step waits for its own stream before the pointer becomes visible.  Once per op and model, never in the steady state.
    Buf b(new DevBuf());
    HIP_TRY(b->alloc(cw.packed_bytes + 16384, true));   // (alloc synchronises behind its zero fill)
    HIP_TRY(launch_sb_repack(cw.packed->p, b->p, cw.cout_pad, cw.sb_n3, cw.sb_g1, u->eng->stream));
    HIP_TRY(hipStreamSynchronize(u->eng->stream));
    cw.packed_sb = std::move(b);
    return TD_OK;
}

static int ensure_packed_s16(td_unet* u, ConvWeights& cw) {
    if (cw.packed_s16 || cw.sb_n3 < 0) return TD_OK;
    Buf b(new DevBuf());   // (published after completion only: see ensure_packed_sb)
    HIP_TRY(b->alloc(cw.packed_bytes + 16384, true));
    HIP_TRY(launch_s16_repack(cw.packed->p, b->p, cw.cout_pad, cw.sb_n3, cw.sb_g1, u->eng->stream));
    HIP_TRY(hipStreamSynchronize(u->eng->stream));
    cw.packed_s16 = std::move(b);
    return TD_OK;
}

// a host table as a device buffer of its own (setup time: blocking)
template <typename T> static int upload_new(Buf& b, const std::vector<T>& v) {
    b.reset(new DevBuf());
    HIP_TRY(b->alloc(v.size() * sizeof(T), false));
    HIP_TRY(hipMemcpy(b->p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return TD_OK;
}

static int finalize(td_unet* u) {
    for (auto& p : u->params) if (!p.set) return fail(TD_ERR_STATE, "parameter not set: " + p.name);
    auto folded = [&](const std::string& n, float gain) -> const std::vector<float>* {
        auto& v = u->folded[n];
        if (v.empty()) fold(P(u, n), gain, v, u->prefolded);
        return &v;
    };
    int rc;
    if (u->kind != 0) {   // no embedding: one row of ones serves every block and every image (+ slack for the epilogues' 16-byte row reads)
        std::vector<float> ones((size_t)u->g.max_cout + 256, 1.f);
        if ((rc = upload_new(u->d_ones, ones))) return rc;
    }
    // embedding path (fp32 on device)
    if (u->kind == 0) {
        if ((rc = upload_new(u->d_freqs, P(u, "noise_fourier.freqs").data))) return rc;
        if ((rc = upload_new(u->d_wnoise, *folded("noise_linear.weight", 1.f)))) return rc;
        {
            std::vector<float> wc, fr;
            EmbDesc& d = u->embd;
            memset(&d, 0, sizeof d);
            d.n = u->cfg.n_cond;
            double wsq = 1.0;
            for (int i = 0; i < d.n; ++i) {
                const std::string pre = "conditional_layers." + std::to_string(i);
                d.type[i] = u->cfg.cond_type[i]; d.dims[i] = u->cfg.cond_dims[i]; d.weight[i] = u->cfg.cond_weights[i];
                d.xoff[i] = d.row_len; d.row_len += d.type[i] == 0 ? d.dims[i] : 1;
                d.foff[i] = d.feat_total; d.feat_total += d.dims[i];
                d.woff[i] = (int)wc.size();
                const std::vector<float>* w = folded(pre + (d.type[i] == 0 ? ".weight" : ".1.weight"), 1.f);
                wc.insert(wc.end(), w->begin(), w->end());
                if (d.type[i] == 1) {
                    d.froff[i] = (int)fr.size();
                    const auto& f = P(u, pre + ".0.freqs").data; const auto& ph = P(u, pre + ".0.phases").data;
                    fr.insert(fr.end(), f.begin(), f.end()); fr.insert(fr.end(), ph.begin(), ph.end());
                }
                wsq += (double)d.weight[i] * d.weight[i];
            }
            d.inv_norm = (float)(1.0 / sqrt(wsq));
            u->cond_row_len = d.row_len;
            if (wc.empty()) wc.push_back(0.f);
            if (fr.empty()) fr.push_back(0.f);
            if ((rc = upload_new(u->d_wcond, wc)) || (rc = upload_new(u->d_fourier, fr))) return rc;
        }
        std::vector<float> wall;
        std::vector<int> woff, coff, cout;
        auto add = [&](const GraphBlock& b) {
            if (b.is_conv) return;
            const std::vector<float>* w = folded(b.name + ".emb_linear.weight", P(u, b.name + ".emb_gain").data[0]);
            woff.push_back((int)wall.size()); coff.push_back(b.cvec_off); cout.push_back(b.cout);
            wall.insert(wall.end(), w->begin(), w->end());
        };
        for (auto& b : u->g.enc) add(b);
        for (auto& b : u->g.dec) add(b);
        u->n_blocks = (int)woff.size();
        if ((rc = upload_new(u->d_wemb, wall))) return rc;
        if ((rc = upload_new(u->d_blk_woff, woff)) || (rc = upload_new(u->d_blk_coff, coff)) || (rc = upload_new(u->d_blk_cout, cout))) return rc;
    }
    // conv weights per fused op: the weight side of the graph's K-segments
    u->convw.clear();
    u->convw.resize(u->g.ops.size());
    for (size_t i = 0; i < u->g.ops.size(); ++i) {
        const GraphOp& gop = u->g.ops[i];
        if (gop.attn) continue;
        ConvWeights& cw = u->convw[i];
        cw.cout = gop.cout;
        for (const GraphSeg& gs : gop.segs) {
            WSeg s;
            static_cast<GraphSeg&>(s) = gs;
            s.w = folded(gs.wname, gs.gain.empty() ? 1.f : P(u, gs.gain).data[0]);
            cw.segs.push_back(s);
        }
        if ((rc = pack_conv(u, cw))) return rc;
    }
    for (auto& p : u->params) { p.data.clear(); p.data.shrink_to_fit(); }
    u->folded.clear();
    HIP_TRY(hipDeviceSynchronize());
    u->finalized = true;
    return TD_OK;
}

// ------------------------------------------------------------------------------------------------ plan
static int new_buf(Plan& pl, size_t bytes, void** out) {
    Buf b(new DevBuf());
    HIP_TRY(b->alloc(bytes, true));
    *out = b->p;
    pl.bytes += b->bytes;
    pl.bufs.push_back(std::move(b));
    return TD_OK;
}

// The plan options (conv_select.h: PlanOptions) with the defaults that ship.  These are the ONLY read sites of plan options: the plan builder and the
// conv selector work on the struct, and build_plan makes the plan-cache key from its members.
static PlanOptions read_plan_options(const td_engine* e) {
    PlanOptions o;
    o.batch_invariant = e->option("batch_invariant", 0);
    o.attn_mfma = e->option("attn_mfma", 1);
    o.bn128_min_wgs = e->option("bn128_min_wgs", 128);
    o.glds = e->option("glds", 1);
    o.glds_bn = e->option("glds_bn", 0);
    o.glds_bn64 = e->option("glds_bn64", 1);
    o.glds_dma1x1 = e->option("glds_dma1x1", 1);
    o.glds_min_wgs = e->option("glds_min_wgs", 8);
    o.glds_round_aware = e->option("glds_round_aware", 1);
    o.glds_small_max_groups = e->option("glds_small_max_groups", 6);
    o.glds_splitk = e->option("glds_splitk", 1);
    o.glds_splitk_from_groups = e->option("glds_splitk_from_groups", 2);
    o.glds_splitk_max = e->option("glds_splitk_max", 32);
    o.glds_splitk_min_groups = e->option("glds_splitk_min_groups", 1);
    o.glds_tiny = e->option("glds_tiny", 0);
    o.glds_variant = e->option("glds_variant", -1);
    o.glds_wide = e->option("glds_wide", 1);
    o.glds_wide_min_wgs = e->option("glds_wide_min_wgs", 384);
    o.glds_wide_tail = e->option("glds_wide_tail", 1);
    o.glds_wide_persist = e->option("glds_wide_persist", 0);
    o.glds_wide_mfma16 = e->option("glds_wide_mfma16", 1);
    o.fewcout = e->option("fewcout", 1);
    o.producer_act = e->option("producer_act", 1);
    o.s16 = e->option("s16", 1);
    o.s16_min_wgs = e->option("s16_min_wgs", 128);
    o.sb = e->option("sb", 1);
    o.sb_m4 = e->option("sb_m4", 0);
    o.sb_max_glds_wgs = e->option("sb_max_glds_wgs", 1 << 30);
    o.sb_mt = e->option("sb_mt", 0);
    o.sb_nt = e->option("sb_nt", 0);
    o.sb_order = e->option("sb_order", -1);
    o.sb_splitk = e->option("sb_splitk", 1);
    o.sb_splitk_max = e->option("sb_splitk_max", 16);
    o.sb_splitk_wgs = e->option("sb_splitk_wgs", 224);
    o.sb_target_wgs = e->option("sb_target_wgs", 160);
    o.splitk = e->option("splitk", 1);
    o.splitk_target_wgs = e->option("splitk_target_wgs", 512);
    o.splitk_weighted = e->option("splitk_weighted", 1);
    o.walk_alternate = e->option("walk_alternate", 1);
    return o;
}

static int build_plan(td_unet* u, int N, int H, int W, Plan** out, int lane = 0) {
    // every plan option is part of the cache key, by its effective value (a plan built under other options must never be reused)
    PlanOptions po = read_plan_options(u->eng);
    std::string key = std::to_string(N) + "_" + std::to_string(H) + "_" + std::to_string(W);
    po.for_each([&](const char*, int64_t v) { key += "_" + std::to_string((long long)v); });
    if (lane) key += "_lane" + std::to_string(lane);   // a second, independent activation set of the same shape (concurrent half-batches)
    auto it = u->plans.find(key);
    if (it != u->plans.end()) { it->second->last_use = ++u->use_clock; *out = it->second.get(); return TD_OK; }
    if (N < 1 || N > 1023 || H > 1023 || W > 1023) return fail(TD_ERR_ARG, "batch/size out of range");
    const int down = 1 << (u->cfg.n_levels - 1);
    if (u->kind != 2 && (H % down || W % down)) return fail(TD_ERR_ARG, "H and W must be divisible by 2^(levels-1)");
    if (u->kind == 2 && (H * down > 1023 || W * down > 1023)) return fail(TD_ERR_ARG, "batch/size out of range");   // (the decoder's input is the latent: its maps grow)
    // plan cache: least-recently-used plans are dropped once the cached plans exceed the byte budget (each owns a full activation set;
    // InfiniteTensor batches vary in size, so an unbounded cache would pin one activation set per batch size ever seen)
    {
        const size_t budget = (size_t)u->eng->option("plan_cache_mb", 65536) << 20;
        const size_t max_plans = (size_t)u->eng->option("plan_cache_max", 12);
        size_t total = 0;
        for (auto& kv : u->plans) total += kv.second->bytes;
        while (!u->plans.empty() && (total > budget || u->plans.size() >= max_plans)) {
            auto victim = u->plans.begin();
            for (auto jt = u->plans.begin(); jt != u->plans.end(); ++jt) if (jt->second->last_use < victim->second->last_use) victim = jt;
            HIP_TRY(hipStreamSynchronize(u->eng->stream));
            total -= victim->second->bytes;
            u->plans.erase(victim);
        }
    }
    std::unique_ptr<Plan> plp(new Plan());
    Plan& pl = *plp;
    pl.N = N; pl.H = H; pl.W = W;
    const size_t es = u->esize();
    const int chunk = u->chunk;
    int rc;
    size_t partial_bytes = 0;
    std::vector<Tensor> T(u->g.tensors.size());   // the graph's tensors at this shape
    auto dim = [](int v, int level) { for (; level > 0; --level) v = (v + 1) / 2; for (; level < 0; ++level) v *= 2; return v; };   // map size at a level

    auto new_tensor = [&](int C, int h, int w, bool want_sumsq, int nparts, Tensor* t) -> int {
        t->C = C; t->cstride = C; t->H = h; t->W = w; t->sumsq = nullptr; t->nparts = 0;
        if ((rc = new_buf(pl, (size_t)N * h * w * C * es, &t->ptr))) return rc;
        if (want_sumsq) {
            void* s;
            if ((rc = new_buf(pl, (size_t)nparts * N * h * w * 4, &s))) return rc;
            t->sumsq = (float*)s; t->nparts = nparts;
        }
        return TD_OK;
    };

    // emits one fused conv op of the graph: wires the activation side of its segments, lets conv_select choose kernel / tile / split-K, allocates its output
    auto conv = [&](const GraphOp& g, ConvWeights& cw) -> int {
        const std::string& label = g.label;
        const int h = dim(H, g.level), w = dim(W, g.level);
        const Tensor* res = g.res >= 0 ? &T[g.res] : nullptr;
        Tensor* outT = &T[g.out];
        Op op;
        op.label = label;
        ConvParams& p = op.p;
        memset(&p, 0, sizeof p);
        p.nseg = (int)g.segs.size();
        int kgroups = 0;
        for (int i = 0; i < p.nseg; ++i) {
            const GraphSeg& s = g.segs[i];
            const Tensor* st = &T[s.src];
            ConvSeg& d = p.seg[i];
            d.src = st->ptr; d.C = s.c_pad; d.cstride = st->cstride; d.Hs = st->H; d.Ws = st->W;
            // the kernels address activations with 32-bit element offsets (pixel * channel stride): refuse instead of wrapping around
            if ((size_t)N * d.Hs * d.Ws * (size_t)d.cstride >= ((size_t)1 << 31))
                return fail(TD_ERR_ARG, "batch too large for 32-bit activation addressing (N*H*W*C >= 2^31 elements in " + label + "): split the batch");
            d.taps = s.taps; d.resample = s.resample; d.xform = s.xform; d.scale = s.scale;
            if (s.xform == 2) {
                if (!st->sumsq) return fail(TD_ERR_STATE, "pixel-norm source without sumsq: " + label);
                d.sumsq = st->sumsq; d.nparts = st->nparts; d.inv_c = 1.f / (float)st->C;
            }
            kgroups += d.C / chunk;
            op.k_alg += (double)s.c_real * s.taps;   // e.g. 6 of the input conv's 64 padded channels
        }
        p.wpack = cw.packed->p;
        p.N = N; p.H = h; p.W = w; p.Cout = cw.cout; p.CoutPad = cw.cout_pad; p.kgroups = kgroups;
        // kernel, tile and split: conv_select.h decides from the shape, the weights' geometry and the plan options
        ConvSelIn in;
        in.N = N; in.h = h; in.w = w; in.cout = cw.cout; in.cout_pad = cw.cout_pad; in.kgroups = kgroups; in.nseg = p.nseg;
        for (int i = 0; i < p.nseg; ++i) in.seg[i] = {p.seg[i].C, p.seg[i].taps, p.seg[i].xform, p.seg[i].resample, p.seg[i].Hs, p.seg[i].Ws};
        in.chunk = chunk; in.dt = u->dt; in.bf16 = u->bf16; in.sb_n3 = cw.sb_n3; in.out_f32 = g.out_f32; in.epi = g.epi; in.has_res = res != nullptr; in.clip_pos = g.clip > 0.f;
        in.n_cus = u->eng->n_cus; in.op_index = (int)pl.ops.size();
        const ConvSel& sel = op.sel = conv_select(in, po);
        p.tiles_x = sel.tiles_x; p.tiles_y = sel.tiles_y; p.img_groups = sel.img_groups; p.n_ntiles = sel.n_ntiles; p.ksplit = sel.ksplit;
        p.persist = sel.persist; p.sb_order = sel.sb_order; p.reverse = sel.reverse; p.dma1x1 = sel.dma1x1;
        if (sel.wcopy == ConvWeightCopy::Sb) { if ((rc = ensure_packed_sb(u, cw))) return rc; p.wpack_sb = cw.packed_sb->p; p.sb_n3 = cw.sb_n3; }
        if (sel.wcopy == ConvWeightCopy::S16) { if ((rc = ensure_packed_s16(u, cw))) return rc; p.wpack_sb = cw.packed_s16->p; p.sb_n3 = cw.sb_n3; }
        if (!conv_set_kbounds(p, po.splitk_weighted != 0, chunk)) return fail(TD_ERR_UNSUPPORTED, "split-K bounds: " + label);
        p.epi = g.epi; p.out_f32 = g.out_f32 ? 1 : 0; p.clip = g.clip; p.zeros = u->eng->zeros;
        if (g.out_f32) {
            outT->C = cw.cout; outT->cstride = 8; outT->H = h; outT->W = w; outT->sumsq = nullptr;
            if ((rc = new_buf(pl, (size_t)N * h * w * 8 * 4, &outT->ptr))) return rc;
        } else if ((rc = new_tensor(cw.cout, h, w, g.want_sumsq, sel.out_parts, outT))) return rc;
        p.out = outT->ptr; p.out_cstride = outT->cstride; p.out_sumsq = outT->sumsq;
        if ((size_t)N * h * w * (size_t)std::max(outT->cstride, cw.cout_pad) >= ((size_t)1 << 31))
            return fail(TD_ERR_ARG, "batch too large for 32-bit activation addressing (output of " + label + "): split the batch");
        op.cvec_off = g.cvec_off; p.cvec_stride = u->g.c_total;
        if (res) {
            p.res = res->ptr; p.res_cstride = res->cstride; p.res_Hs = res->H; p.res_Ws = res->W; p.res_resample = g.res_resample;
            p.res_scale = kMixRes;
            if (g.res_norm) {
                if (!res->sumsq) return fail(TD_ERR_STATE, "normed residual without sumsq: " + label);
                p.res_sumsq = res->sumsq; p.res_nparts = res->nparts; p.res_inv_c = 1.f / (float)res->C;
            }
        }
        if (p.ksplit > 1) partial_bytes = std::max(partial_bytes, (size_t)p.ksplit * N * h * w * cw.cout_pad * 4);
        op.out_C = cw.cout; op.out_H = h; op.out_W = w;
        pl.ops.push_back(op);
        return TD_OK;
    };

    // bf16 mode: attention blocks run on the MFMA kernel (attn_mfma.hip); its packed operands live in a per-op workspace.  Everything else -- fp16, fp32, and bf16
    // with option attn_mfma = 0 -- runs the scalar attn_kernel (small_kernels.hip), whose LDS tiles hold 64 tokens: more is refused here, before anything is launched
    const bool attn_on_mfma = u->dt == TD_DTYPE_BF16 && po.attn_mfma != 0;
    auto attn_fits = [&](int tokens, const std::string& name) -> int {
        // (the autoencoder graphs run such a block on the one-wave-per-query kernel of ae_kernels.hip instead: run_unet)
        if (tokens > 65535) return fail(TD_ERR_UNSUPPORTED, "attention over more than 65535 tokens: " + name);
        if (tokens > 64 && !attn_on_mfma && u->kind == 0)
            return fail(TD_ERR_UNSUPPORTED, "attention over more than 64 tokens needs bf16 mode with option attn_mfma = 1 (MFMA kernel; the scalar kernel holds 64): " + name);
        return TD_OK;
    };
    auto attn_workspace = [&](Op& a) -> int {
        if (!attn_on_mfma) return TD_OK;
        size_t qn, kn, vn;
        const size_t tot = attn_workspace_elems(N, a.C / 64, a.tokens, a.tokens, 64, &qn, &kn, &vn);
        void* ws;
        int r = new_buf(pl, tot * 2, &ws);
        if (r) return r;
        a.attn_ws = ws;
        return TD_OK;
    };

    // input tensor (ones channel appended, zero padded to one K chunk)
    Tensor& xin = T[0];
    xin.C = chunk; xin.cstride = chunk; xin.H = H; xin.W = W;
    if ((rc = new_buf(pl, (size_t)N * H * W * chunk * es, &xin.ptr))) return rc;
    pl.xin = xin.ptr;

    for (size_t i = 0; i < u->g.ops.size(); ++i) {
        const GraphOp& g = u->g.ops[i];
        const int h = dim(H, g.level), w = dim(W, g.level);
        if (!g.attn) {
            if (i + 1 < u->g.ops.size() && u->g.ops[i + 1].attn && (rc = attn_fits(h * w, u->g.ops[i + 1].block))) return rc;   // before its qkv conv allocates
            if ((rc = conv(g, u->convw[i]))) return rc;
            continue;
        }
        if ((rc = new_tensor(g.cout, h, w, false, 0, &T[g.out]))) return rc;
        Op a; a.kind = Op::ATTN; a.qkv = T[g.qkv].ptr; a.att = T[g.out].ptr; a.tokens = h * w; a.C = g.cout; a.label = g.label; a.out_C = g.cout; a.out_H = h; a.out_W = w;
        if ((rc = attn_workspace(a))) return rc;
        pl.ops.push_back(a);
    }
    pl.F = (float*)T[u->g.ops.back().out].ptr;
    // Producer-side activation: a segment that takes mp_silu(scale * x) of a whole conv output (decoder blocks: the running tensor
    // and the skip tensor of the concatenation) reads a second copy that the PRODUCER's epilogue writes already activated, instead of
    // applying exp/rcp to every 16-byte piece of every halo patch in every cout-tile workgroup of the consumer.  One copy per
    // producer (the first such consumer's scale); computed from the rounded output, so results are bit-identical to the in-kernel form.
    if (po.producer_act) {
        std::unordered_map<const void*, size_t> producer;
        for (size_t k = 0; k < pl.ops.size(); ++k)
            if (pl.ops[k].kind == Op::CONV && !pl.ops[k].p.out_f32) producer[pl.ops[k].p.out] = k;
        for (size_t j = 0; j < pl.ops.size(); ++j) {
            if (pl.ops[j].kind != Op::CONV) continue;
            ConvParams& c = pl.ops[j].p;
            for (int i = 0; i < c.nseg; ++i) {
                if (c.seg[i].xform != 1) continue;
                auto it = producer.find(c.seg[i].src);
                if (it == producer.end() || it->second >= j) continue;
                ConvParams& q = pl.ops[it->second].p;
                if (q.out2 && q.out2_scale != c.seg[i].scale) continue;
                if (!q.out2) {
                    void* b2;
                    if ((rc = new_buf(pl, (size_t)q.N * q.H * q.W * q.out_cstride * es, &b2))) return rc;
                    q.out2 = b2; q.out2_scale = c.seg[i].scale;
                }
                c.seg[i].src = q.out2; c.seg[i].xform = 0; c.seg[i].scale = 1.f;
            }
        }
    }
    if (partial_bytes) {
        void* pp;
        if ((rc = new_buf(pl, partial_bytes, &pp))) return rc;
        pl.partial = (float*)pp;
        for (auto& op : pl.ops) if (op.kind == Op::CONV) op.p.partial = pl.partial;
    }
    const size_t xbytes = u->kind != 0 ? 16 : (size_t)N * std::max(u->cfg.in_channels, u->cfg.out_channels) * H * W * 4;   // (no sampler runs on the autoencoder's stacks)
    pl.x.reset(new DevBuf()); pl.m1.reset(new DevBuf()); pl.m2.reset(new DevBuf()); pl.xt.reset(new DevBuf()); pl.cond.reset(new DevBuf());
    HIP_TRY(pl.x->alloc(xbytes)); HIP_TRY(pl.m1->alloc(xbytes)); HIP_TRY(pl.m2->alloc(xbytes)); HIP_TRY(pl.xt->alloc(xbytes));
    HIP_TRY(pl.cond->alloc((size_t)N * std::max(1, u->cond_row_len) * 4));
    HIP_TRY(hipDeviceSynchronize());  // buffer memsets ran on the null stream; the engine stream is non-blocking
    pl.bytes += 4 * xbytes + (size_t)N * std::max(1, u->cond_row_len) * 4;   // x, m1, m2, xt (+ cond): what the plan-cache budget has to see
    pl.last_use = ++u->use_clock;
    *out = plp.get();
    u->plans[key] = std::move(plp);
    return TD_OK;
}

// per-(step,tile) embeddings and per-block modulation vectors for all steps at once (t depends on the step only)
static int compute_cvecs(td_unet* u, Plan& pl, const std::vector<float>& t_steps, const float* d_cond, Call& c) {
    hipStream_t st = u->eng->stream;
    const int rows = (int)t_steps.size() * pl.N;
    if (!pl.emb || pl.cvec_rows < rows) {
        // a captured EDM graph holds raw pointers into cvec (run_unet's cbase): it dies with the buffers it points into
        pl.drop_graph();
        HIP_TRY(hipStreamSynchronize(st));
        pl.emb.reset(new DevBuf()); pl.cvec.reset(new DevBuf()); pl.tsteps.reset(new DevBuf());
        HIP_TRY(pl.emb->alloc((size_t)rows * u->g.emb_ch * 4));
        HIP_TRY(pl.cvec->alloc((size_t)rows * u->g.c_total * 4));
        HIP_TRY(pl.tsteps->alloc(std::max<size_t>(64, t_steps.size()) * 4));
        pl.cvec_rows = rows;
    }
    // `t_steps` lives on the caller's stack: with option "async" the call may return before the stream gets here, so the (80-byte) upload goes
    // through the engine's pinned ring
    { int rc_ = c.up(pl.tsteps->p, t_steps.data(), t_steps.size() * 4); if (rc_) return rc_; }
    const int half = u->g.noise_dims / 2;
    hipLaunchKernelGGL(emb_kernel, dim3(rows, (u->g.emb_ch + 63) / 64), dim3(256), (size_t)(2 * half + u->embd.feat_total) * 4, st, (const float*)pl.tsteps->p, d_cond, pl.N,
                       (const float*)u->d_freqs->p, half, (const float*)u->d_wnoise->p, (const float*)u->d_wcond->p, (const float*)u->d_fourier->p,
                       u->embd, u->g.emb_ch, (float*)pl.emb->p);
    const int max_cout = u->g.max_cout;
    const bool c16 = u->g.emb_ch % 16 == 0 && u->g.c_total % 4 == 0 && u->g.cout16;   // the matrix-core form needs 16-byte operand pieces and whole 16-cout slices
    if (c16 && u->g.emb_ch % 64 == 0)
        hipLaunchKernelGGL(cvec_mfma_kernel<4>, dim3((max_cout + 63) / 64, (rows + 63) / 64, u->n_blocks), dim3(256), 0, st, (const float*)pl.emb->p, rows,
                           u->g.emb_ch, (const float*)u->d_wemb->p, (const int*)u->d_blk_woff->p, (const int*)u->d_blk_coff->p, (const int*)u->d_blk_cout->p,
                           u->g.c_total, (float*)pl.cvec->p);
    else if (c16)
        hipLaunchKernelGGL(cvec_mfma_kernel<1>, dim3((max_cout + 63) / 64, (rows + 63) / 64, u->n_blocks), dim3(256), 0, st, (const float*)pl.emb->p, rows,
                           u->g.emb_ch, (const float*)u->d_wemb->p, (const int*)u->d_blk_woff->p, (const int*)u->d_blk_coff->p, (const int*)u->d_blk_cout->p,
                           u->g.c_total, (float*)pl.cvec->p);
    else
    hipLaunchKernelGGL(cvec_kernel, dim3((max_cout + 63) / 64, (rows + 15) / 16, u->n_blocks), dim3(256), (size_t)16 * u->g.emb_ch * 4, st, (const float*)pl.emb->p, rows,
                       u->g.emb_ch, (const float*)u->d_wemb->p, (const int*)u->d_blk_woff->p, (const int*)u->d_blk_coff->p, (const int*)u->d_blk_cout->p,
                       u->g.c_total, (float*)pl.cvec->p);
    hipLaunchKernelGGL(cvec_norm_kernel, dim3(rows, u->n_blocks), dim3(256), 0, st, (float*)pl.cvec->p, (const int*)u->d_blk_coff->p,
                       (const int*)u->d_blk_cout->p, u->g.c_total);
    HIP_TRY(hipGetLastError());
    pl.cvec_written = rows;
    return TD_OK;
}

static hipError_t launch_selected(const ConvParams& p, const ConvSel& s, int dt, hipStream_t st) {
    switch (s.kernel) {
        case ConvKernel::PerTap: return launch_conv(p, dt, s.narrow, s.bn, 0, st);
        case ConvKernel::Glds: return launch_conv_glds(p, dt, s.narrow, s.bn, s.glds_variant, st);
        case ConvKernel::GldsWide: return launch_conv_glds_wide(p, dt, s.bn, st);
        case ConvKernel::GldsWide16: return launch_conv_glds_wide16(p, dt, st);
        case ConvKernel::Sb: return launch_conv_sb(p, dt, s.narrow, s.sb_mt, s.sb_nt, st);
        case ConvKernel::S16: return launch_conv_s16(p, dt, s.narrow, st);
        case ConvKernel::FewCout: return launch_conv_fewcout(p, dt, st);   // with the solver step fused too: the same sums as the plain launch, then epilogue4's step
    }
    return hipErrorInvalidValue;
}

// Option "profile": a HIP event pair around each launch of one call (eager mode).  The destructor waits for the stream once -- a profiled call is
// not enqueue-only -- and accumulates per label (td_engine_profile_dump) and into the conv / other / LDS-DMA-family totals of the engine.
struct ProfScope {
    td_engine* const e;
    const hipStream_t st;
    const bool on;
    struct Rec { hipEvent_t a, b; std::string label; bool conv; double flop; };
    std::vector<Rec> recs;
    hipEvent_t open = nullptr;
    explicit ProfScope(td_engine* e_) : e(e_), st(e_->stream), on(e_->option("profile", 0) != 0) {}
    void begin() {
        if (!on || hipEventCreate(&open) != hipSuccess) { open = nullptr; return; }
        (void)hipEventRecord(open, st);
    }
    // `conv`: counted with the conv launches, else with the others; `flop`: the launch's roofline FLOP (0: not part of the LDS-DMA family's total)
    void end(const std::string& label, bool conv = false, double flop = 0.0) {
        hipEvent_t b;
        if (!open || hipEventCreate(&b) != hipSuccess) return;
        (void)hipEventRecord(b, st);
        recs.push_back({open, b, label, conv, flop});
        open = nullptr;
    }
    ~ProfScope() {
        if (open) (void)hipEventDestroy(open);
        if (recs.empty()) return;
        (void)hipStreamSynchronize(st);
        for (const Rec& r : recs) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, r.a, r.b);
            auto& po = e->prof_ops[r.label]; po.first += ms; po.second++;
            if (r.flop > 0) { e->prof_glds_ms += ms; e->prof_glds_flop += r.flop; e->prof_glds_launches++; }
            if (r.conv) { e->prof_conv_ms += ms; e->prof_conv_launches++; } else { e->prof_other_ms += ms; e->prof_other_launches++; }
            (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
        }
    }
};

// profile label of one conv launch: the op's label, its geometry, the selector's tag (x16: conv_glds_wide16.hip; the flavour tag stays f2w) and the
// algorithmic work of the launch
static std::string conv_prof_label(const td_unet* u, const Op& op, const ConvParams& p) {
    // GFLOP: REAL input channels (the 6-channel input conv is 5.4 GFLOP at batch 64, not the 58 its K padding to 64 would give)
    const double gf = op.k_alg * 2.0 * p.N * p.H * p.W * p.Cout * 1e-9;
    // HBM megabytes: every source tensor once (at ITS resolution), the residual once, the outputs once, the weights once
    double mb = 0.0;
    const double es = (double)u->esize();
    for (int si = 0; si < p.nseg; ++si) mb += (double)p.N * p.seg[si].Hs * p.seg[si].Ws * p.seg[si].C * es + (double)p.seg[si].C / 64.0 * p.seg[si].taps * p.CoutPad * 128.0 * (es / 2.0);
    if (p.res) mb += (double)p.N * p.res_Hs * p.res_Ws * p.Cout * es;
    const double o1 = (double)p.N * p.H * p.W * p.Cout * (p.out_f32 ? 4.0 : es);
    const double mbs = (mb + o1) * 1e-6;   // strict: without the optional pre-activated second output (an optimisation, not part of the layer's definition)
    mb += o1 * (p.out2 ? 2.0 : 1.0);
    mb *= 1e-6;
    char head[48], nums[112];
    snprintf(head, sizeof head, " [%dx%d k%d ", p.H, p.W, p.kgroups);
    snprintf(nums, sizeof nums, " wg%d ks%d gf%.2f mb%.2f mbs%.2f", p.n_ntiles * p.tiles_x * p.tiles_y * p.img_groups, p.ksplit, gf, mb, mbs);
    return op.label + head + conv_sel_tag(op.sel, nums) + "]";
}

// runs the conv stack: xin -> F, using modulation vectors of `step`
// `fuse` (EDM sampler): the output conv runs the DPM-Solver++ update of this step in its epilogue (EPI_DPM_STEP) instead of writing F
static int run_unet(td_unet* u, Plan& pl, int step, const SchedCoef* fuse = nullptr) {
    hipStream_t st = u->eng->stream;
    const float* cbase = u->kind != 0 ? (const float*)u->d_ones->p : (const float*)pl.cvec->p + (size_t)step * pl.N * u->g.c_total;
    ProfScope prof(u->eng);
    for (auto& op : pl.ops) {
        if (op.kind == Op::ATTN) {
            prof.begin();
            if (op.attn_ws) {   // bf16: pack (de-interleave + unit-RMS norm) -> MFMA flash kernel; unet_block.py:102-108
                const int Hh = op.C / 64, L = op.tokens;
                size_t qn, kn, vn;
                attn_workspace_elems(pl.N, Hh, L, L, 64, &qn, &kn, &vn);
                __bf16 *Qp = (__bf16*)op.attn_ws, *Kp = Qp + qn, *Vt = Kp + kn;
                const __bf16* qkv = (const __bf16*)op.qkv;
                const AttnStrides so = {(long)L * op.C, 64L, (long)op.C, 1L};   // (input: element (b, token, head, d, q|k|v) of the qkv conv's NHWC output)
                hipError_t ea = attn_pack_qkv64<__bf16>(qkv, 3L * op.C, pl.N, Hh, L, 0.125f, Qp, Kp, Vt, st);   // one launch for q, k and v (the generic attn_pack: td_attention)
                if (ea == hipSuccess) ea = attn_mfma(Qp, Kp, Vt, nullptr, (__bf16*)op.att, so, pl.N, Hh, L, L, 64, st);
                if (ea != hipSuccess) return fail(TD_ERR_HIP, std::string("attention launch: ") + hipGetErrorString(ea));
            } else if (op.tokens > 64)   // autoencoder graphs only (build_plan refuses it for the U-Net)
            TD_DISPATCH_T(u, hipLaunchKernelGGL(ae_attn_wave_kernel<T_>, dim3(pl.N, op.C / 64, (op.tokens + 3) / 4), dim3(256), 0, st, (const T_*)op.qkv, (T_*)op.att, op.tokens, op.C));
            else
            TD_DISPATCH_T(u, hipLaunchKernelGGL(attn_kernel<T_>, dim3(pl.N, op.C / 64), dim3(256), 0, st, (const T_*)op.qkv, (T_*)op.att, op.tokens, op.C));
            prof.end(op.label);
            HIP_TRY(hipGetLastError());
            continue;
        }
        ConvParams p = op.p;
        if (op.cvec_off >= 0) p.cvec = cbase + op.cvec_off;
        if (fuse && &op == &pl.ops.back()) {   // the output conv (EPI_PLAIN, fp32 F): results go straight into the solver state
            p.epi = EPI_DPM_STEP; p.dpm_x = (float*)pl.x->p; p.dpm_m1 = (float*)pl.m1->p; p.dpm_m2 = u->eng->option("solver_order", 2) == 3 ? (float*)pl.m2->p : nullptr; p.dpm_xin = pl.xin; p.dpm_xin_cstride = u->chunk; p.dpm_k = *fuse;
        }
        prof.begin();
        hipError_t e = launch_selected(p, op.sel, u->dt, st);
        // (roofline FLOP for the LDS-DMA family alone: bench.py's roofline kernel; small-batch launches are told apart by their f4 label)
        if (prof.on) prof.end(conv_prof_label(u, op, p), true, op.sel.glds_family() ? 2.0 * p.N * p.H * p.W * (double)p.Cout * op.k_alg : 0.0);
        if (e != hipSuccess) return fail(TD_ERR_HIP, "conv launch " + op.label + ": " + hipGetErrorString(e));
    }
    return TD_OK;
}

// debug read-back: NHWC with channel stride `cs`, fp32 (`f32`) or the model's 16-bit storage type, -> planar fp32 [n][C][HW] of its first C channels
static void widen_nhwc(const td_unet* u, bool f32, const uint8_t* raw, int n, int C, size_t HW, int cs, float* out) {
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < C; ++c)
            for (size_t p = 0; p < HW; ++p) {
                const size_t src = ((size_t)i * HW + p) * cs + c;
                float v;
                if (f32) v = ((const float*)raw)[src];
                else if (u->dt == TD_DTYPE_F16) { _Float16 h; memcpy(&h, (const uint16_t*)raw + src, 2); v = (float)h; }
                else { uint32_t b = (uint32_t)((const uint16_t*)raw)[src] << 16; memcpy(&v, &b, 4); }
                out[((size_t)i * C + c) * HW + p] = v;
            }
}

static inline dim3 grid1(size_t n, int b = 256) { return dim3((unsigned)((n + b - 1) / b)); }

// ================================================================================================ C ABI
extern "C" {

const char* td_last_error(void) { return g_err.c_str(); }
int td_version(void) { return 1; }
#ifndef TD_CSRC_SHA
#define TD_CSRC_SHA "unstamped"
#endif
const char* td_build_id(void) { return TD_CSRC_SHA; }

int td_engine_create(int device_id, td_engine** out) {
    if (!out) return fail(TD_ERR_ARG, "null out");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(TD_ERR_HIP, "no HIP device visible: the engine has no CPU fallback");
    if (device_id < 0 || device_id >= ndev) return fail(TD_ERR_ARG, "bad device id");
    DevGuard dg_(device_id);
    td_engine* e = new td_engine();
    e->device = device_id;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) e->n_cus = prop.multiProcessorCount; }
    hipError_t err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    e->own_stream = e->stream;
    if (err == hipSuccess) err = hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming);
    if (err == hipSuccess) err = hipMalloc(&e->zeros, 4096);
    if (err == hipSuccess) err = hipMemset(e->zeros, 0, 4096);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) { if (e->stream) (void)hipStreamDestroy(e->stream); if (e->stream2) (void)hipStreamDestroy(e->stream2); if (e->ev_fork) (void)hipEventDestroy(e->ev_fork); if (e->ev_join) (void)hipEventDestroy(e->ev_join); delete e; return fail(TD_ERR_HIP, hipGetErrorString(err)); }
    *out = e;
    return TD_OK;
}
void td_engine_destroy(td_engine* e) {
    if (!e) return;
    DevGuard dg_(e->device);
    // (the engine's OWN stream: e->stream may be the caller's -- td_engine_set_stream -- and is not ours to destroy)
    if (e->own_stream) { (void)hipStreamSynchronize(e->stream); (void)hipStreamDestroy(e->own_stream); }
    if (e->stream2) (void)hipStreamDestroy(e->stream2);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->zeros) (void)hipFree(e->zeros);
    delete e;
}
int td_engine_synchronize(td_engine* e) {
    DevGuard dg_(e->device); HIP_TRY(hipStreamSynchronize(e->stream)); e->deferred.clear(); e->ring.reset(); return TD_OK; }
void* td_engine_stream(td_engine* e) { return (void*)e->stream; }
int td_engine_set_stream(td_engine* e, void* hip_stream) {
    if (!e) return fail(TD_ERR_ARG, "null engine");
    DevGuard dg_(e->device);
    HIP_TRY(hipStreamSynchronize(e->stream));   // nothing of the old stream may be pending when the order of work changes hands
    e->deferred.clear();
    e->ring.reset();
    e->stream = hip_stream ? (hipStream_t)hip_stream : e->own_stream;
    return TD_OK;
}
// Every option the runtime reads.  td_engine_set_option refuses anything else: a misspelt key ("batch_invarient") used to be stored and never
// read -- silently losing, e.g., the bit-identity of sharded runs.
static const char* const kKnownOptions[] = {
    // behaviour
    "async", "batch_invariant", "fuse_solver", "graph", "lower_order_final", "profile", "solver_order", "dual_stream", "dual_stream_min_batch", "sampler_stop_after",
    "plan_cache_mb", "plan_cache_max", "grid_fused",
    // plan builder (speed only, or test hooks that force a tile shape; all part of the plan-cache key)
    "attn_mfma", "bn128_min_wgs", "glds", "glds_bn", "glds_bn64", "glds_dma1x1", "glds_min_wgs", "glds_round_aware", "glds_small_max_groups",
    "glds_splitk", "glds_splitk_from_groups", "glds_splitk_max", "glds_splitk_min_groups", "glds_tiny", "glds_variant", "glds_wide", "glds_wide_min_wgs", "glds_wide_tail", "glds_wide_persist", "glds_wide_mfma16", "fewcout",
    "producer_act", "s16", "s16_min_wgs", "sb", "sb_m4", "sb_max_glds_wgs", "sb_mt", "sb_nt", "sb_order", "sb_splitk", "sb_splitk_max", "sb_splitk_wgs", "sb_target_wgs", "splitk",
    "splitk_target_wgs", "splitk_weighted", "walk_alternate"};
int td_engine_set_option(td_engine* e, const char* key, int64_t value) {
    if (!e || !key) return fail(TD_ERR_ARG, "null");
    bool known = false;
    for (const char* k : kKnownOptions) known = known || strcmp(k, key) == 0;
    if (!known) return fail(TD_ERR_ARG, std::string("unknown engine option \"") + key + "\" (include/td_engine.h lists the options)");
    e->opt[key] = value;
    return TD_OK;
}

int64_t td_engine_get_option(td_engine* e, const char* key, int64_t dflt) { return (e && key) ? e->option(key, dflt) : dflt; }

int td_engine_profile_read(td_engine* e, double* conv_ms, int64_t* conv_launches, double* other_ms, int64_t* other_launches, int reset) {
    if (conv_ms) *conv_ms = e->prof_conv_ms;
    if (conv_launches) *conv_launches = e->prof_conv_launches;
    if (other_ms) *other_ms = e->prof_other_ms;
    if (other_launches) *other_launches = e->prof_other_launches;
    if (reset) { e->prof_conv_ms = e->prof_other_ms = 0.0; e->prof_conv_launches = e->prof_other_launches = 0; e->prof_ops.clear(); }
    return TD_OK;
}
int td_engine_profile_read_glds(td_engine* e, double* ms, double* flop, int64_t* launches, int reset) {
    if (ms) *ms = e->prof_glds_ms;
    if (flop) *flop = e->prof_glds_flop;
    if (launches) *launches = e->prof_glds_launches;
    if (reset) { e->prof_glds_ms = e->prof_glds_flop = 0.0; e->prof_glds_launches = 0; }
    return TD_OK;
}
int td_engine_profile_dump(td_engine* e, char* buf, int64_t capacity) {
    std::string out;
    for (auto& kv : e->prof_ops) {
        char line[256];
        snprintf(line, sizeof line, "%s\t%.4f\t%lld\n", kv.first.c_str(), kv.second.first, (long long)kv.second.second);
        out += line;
    }
    if ((int64_t)out.size() + 1 > capacity) return fail(TD_ERR_ARG, "capacity");
    memcpy(buf, out.c_str(), out.size() + 1);
    return TD_OK;
}

int td_unet_create(td_engine* e, const td_unet_config* cfg, int dtype, td_unet** out) {
    if (!e || !cfg || !out) return fail(TD_ERR_ARG, "null argument");
    if (dtype != TD_DTYPE_F32 && dtype != TD_DTYPE_BF16 && dtype != TD_DTYPE_F16) return fail(TD_ERR_ARG, "dtype");
    std::unique_ptr<td_unet> u(new td_unet());
    u->eng = e; u->cfg = *cfg; u->dt = dtype; u->bf16 = dtype != TD_DTYPE_F32; u->chunk = u->bf16 ? 64 : 32;
    int rc = init_graph(u.get(), nullptr);
    if (rc) return rc;
    *out = u.release();
    return TD_OK;
}
void td_unet_destroy(td_unet* u) {
    if (!u) return;
    DevGuard dg_(u->eng->device);
    (void)hipStreamSynchronize(u->eng->stream);
    delete u;
}
int td_unet_num_params(td_unet* u) { return (int)u->params.size(); }
int td_unet_param_info(td_unet* u, int i, const char** name, int32_t* ndim, int64_t shape[4]) {
    if (i < 0 || i >= (int)u->params.size()) return fail(TD_ERR_ARG, "index");
    *name = u->params[i].name.c_str(); *ndim = u->params[i].ndim;
    for (int k = 0; k < 4; ++k) shape[k] = u->params[i].shape[k];
    return TD_OK;
}
int td_unet_set_param(td_unet* u, const char* name, const float* host_data, int64_t numel) {
    if (u->finalized) return fail(TD_ERR_STATE, "already finalized");
    auto it = u->pindex.find(name);
    if (it == u->pindex.end()) return fail(TD_ERR_ARG, std::string("unknown parameter ") + name);
    Param& p = u->params[it->second];
    if (numel != p.numel()) return fail(TD_ERR_ARG, std::string("size mismatch for ") + name);
    p.data.assign(host_data, host_data + numel);
    p.set = true;
    return TD_OK;
}
int td_unet_set_prefolded(td_unet* u, int prefolded) {
    if (u->finalized) return fail(TD_ERR_STATE, "already finalized");
    u->prefolded = prefolded != 0;
    return TD_OK;
}
int td_unet_finalize(td_unet* u) {
    DevGuard dg_(u->eng->device);
    if (u->finalized) return TD_OK;
    return finalize(u);
}

int td_unet_cond_row_len(td_unet* u) { return u->cond_row_len; }

int td_unet_forward(td_unet* u, int n, int H, int W, const float* x, const float* t_host, const float* cond, float* out) {
    Call c(u->eng);
    if (!u->finalized) return fail(TD_ERR_STATE, "finalize first");
    Plan* pl;
    int rc = build_plan(u, n, H, W, &pl);
    if (rc) return rc;
    hipStream_t st = c.e->stream;
    const int C = u->cfg.in_channels, Co = u->cfg.out_channels, HW = H * W;
    const float *dx, *dcond = nullptr;
    float* dout;
    if ((rc = c.in(x, (size_t)n * C * HW * 4, &dx))) return rc;
    if (u->cond_row_len > 0 && (rc = c.in(cond, (size_t)n * u->cond_row_len * 4, &dcond))) return rc;
    if ((rc = c.out(out, (size_t)n * Co * HW * 4, &dout))) return rc;
    // per-sample t: treat every sample as its own "step" row set (rows = n steps x n tiles would be wasteful): run per distinct t
    // general case: one embedding row per sample -> emulate with steps=n, tiles=n and pick row i*n+i.  Keep it simple: loop unique t values.
    std::vector<float> ts(t_host, t_host + n);
    bool uniform = true;
    for (int i = 1; i < n; ++i) uniform = uniform && ts[i] == ts[0];
    if (uniform) {
        if ((rc = compute_cvecs(u, *pl, std::vector<float>(1, ts[0]), dcond, c))) return rc;
    } else {
        // rows = n "steps" x n tiles; sample i uses row i*n + i.  Build a compact [n][c_total] table by copying those rows to step 0's slot.
        if ((rc = compute_cvecs(u, *pl, ts, dcond, c))) return rc;
        for (int i = 1; i < n; ++i) {
            HIP_TRY(hipMemcpyAsync((float*)pl->cvec->p + (size_t)i * u->g.c_total, (float*)pl->cvec->p + ((size_t)i * n + i) * u->g.c_total, (size_t)u->g.c_total * 4,
                                   hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync((float*)pl->emb->p + (size_t)i * u->g.emb_ch, (float*)pl->emb->p + ((size_t)i * n + i) * u->g.emb_ch, (size_t)u->g.emb_ch * 4,
                                   hipMemcpyDeviceToDevice, st));
        }
    }
    TD_DISPATCH_T(u, hipLaunchKernelGGL(prep_input_kernel<T_>, grid1((size_t)n * HW), dim3(256), 0, st, dx, (T_*)pl->xin, n, C, HW, u->chunk, 1.f, C));
    if ((rc = run_unet(u, *pl, 0))) return rc;
    hipLaunchKernelGGL(unpack_output_kernel, grid1((size_t)n * HW), dim3(256), 0, st, (const float*)pl->F, dout, n, Co, HW, 8, 1.f);
    HIP_TRY(hipGetLastError());
    return c.finish(true);
}

int td_unet_read_activation(td_unet* u, int n, int H, int W, const char* label, float* out_host, int64_t capacity, int32_t dims[4]) {
    DevGuard dg_(u->eng->device);
    Plan* pl;
    int rc = build_plan(u, n, H, W, &pl);
    if (rc) return rc;
    if (!strcmp(label, "@emb") || !strcmp(label, "@cvec")) {
        const bool is_emb = !strcmp(label, "@emb");
        const int width = is_emb ? u->g.emb_ch : u->g.c_total;
        dims[0] = n; dims[1] = width; dims[2] = 1; dims[3] = 1;
        if ((int64_t)n * width > capacity) return fail(TD_ERR_ARG, "capacity");
        HIP_TRY(hipStreamSynchronize(u->eng->stream));
        HIP_TRY(hipMemcpy(out_host, is_emb ? pl->emb->p : pl->cvec->p, (size_t)n * width * 4, hipMemcpyDeviceToHost));
        return TD_OK;
    }
    if (!strcmp(label, "@emb:rows") || !strcmp(label, "@cvec:rows")) {
        // every (step, tile) row the last compute_cvecs on this plan wrote, not only the first n
        const bool is_emb = !strcmp(label, "@emb:rows");
        const int width = is_emb ? u->g.emb_ch : u->g.c_total, rows = pl->cvec_written;
        if (rows < 1 || !pl->emb) return fail(TD_ERR_STATE, "no embedding rows on this plan yet: run a forward or a sampler call first");
        dims[0] = rows; dims[1] = width; dims[2] = 1; dims[3] = 1;
        if ((int64_t)rows * width > capacity) return fail(TD_ERR_ARG, "capacity");
        HIP_TRY(hipStreamSynchronize(u->eng->stream));
        HIP_TRY(hipMemcpy(out_host, is_emb ? pl->emb->p : pl->cvec->p, (size_t)rows * width * 4, hipMemcpyDeviceToHost));
        return TD_OK;
    }
    if (!strcmp(label, "@x") || !strcmp(label, "@m1") || !strcmp(label, "@m2") || !strcmp(label, "@xt")) {
        // sampler state of this plan as the last call left it: planar fp32 [n][C_out][H][W]
        const int C = u->cfg.out_channels;
        const Buf& b = !strcmp(label, "@x") ? pl->x : !strcmp(label, "@m1") ? pl->m1 : !strcmp(label, "@m2") ? pl->m2 : pl->xt;
        dims[0] = n; dims[1] = C; dims[2] = H; dims[3] = W;
        if ((int64_t)n * C * H * W > capacity) return fail(TD_ERR_ARG, "capacity");
        HIP_TRY(hipStreamSynchronize(u->eng->stream));
        HIP_TRY(hipMemcpy(out_host, b->p, (size_t)n * C * H * W * 4, hipMemcpyDeviceToHost));
        return TD_OK;
    }
    if (!strcmp(label, "@xin")) {
        // the NHWC model input, every channel of the K chunk (sample, conditioning image, ones channel, padding), widened to fp32
        const int cs = u->chunk;
        const size_t HW = (size_t)H * W, elems = (size_t)n * HW * cs;
        dims[0] = n; dims[1] = cs; dims[2] = H; dims[3] = W;
        if ((int64_t)elems > capacity) return fail(TD_ERR_ARG, "capacity");
        HIP_TRY(hipStreamSynchronize(u->eng->stream));
        std::vector<uint8_t> raw(elems * (u->bf16 ? 2 : 4));
        HIP_TRY(hipMemcpy(raw.data(), pl->xin, raw.size(), hipMemcpyDeviceToHost));
        widen_nhwc(u, !u->bf16, raw.data(), n, cs, HW, cs, out_host);
        return TD_OK;
    }
    if (!strncmp(label, "sumsq:", 6)) {
        for (auto& op : pl->ops) {
            if (op.kind != Op::CONV || op.label != label + 6 || !op.p.out_sumsq) continue;
            // (an S16 op keeps sel.out_parts = CoutPad / 16 planes; this read-back has always returned the first CoutPad / 32 of them, which is what its callers expect)
            const int parts = op.sel.kernel == ConvKernel::S16 ? op.p.CoutPad / 32 : op.sel.out_parts;
            const size_t M = (size_t)n * op.out_H * op.out_W;
            dims[0] = parts; dims[1] = n; dims[2] = op.out_H; dims[3] = op.out_W;
            if ((int64_t)(parts * M) > capacity) return fail(TD_ERR_ARG, "capacity");
            HIP_TRY(hipStreamSynchronize(u->eng->stream));
            HIP_TRY(hipMemcpy(out_host, op.p.out_sumsq, parts * M * 4, hipMemcpyDeviceToHost));
            return TD_OK;
        }
        return fail(TD_ERR_ARG, "no sumsq for that op");
    }
    for (auto& op : pl->ops) {
        if (op.label != label) continue;
        // a conv op, or an attention op ("<block>.attn": its NHWC output, channel stride C, in the storage type)
        const bool is_attn = op.kind == Op::ATTN;
        const int C = op.out_C, h = op.out_H, w = op.out_W, cs = is_attn ? op.C : op.p.out_cstride;
        dims[0] = n; dims[1] = C; dims[2] = h; dims[3] = w;
        if ((int64_t)n * C * h * w > capacity) return fail(TD_ERR_ARG, "capacity");
        HIP_TRY(hipStreamSynchronize(u->eng->stream));
        const size_t elems = (size_t)n * h * w * cs;
        const bool f32out = (!is_attn && op.p.out_f32) || !u->bf16;
        std::vector<uint8_t> raw(elems * (f32out ? 4 : 2));
        HIP_TRY(hipMemcpy(raw.data(), is_attn ? op.att : op.p.out, raw.size(), hipMemcpyDeviceToHost));
        widen_nhwc(u, f32out, raw.data(), n, C, (size_t)h * w, cs, out_host);
        return TD_OK;
    }
    return fail(TD_ERR_ARG, std::string("no conv or attention op labelled ") + label);
}

// ---- schedule: the Karras sigma ladder is computed by the host scheduler with the reference's own fp32 torch ops (bit-exact,
// terrain_diffusion_amd/scheduler.py); the engine receives the sigmas and derives the per-step solver coefficients here.
static void dpm_coefs(const float* sig, int n_steps, float sigma_data, int solver_order, bool lower_order_final, std::vector<SchedCoef>& ks) {
    // fp32 scalar arithmetic in the reference's order (dpmsolver.py:245-258, 472-482, 515-540); order rule :688-715
    ks.resize(n_steps);
    int lower = 0;
    for (int i = 0; i < n_steps; ++i) {
        SchedCoef k;
        const float s = sig[i], st = sig[i + 1], sd = sigma_data;
        k.c_skip = (sd * sd) / (s * s + sd * sd);
        k.c_out = s * sd / sqrtf(s * s + sd * sd);
        const bool final = (i == n_steps - 1);
        const bool second = (i == n_steps - 2) && lower_order_final && n_steps < 15;   // lower_order_second (dpmsolver.py:694-696), engine option "lower_order_final"
        // dpmsolver.py:703-708 with config.solver_order and lower_order_final
        k.order = (solver_order < 2 || lower < 1 || final) ? 1 : ((solver_order == 2 || lower < 2 || second) ? 2 : 3);
        const float lam_t = 0.f - logf(st), lam_s = 0.f - logf(s);
        const float h = lam_t - lam_s;
        k.a = st / s;
        k.b0 = expf(-h) - 1.0f;
        k.inv_r0 = 0.f; k.inv_r1 = 0.f; k.f01 = 0.f; k.inv_r01 = 0.f; k.c1 = 0.f; k.c2 = 0.f;
        if (k.order >= 2) {
            const float lam_s1 = 0.f - logf(sig[i - 1]);
            const float h0 = lam_s - lam_s1;
            const float r0 = h0 / h;
            k.inv_r0 = 1.0f / r0;
            if (k.order == 3) {   // dpmsolver.py:586-613
                const float lam_s2 = 0.f - logf(sig[i - 2]);
                const float r1 = (lam_s1 - lam_s2) / h;
                k.inv_r1 = 1.0f / r1; k.f01 = r0 / (r0 + r1); k.inv_r01 = 1.0f / (r0 + r1);
                k.c1 = (expf(-h) - 1.0f) / h + 1.0f;
                k.c2 = (expf(-h) - 1.0f + h) / (h * h) - 0.5f;
            }
        }
        k.last = final ? 1 : 0;
        k.c_in_next = final ? 0.f : 1.f / sqrtf(st * st + sd * sd);
        if (lower < solver_order) ++lower;
        ks[i] = k;
    }
}

// The table above as the sampler uses it, for inspection: n_steps rows of 13 floats, the fields of SchedCoef in declaration order (order / last as floats).
int td_dpm_coefs(const float* sigmas_host, int n_steps, float sigma_data, int solver_order, int lower_order_final, float* out) {
    if (!sigmas_host || !out || n_steps < 1) return fail(TD_ERR_ARG, "td_dpm_coefs: null argument or n_steps < 1");
    if (solver_order < 1 || solver_order > 3) return fail(TD_ERR_ARG, "solver_order must be 1, 2 or 3");
    std::vector<SchedCoef> ks;
    dpm_coefs(sigmas_host, n_steps, sigma_data, solver_order, lower_order_final != 0, ks);
    for (int i = 0; i < n_steps; ++i) {
        const SchedCoef& k = ks[i];
        const float row[13] = {k.c_skip, k.c_out, k.a, k.b0, k.inv_r0, k.inv_r1, k.f01, k.inv_r01, k.c1, k.c2, k.c_in_next, (float)k.order, (float)k.last};
        memcpy(out + (size_t)i * 13, row, sizeof row);
    }
    return TD_OK;
}

// writes the conditioning-image channels [Cs, Cs+cimg) of the NHWC model input (constant over the solver steps)
static int stage_cond_img(td_unet* u, Plan& pl, int n, int HW, const float* cond_img, int cimg, int Cs, Call& c) {
    if (cimg == 0) { c.direct(cond_img); return TD_OK; }   // (not read, but a host pointer here has always made the call end synchronously)
    if (!cond_img) return fail(TD_ERR_ARG, "cond_img is null");
    const float* dimg;
    int rc = c.in(cond_img, (size_t)n * cimg * HW * 4, &dimg);
    if (rc) return rc;
    hipStream_t st = u->eng->stream;
    TD_DISPATCH_T(u, hipLaunchKernelGGL(write_cond_img_kernel<T_>, grid1((size_t)n * HW), dim3(256), 0, st, dimg, (T_*)pl.xin, n, cimg, HW, u->chunk, Cs));
    HIP_TRY(hipGetLastError());
    return TD_OK;
}

// One lane of the batched EDM sampler, on the arguments of td_sample_edm_ext (guide == NULL: guidance_scale is 1; score_scaling == 1 is off and reads
// nothing else): everything is enqueued on e->stream (the caller swaps the engine's streams for the second lane) and NOT waited for; temporaries
// that must outlive the queue go to the call scope.
static int sample_edm_lane(td_unet* u, const td_edm_ext& a, int lane, Call& c) {
    td_unet* const guide = a.guide;
    const int n = a.n, H = a.H, W = a.W, n_steps = a.n_steps, cimg = a.cimg_channels;
    const float gscale = a.guidance_scale, sigma_data = a.sigma_data, alpha = a.score_scaling;
    const float *sigmas_host = a.sigmas_host, *cond = a.cond, *cond_img = a.cond_img;
    float* const x = a.x;
    if (guide) {
        if (!guide->finalized) return fail(TD_ERR_STATE, "finalize the guide model first");
        if (guide->eng != u->eng || guide->dt != u->dt) return fail(TD_ERR_ARG, "guide model must live on the same engine and use the same dtype");
        if (guide->cfg.in_channels != u->cfg.in_channels || guide->cfg.out_channels != u->cfg.out_channels || guide->cond_row_len != u->cond_row_len)
            return fail(TD_ERR_ARG, "guide model must take the same inputs as the main model");
    }
    if (!u->finalized) return fail(TD_ERR_STATE, "finalize first");
    if (n_steps < 1) return fail(TD_ERR_ARG, "n_steps");
    if (alpha != 1.f && !a.score_cs_host) return fail(TD_ERR_ARG, "score_scaling != 1 needs score_cs_host (n_steps pairs cos t_i, sin t_i)");
    if (!std::isfinite(alpha)) return fail(TD_ERR_ARG, "score_scaling must be finite");
    const std::vector<float> cs = alpha != 1.f ? std::vector<float>(a.score_cs_host, a.score_cs_host + 2 * (size_t)n_steps) : std::vector<float>();
    Plan* pl;
    int rc = build_plan(u, n, H, W, &pl, lane);
    if (rc) return rc;
    td_engine* e = u->eng;
    hipStream_t st = e->stream;
    const int Cin = u->cfg.in_channels, C = u->cfg.out_channels, HW = H * W;
    if (C + cimg != Cin) return fail(TD_ERR_ARG, "in_channels must equal out_channels + conditioning-image channels");
    const size_t xbytes = (size_t)n * C * HW * 4;
    const bool x_dev = c.direct(x), cond_dev = c.direct(cond);
    HIP_TRY(hipMemcpyAsync(pl->x->p, x, xbytes, x_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (u->cond_row_len > 0) {
        const size_t cb = (size_t)n * u->cond_row_len * 4;
        HIP_TRY(hipMemcpyAsync(pl->cond->p, cond, cb, cond && cond_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    }
    if ((rc = stage_cond_img(u, *pl, n, HW, cond_img, cimg, C, c))) return rc;
    std::vector<float> ts(n_steps);
    for (int i = 0; i < n_steps; ++i) ts[i] = atanf(sigmas_host[i] / sigma_data);  // trigflow_precondition_noise (dpmsolver.py:240-242)
    if ((rc = compute_cvecs(u, *pl, ts, (const float*)pl->cond->p, c))) return rc;
    Plan* gpl = nullptr;
    if (guide) {
        if ((rc = build_plan(guide, n, H, W, &gpl, lane))) return rc;
        if ((rc = stage_cond_img(guide, *gpl, n, HW, cond_img, cimg, C, c))) return rc;
        if ((rc = compute_cvecs(guide, *gpl, ts, (const float*)pl->cond->p, c))) return rc;
    }
    std::vector<SchedCoef> ks;
    const int solver_order = (int)e->option("solver_order", 2);
    if (solver_order < 1 || solver_order > 3) return fail(TD_ERR_ARG, "solver_order must be 1, 2 or 3");
    const bool lof = e->option("lower_order_final", 1) != 0;
    const int fuse_opt = (int)e->option("fuse_solver", 1);
    dpm_coefs(sigmas_host, n_steps, sigma_data, solver_order, lof, ks);
    const float c_in0 = 1.f / sqrtf(sigmas_host[0] * sigmas_host[0] + sigma_data * sigma_data);
    // option "sampler_stop_after" = k >= 0 (test read-back): the table is that of the n_steps-step run, only its first k steps are enqueued, and the
    // solver history starts from zeros, so that "@m1" / "@m2" after the call depend on this call alone (a full run never reads what an earlier call
    // left there: the first step ignores m1, and m2 is overwritten twice before the first third-order step reads it)
    const int stop_after = (int)e->option("sampler_stop_after", -1);
    const int n_run = stop_after >= 0 ? std::min(stop_after, n_steps) : n_steps;
    if (stop_after >= 0) {
        HIP_TRY(hipMemsetAsync(pl->m1->p, 0, xbytes, st));
        HIP_TRY(hipMemsetAsync(pl->m2->p, 0, xbytes, st));
    }

    auto enqueue = [&]() -> int {
        TD_DISPATCH_T(u, hipLaunchKernelGGL(prep_input_kernel<T_>, grid1((size_t)n * HW), dim3(256), 0, st, (const float*)pl->x->p, (T_*)pl->xin, n, C, HW, u->chunk, c_in0, Cin));
        if (gpl) {
            TD_DISPATCH_T(u, hipLaunchKernelGGL(prep_input_kernel<T_>, grid1((size_t)n * HW), dim3(256), 0, st, (const float*)pl->x->p, (T_*)gpl->xin, n, C, HW, u->chunk, c_in0, Cin));
        }
        const float* Fg = gpl ? (const float*)gpl->F : nullptr;
        // north_star: "the per-tile EDM scheduler step fused into the epilogue".  Without a guide model the solver update of step i runs in the
        // epilogue of the U-Net's output conv (option "fuse_solver", default on; bit-identical to the separate kernel: same arithmetic on the same
        // fp32 F); with autoguidance the update needs BOTH models' outputs and stays a kernel of its own.
        const bool fuse = !gpl && alpha == 1.f && fuse_opt != 0 && pl->ops.back().kind == Op::CONV && pl->ops.back().p.epi == EPI_PLAIN && pl->ops.back().p.out_f32;
        for (int i = 0; i < n_run; ++i) {
            int r = run_unet(u, *pl, i, fuse ? &ks[i] : nullptr);
            if (r) return r;
            if (fuse) continue;
            if (gpl && (r = run_unet(guide, *gpl, i))) return r;
            if (alpha == 1.f) {
                TD_DISPATCH_T(u, hipLaunchKernelGGL(dpm_step_kernel<T_>, grid1((size_t)n * HW), dim3(256), 0, st, (float*)pl->x->p, (float*)pl->m1->p, (const float*)pl->F, (T_*)pl->xin, n, C, HW, 8, u->chunk, ks[i], Fg, gscale, gpl ? (T_*)gpl->xin : (T_*)nullptr, solver_order == 3 ? (float*)pl->m2->p : (float*)nullptr));
            } else {   // score scaling: the compile-time variant of the same step, scalars of step i from the caller's table
                const ScoreScale ss{alpha, cs[2 * i], cs[2 * i + 1], -sigma_data};
                TD_DISPATCH_T(u, hipLaunchKernelGGL(dpm_step_ss_kernel<T_>, grid1((size_t)n * HW), dim3(256), 0, st, (float*)pl->x->p, (float*)pl->m1->p, (const float*)pl->F, (T_*)pl->xin, n, C, HW, 8, u->chunk, ks[i], Fg, gscale, gpl ? (T_*)gpl->xin : (T_*)nullptr, solver_order == 3 ? (float*)pl->m2->p : (float*)nullptr, ss));
            }
        }
        HIP_TRY(hipGetLastError());
        return TD_OK;
    };

    const bool use_graph = e->option("graph", 1) != 0 && e->option("profile", 0) == 0;
    if (use_graph) {
        GraphKey key;
        key.sigmas.assign(sigmas_host, sigmas_host + n_steps + 1); key.sigma_data = sigma_data; key.solver_order = solver_order;
        key.lof = (int)lof; key.fuse = fuse_opt; key.stop = stop_after;
        // the guide's plan can be evicted / its buffers re-allocated independently of this plan: key the graph on them too
        key.guide = gpl; key.guide_cvec = gpl ? (const void*)gpl->cvec->p : nullptr; key.gscale = gscale;
        key.alpha = alpha; key.cs = cs;
        if (!pl->graph || !(pl->graph_key == key)) {
            pl->drop_graph();
            hipGraph_t g = nullptr;
            HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            rc = enqueue();
            hipError_t ce = hipStreamEndCapture(st, &g);
            if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
            if (ce != hipSuccess) return fail(TD_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(ce));
            hipError_t ie = hipGraphInstantiate(&pl->graph, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ie != hipSuccess) { pl->graph = nullptr; return fail(TD_ERR_HIP, std::string("graph instantiate: ") + hipGetErrorString(ie)); }
            pl->graph_key = std::move(key);
        }
        HIP_TRY(hipGraphLaunch(pl->graph, st));
    } else if ((rc = enqueue())) return rc;
    HIP_TRY(hipMemcpyAsync(x, pl->x->p, xbytes, x_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    return TD_OK;
}

// Engine option "dual_stream" (default 1 since round 6: +4.9 ... +5.1 % on the 8x8-grid bench in both A/B orders, +4.5 % on the 32x32 grid,
// profiles/r06_dual_stream_ab.txt; +2.3 % in round 2, profiles/r02_dual_stream_ab.txt):
// batches of >= "dual_stream_min_batch" tiles (default 32) run as TWO independent half-batches on two streams: tiles are independent, and a
// kernel whose grid does not fill a whole number of rounds of the 256 CUs (768 workgroups on 512 slots at the 16x16 level of a 64-tile
// batch: 1.5 rounds), its launch gap and its epilogue tail leave CUs idle that the other lane's kernels fill.  Every window's arithmetic is
// that of a half-size batch: the plan of a 32-window batch differs from a 64-window batch's in the layers whose tile / flavour / split-K choice
// depends on the grid size (1.6e-3 rel-RMS on the blended configs[2] canvas, bf16); batch_invariant mode pins those choices and gives the same bits.
// The second lane's stream is ordered behind the first lane's at entry (inputs produced on the engine's stream -- the caller's, with
// td_engine_set_stream -- are complete before lane two reads them) and the first lane's stream waits for the second at the end, so that the call ends
// like a single-lane one: results ordered on the engine's stream, enqueue-only under option "async".
// The sampler's body, enqueue-only: one lane or two on the engine's streams, ending ordered on e->stream.  On failure both streams are drained.
static int sample_edm_enqueue(td_unet* u, const td_edm_ext& a, Call& c) {
    td_engine* e = u->eng;
    const int n = a.n;
    const bool dual = e->stream2 && e->option("dual_stream", 1) != 0 && n >= std::max<int64_t>(2, e->option("dual_stream_min_batch", 32));
    const bool concurrent = e->option("profile", 0) == 0;  // profile mode times every launch with events on ONE stream: the lanes run one after the other
    if (!dual) {
        int rc = sample_edm_lane(u, a, 0, c);
        if (rc) (void)hipStreamSynchronize(e->stream);
        return rc;
    }
    // the second lane: the same call on the rest of the batch
    const int nA = n / 2, C = u->cfg.out_channels;
    const size_t HW = (size_t)a.H * a.W;
    td_edm_ext la = a, lb = a;
    la.n = nA; lb.n = n - nA;
    lb.cond = a.cond ? a.cond + (size_t)nA * u->cond_row_len : nullptr;
    lb.cond_img = a.cond_img ? a.cond_img + (size_t)nA * a.cimg_channels * HW : nullptr;
    lb.x = a.x + (size_t)nA * C * HW;
    if (concurrent) { HIP_TRY(hipEventRecord(e->ev_fork, e->stream)); HIP_TRY(hipStreamWaitEvent(e->stream2, e->ev_fork, 0)); }
    int rc = sample_edm_lane(u, la, 0, c);
    if (!rc) {
        if (concurrent) std::swap(e->stream, e->stream2);
        rc = sample_edm_lane(u, lb, 1, c);
        if (concurrent) std::swap(e->stream, e->stream2);
    }
    if (rc) { (void)hipStreamSynchronize(e->stream); (void)hipStreamSynchronize(e->stream2); return rc; }
    if (concurrent) { HIP_TRY(hipEventRecord(e->ev_join, e->stream2)); HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_join, 0)); }
    return TD_OK;
}

// default: results complete on return (the caller's framework uses other streams); option "async": left enqueued on e->stream
static int sample_edm_impl(td_unet* u, const td_edm_ext& a) {
    Call c(u->eng);
    int rc = sample_edm_enqueue(u, a, c);
    return rc ? rc : c.finish();
}

// the plain sampler's arguments as the struct: no guide, no score scaling
static td_edm_ext edm_args(int n, int H, int W, int n_steps, const float* sigmas_host, float sigma_data, const float* cond, const float* cond_img, int cimg, float* x) {
    td_edm_ext a;
    memset(&a, 0, sizeof a);
    a.n = n; a.H = H; a.W = W; a.n_steps = n_steps; a.sigmas_host = sigmas_host; a.sigma_data = sigma_data;
    a.cond = cond; a.cond_img = cond_img; a.cimg_channels = cimg; a.x = x;
    a.guidance_scale = 1.f; a.score_scaling = 1.f;
    return a;
}

int td_sample_edm_img(td_unet* u, int n, int H, int W, int n_steps, const float* sigmas_host, float sigma_data, const float* cond,
                      const float* cond_img, int cimg, float* x) {
    return sample_edm_impl(u, edm_args(n, H, W, n_steps, sigmas_host, sigma_data, cond, cond_img, cimg, x));
}
int td_sample_edm(td_unet* u, int n, int H, int W, int n_steps, const float* sigmas_host, float sigma_data, const float* cond, float* x) {
    return sample_edm_impl(u, edm_args(n, H, W, n_steps, sigmas_host, sigma_data, cond, nullptr, 0, x));
}
int td_sample_edm_guided(td_unet* u, td_unet* guide, float guidance_scale, int n, int H, int W, int n_steps, const float* sigmas_host, float sigma_data,
                         const float* cond, float* x) {
    if (!guide) return fail(TD_ERR_ARG, "null guide model");
    td_edm_ext a = edm_args(n, H, W, n_steps, sigmas_host, sigma_data, cond, nullptr, 0, x);
    a.guide = guide; a.guidance_scale = guidance_scale;
    return sample_edm_impl(u, a);
}

// Every argument of the EDM sampler in one struct: conditioning-image channels, a guide model and score scaling in any combination.  With no
// guide (or scale 1), score_scaling == 1 it is the call td_sample_edm_img makes; the guide's plan gets the same cond_img staged as the main one.
int td_sample_edm_ext(td_unet* u, const td_edm_ext* args) {
    if (!u || !args) return fail(TD_ERR_ARG, "td_sample_edm_ext: null argument");
    td_edm_ext a = *args;
    if (!a.sigmas_host || !a.x) return fail(TD_ERR_ARG, "td_sample_edm_ext: sigmas_host / x is null");
    if (a.cimg_channels < 0 || (a.cimg_channels > 0 && !a.cond_img)) return fail(TD_ERR_ARG, "td_sample_edm_ext: cond_img is null");
    if (!a.guide) a.guidance_scale = 1.f;
    if (a.cimg_channels == 0) a.cond_img = nullptr;
    return sample_edm_impl(u, a);
}

int td_sample_consistency_img(td_unet* u, int n, int H, int W, float t, float sigma_data, const float* sample, const float* z, const float* cond,
                              const float* cond_img, int cimg, float* out) {
    Call c(u->eng);
    if (!u->finalized) return fail(TD_ERR_STATE, "finalize first");
    Plan* pl;
    int rc = build_plan(u, n, H, W, &pl);
    if (rc) return rc;
    hipStream_t st = c.e->stream;
    const int Cin = u->cfg.in_channels, C = u->cfg.out_channels, HW = H * W;
    if (C + cimg != Cin) return fail(TD_ERR_ARG, "in_channels must equal out_channels + conditioning-image channels");
    const size_t xbytes = (size_t)n * C * HW * 4;
    const float* dz;
    if ((rc = c.in(z, xbytes, &dz))) return rc;
    const bool cond_dev = c.direct(cond);
    if (sample) HIP_TRY(hipMemcpyAsync(pl->x->p, sample, xbytes, c.direct(sample) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemsetAsync(pl->x->p, 0, xbytes, st));
    if (u->cond_row_len > 0)
        HIP_TRY(hipMemcpyAsync(pl->cond->p, cond, (size_t)n * u->cond_row_len * 4, cond && cond_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if ((rc = stage_cond_img(u, *pl, n, HW, cond_img, cimg, C, c))) return rc;
    if ((rc = compute_cvecs(u, *pl, std::vector<float>(1, t), (const float*)pl->cond->p, c))) return rc;
    float* dout;
    if ((rc = c.out(out, xbytes, &dout))) return rc;
    const float ct = cosf(t), sn = sinf(t);
    TD_DISPATCH_T(u, hipLaunchKernelGGL(consistency_pre_kernel<T_>, grid1((size_t)n * HW), dim3(256), 0, st, (const float*)pl->x->p, dz, (float*)pl->xt->p, (T_*)pl->xin, n, C, HW, u->chunk, ct, sn, sigma_data, Cin));
    if ((rc = run_unet(u, *pl, 0))) return rc;
    hipLaunchKernelGGL(consistency_post_kernel, grid1((size_t)n * HW), dim3(256), 0, st, (const float*)pl->xt->p, (const float*)pl->F, dout, n, C, HW, 8, ct, sn, sigma_data);
    HIP_TRY(hipGetLastError());
    return c.finish();
}

int td_sample_consistency(td_unet* u, int n, int H, int W, float t, float sigma_data, const float* sample, const float* z, const float* cond, float* out) {
    return td_sample_consistency_img(u, n, H, W, t, sigma_data, sample, z, cond, nullptr, 0, out);
}

// ---- noise
uint64_t td_tile_seed(uint64_t base_seed, int64_t ty, int64_t tx) {
    const uint64_t G = 0x9E3779B9ULL;
    uint64_t h = base_seed * G;
    h = h + ((uint64_t)ty & 0xFFFFFFFFULL);
    h = h * G + ((uint64_t)tx & 0xFFFFFFFFULL);
    return h;
}

int td_standard_normal(td_engine* e, uint64_t seed, int64_t n, float* out) {
    Call c(e);
    if (n <= 0) return TD_OK;
    float* dout;
    int rc;
    if ((rc = c.out(out, (size_t)n * 4, &dout))) return rc;
    Buf sd(new DevBuf());
    HIP_TRY(sd->alloc(8, false));
    HIP_TRY(hipMemcpyAsync(sd->p, &seed, 8, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(noise_tiles_kernel, dim3(1), dim3(256), 0, e->stream, (const uint64_t*)sd->p, dout, n);
    HIP_TRY(hipGetLastError());
    return c.finish(true);
}

static inline int64_t fdiv(int64_t a, int64_t b) { int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

// td_noise_patches in two halves: host preparation with its uploads, and the two launches.  NoiseJob owns the host arrays the uploads read
// (they have to outlive a copy that has not run yet: declared before the Call); the device side lives in the call scope.
struct NoiseJob {
    std::vector<uint64_t> seeds;
    std::vector<int> index, org;
    const uint64_t* dseeds = nullptr;
    float* dtiles = nullptr;
    const int *dindex = nullptr, *dorg = nullptr;
    int64_t tn = 0;
};
static int noise_prepare(Call& c, NoiseJob& j, uint64_t base_seed, int n_windows, const int64_t* origins, int h, int w, int channels, int tile_h, int tile_w) {
    if (h > tile_h || w > tile_w) return fail(TD_ERR_UNSUPPORTED, "window larger than the noise tile");
    // unique noise tiles touched by the windows
    std::map<std::pair<int64_t, int64_t>, int> slot;
    std::vector<uint64_t>& seeds = j.seeds;
    std::vector<int>& index = j.index; std::vector<int>& org = j.org;
    index.assign((size_t)n_windows * 4, 0); org.resize((size_t)n_windows * 2);
    for (int i = 0; i < n_windows; ++i) {
        const int64_t y0 = origins[2 * i], x0 = origins[2 * i + 1];
        org[2 * i] = (int)y0; org[2 * i + 1] = (int)x0;
        const int64_t ty0 = fdiv(y0, tile_h), ty1 = fdiv(y0 + h - 1, tile_h), tx0 = fdiv(x0, tile_w), tx1 = fdiv(x0 + w - 1, tile_w);
        for (int64_t ty = ty0; ty <= ty1; ++ty)
            for (int64_t tx = tx0; tx <= tx1; ++tx) {
                auto key = std::make_pair(ty, tx);
                auto it = slot.find(key);
                int s;
                if (it == slot.end()) { s = (int)seeds.size(); slot[key] = s; seeds.push_back(td_tile_seed(base_seed, ty, tx)); } else s = it->second;
                index[(size_t)i * 4 + (ty - ty0) * 2 + (tx - tx0)] = s;
            }
    }
    j.tn = (int64_t)channels * tile_h * tile_w;
    int rc;
    if ((rc = c.table(seeds.data(), seeds.size() * 8, &j.dseeds)) || (rc = c.scratch(seeds.size() * j.tn * 4, &j.dtiles)) ||
        (rc = c.table(index.data(), index.size() * 4, &j.dindex)) || (rc = c.table(org.data(), org.size() * 4, &j.dorg))) return rc;
    return TD_OK;
}
static int noise_enqueue(td_engine* e, const NoiseJob& j, int n_windows, int h, int w, int channels, int tile_h, int tile_w, float scale, float* out_dev) {
    hipStream_t st = e->stream;
    hipLaunchKernelGGL(noise_tiles_kernel, dim3((unsigned)j.seeds.size()), dim3(256), 0, st, j.dseeds, j.dtiles, j.tn);
    hipLaunchKernelGGL(noise_gather_kernel, dim3((channels * h * w + 255) / 256, n_windows), dim3(256), 0, st, (const float*)j.dtiles, j.dindex,
                       j.dorg, out_dev, channels, h, w, tile_h, tile_w, scale);
    HIP_TRY(hipGetLastError());
    return TD_OK;
}

int td_noise_patches(td_engine* e, uint64_t base_seed, int n_windows, const int64_t* origins, int h, int w, int channels, int tile_h, int tile_w,
                     float scale, float* out) {
    NoiseJob j;
    Call c(e);
    if (n_windows <= 0) return TD_OK;
    int rc;
    if ((rc = noise_prepare(c, j, base_seed, n_windows, origins, h, w, channels, tile_h, tile_w))) return rc;
    float* dout;
    if ((rc = c.out(out, (size_t)n_windows * channels * h * w * 4, &dout))) return rc;
    if ((rc = noise_enqueue(e, j, n_windows, h, w, channels, tile_h, tile_w, scale, dout))) return rc;
    return c.finish();
}

// ---- blend
static void weight_window_host(int size, std::vector<float>& w) {
    // world_pipeline.py:117-124 in fp32: wy = 1 - (1-eps)*clamp(|y-mid|/mid, 0, 1), eps = 1e-3, mid = (s-1)/2 (python float -> fp32 tensor ops)
    w.resize((size_t)size * size);
    const float mid = (float)((size - 1) / 2.0);
    const float k = (float)(1 - 1e-3);
    std::vector<float> a(size);
    for (int i = 0; i < size; ++i) {
        float d = fabsf((float)i - mid) / mid;
        d = fminf(fmaxf(d, 0.f), 1.f);
        a[i] = 1.f - k * d;
    }
    for (int y = 0; y < size; ++y)
        for (int x = 0; x < size; ++x) w[(size_t)y * size + x] = a[y] * a[x];
}

int td_linear_weight_window(td_engine* e, int size, float* out) {
    DevGuard dg_(e->device);
    std::vector<float> w;
    weight_window_host(size, w);
    HIP_TRY(hipMemcpy(out, w.data(), w.size() * 4, is_device_ptr(out) ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
    return TD_OK;
}

// td_blend_windows in two halves, like the noise: the row / column / slot maps with their six uploads, and the launch.
struct BlendJob {
    std::vector<int> rowmap, colmap, tile_of;
    std::vector<float> ww;
    const int32_t *drow = nullptr, *dcol = nullptr, *drs = nullptr, *dcs = nullptr, *dtof = nullptr;
    const float* dww = nullptr;
};
static int blend_prepare(Call& c, BlendJob& j, int C, int Hc, int Wc, int size, int n_rows, const int32_t* row_starts, int n_cols, const int32_t* col_starts,
                         int n_tiles, const int32_t* wi, const int32_t* wj, const float* window = nullptr) {
    if (C + 1 > 8) return fail(TD_ERR_UNSUPPORTED, "C+1 must be <= 8");
    std::vector<int>& rowmap = j.rowmap; std::vector<int>& colmap = j.colmap; std::vector<int>& tile_of = j.tile_of;
    rowmap.assign((size_t)Hc * 4, -1); colmap.assign((size_t)Wc * 4, -1); tile_of.assign((size_t)n_rows * n_cols, -1);
    for (int ic = 0; ic < n_rows; ++ic)
        for (int y = std::max(0, row_starts[ic]); y < std::min(Hc, row_starts[ic] + size); ++y) {
            int k = 0;
            while (k < 4 && rowmap[(size_t)y * 4 + k] >= 0) ++k;
            if (k == 4) return fail(TD_ERR_UNSUPPORTED, "more than 4 windows cover a canvas row");
            rowmap[(size_t)y * 4 + k] = ic;
        }
    for (int jc = 0; jc < n_cols; ++jc)
        for (int x = std::max(0, col_starts[jc]); x < std::min(Wc, col_starts[jc] + size); ++x) {
            int k = 0;
            while (k < 4 && colmap[(size_t)x * 4 + k] >= 0) ++k;
            if (k == 4) return fail(TD_ERR_UNSUPPORTED, "more than 4 windows cover a canvas column");
            colmap[(size_t)x * 4 + k] = jc;
        }
    for (int i = 0; i < n_tiles; ++i) {
        if (wi[i] < 0 || wi[i] >= n_rows || wj[i] < 0 || wj[i] >= n_cols) return fail(TD_ERR_ARG, "window index out of range");
        tile_of[(size_t)wi[i] * n_cols + wj[i]] = i;
    }
    // a caller's window (td_blend_windows_w) goes to this job's scratch like the linear one: never into the per-size cache e->wwin, which is keyed by size only
    if (!window) weight_window_host(size, j.ww);
    else {
        j.ww.resize((size_t)size * size);
        HIP_TRY(hipMemcpy(j.ww.data(), window, j.ww.size() * 4, is_device_ptr(window) ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
    }
    int rc;
    if ((rc = c.table(rowmap.data(), rowmap.size() * 4, &j.drow)) || (rc = c.table(colmap.data(), colmap.size() * 4, &j.dcol)) ||
        (rc = c.table(row_starts, (size_t)n_rows * 4, &j.drs)) || (rc = c.table(col_starts, (size_t)n_cols * 4, &j.dcs)) ||
        (rc = c.table(tile_of.data(), tile_of.size() * 4, &j.dtof)) || (rc = c.table(j.ww.data(), j.ww.size() * 4, &j.dww)))
        return rc;
    return TD_OK;
}
static int blend_enqueue(td_engine* e, const BlendJob& j, float* dcanvas, int C, int Hc, int Wc, int size, int n_cols, const float* dtiles, int accumulate) {
    hipLaunchKernelGGL(blend_gather_kernel, grid1((size_t)Hc * Wc), dim3(256), 0, e->stream, dtiles, j.dww, dcanvas, C, Hc, Wc, size,
                       j.drow, j.dcol, j.drs, j.dcs, j.dtof, n_cols, accumulate);
    HIP_TRY(hipGetLastError());
    return TD_OK;
}

int td_blend_windows(td_engine* e, float* canvas, int C, int Hc, int Wc, int size, int n_rows, const int32_t* row_starts, int n_cols,
                     const int32_t* col_starts, int n_tiles, const int32_t* wi, const int32_t* wj, const float* tiles, int accumulate) {
    return td_blend_windows_w(e, canvas, C, Hc, Wc, size, n_rows, row_starts, n_cols, col_starts, n_tiles, wi, wj, tiles, accumulate, nullptr);
}

int td_blend_windows_w(td_engine* e, float* canvas, int C, int Hc, int Wc, int size, int n_rows, const int32_t* row_starts, int n_cols,
                       const int32_t* col_starts, int n_tiles, const int32_t* wi, const int32_t* wj, const float* tiles, int accumulate, const float* window) {
    BlendJob j;
    Call c(e);
    int rc;
    if ((rc = blend_prepare(c, j, C, Hc, Wc, size, n_rows, row_starts, n_cols, col_starts, n_tiles, wi, wj, window))) return rc;
    const float* dt;
    float* dcanvas;
    if ((rc = c.in(tiles, (size_t)n_tiles * C * size * size * 4, &dt))) return rc;
    if ((rc = c.inout(canvas, (size_t)(C + 1) * Hc * Wc * 4, accumulate != 0, &dcanvas))) return rc;   // (a host canvas is read only when it is added to)
    if ((rc = blend_enqueue(e, j, dcanvas, C, Hc, Wc, size, n_cols, dt, accumulate))) return rc;
    return c.finish();
}

int td_gather_regions(td_engine* e, int C, int size, int n_regions, int h, int w, int maxk, const int32_t* desc_host, int n_windows,
                      const uint64_t* window_ptrs_host, float* out) {
    Call c(e);
    if (C + 1 > 8) return fail(TD_ERR_UNSUPPORTED, "C+1 must be <= 8");
    if (n_regions <= 0) return TD_OK;
    if (maxk < 1 || h < 1 || w < 1 || n_windows < 0 || !is_device_ptr(out)) return fail(TD_ERR_ARG, "td_gather_regions: bad shape / host output");
    for (size_t i = 0; i < (size_t)n_regions * maxk; ++i)
        if (desc_host[i * 3] >= n_windows) return fail(TD_ERR_ARG, "td_gather_regions: window slot out of range");
    hipStream_t st = e->stream;
    auto& ww = e->wwin[size];
    if (!ww) {
        std::vector<float> hw;
        weight_window_host(size, hw);
        ww.reset(new DevBuf());
        HIP_TRY(ww->alloc(hw.size() * 4, false));
        HIP_TRY(hipMemcpy(ww->p, hw.data(), hw.size() * 4, hipMemcpyHostToDevice));
    }
    const uint64_t* dptrs;
    const int32_t* ddesc;
    int rc;
    if ((rc = c.table(window_ptrs_host, (size_t)n_windows * 8, &dptrs)) || (rc = c.table(desc_host, (size_t)n_regions * maxk * 3 * 4, &ddesc))) return rc;
    hipLaunchKernelGGL(regions_gather_kernel, dim3((unsigned)(((size_t)h * w + 255) / 256), (unsigned)n_regions), dim3(256), 0, st, (const float* const*)dptrs,
                       ddesc, maxk, (const float*)ww->p, out, C, h, w, size);
    HIP_TRY(hipGetLastError());
    // default: complete on return.  Option "async": enqueued; the window tensors are then the caller's to keep valid IN STREAM ORDER (a torch
    // tensor released on the stream the engine runs on is: the allocator reuses its memory for later work of that stream only)
    return c.finish();
}

int td_blend_normalize(td_engine* e, const float* canvas, int C, int Hc, int Wc, float scale, float* out) {
    Call c(e);
    const float* dc;
    float* dout;
    int rc;
    if ((rc = c.in(canvas, (size_t)(C + 1) * Hc * Wc * 4, &dc)) || (rc = c.out(out, (size_t)C * Hc * Wc * 4, &dout))) return rc;
    hipLaunchKernelGGL(blend_normalize_kernel, grid1((size_t)Hc * Wc), dim3(256), 0, e->stream, dc, dout, C, Hc * Wc, scale);
    HIP_TRY(hipGetLastError());
    return c.finish();
}

// ---- conditioning rows (sample_diffusion_base.py:11-48 per window, on the GPU)
struct CondJob {
    std::vector<int32_t> stage;   // 2 n window positions, then the nh histogram floats (one upload)
    const int32_t* dstage = nullptr;
    const float* dgrid = nullptr;
    CondRowsParams p;
};
static int cond_prepare(Call& c, CondJob& j, const float* grid, int R, int Cg, int n, const int32_t* pos, const float* means, const float* stds,
                        const float* hist, int nh, float noise_level) {
    if (!grid || !pos || !means || !stds || (nh > 0 && !hist)) return fail(TD_ERR_ARG, "td_cond_rows: null argument");
    if (n < 1 || R < 4 || Cg < 4 || nh < 0 || nh > 4096) return fail(TD_ERR_ARG, "td_cond_rows: n >= 1, a grid of at least 4 x 4 cells, 0 <= nh <= 4096");
    for (int i = 0; i < n; ++i)
        if (pos[2 * i] < 0 || pos[2 * i] + 4 > R || pos[2 * i + 1] < 0 || pos[2 * i + 1] + 4 > Cg) return fail(TD_ERR_ARG, "td_cond_rows: window position outside the grid");
    CondRowsParams& p = j.p;
    for (int c = 0; c < 7; ++c) { p.mean[c] = means[c]; p.stdv[c] = stds[c]; }
    // the host path's python-float arithmetic, in its order: Cc = sqrt(sum_L / (6 * (1/6)^2)), factor_L = Cc / sqrt(L) * (1/6), then one cast to fp32
    const int L[6] = {16, 16, 4, 16, nh, 1};
    const double inv = 1.0 / 6;
    const double Cc = sqrt((double)(53 + nh) / (6 * pow(inv, 2.0)));
    for (int k = 0; k < 6; ++k) p.factor[k] = L[k] > 0 ? (float)(Cc / sqrt((double)L[k]) * inv) : 0.f;
    p.nan_fill = means[0];
    p.noise_entry = (noise_level - 0.5f) * (float)sqrt(12.0);
    p.R = R; p.Cg = Cg; p.nh = nh; p.n = n;
    int rc;
    if ((rc = c.in(grid, (size_t)7 * R * Cg * 4, &j.dgrid))) return rc;
    j.stage.resize((size_t)2 * n + nh);
    memcpy(j.stage.data(), pos, (size_t)2 * n * 4);
    if (nh) memcpy(j.stage.data() + (size_t)2 * n, hist, (size_t)nh * 4);
    return c.table(j.stage.data(), j.stage.size() * 4, &j.dstage);
}
static int cond_enqueue(td_engine* e, const CondJob& j, float* out_dev) {
    const int32_t* d = j.dstage;
    hipLaunchKernelGGL(cond_rows_kernel, grid1((size_t)j.p.n * (53 + j.p.nh)), dim3(256), 0, e->stream, j.dgrid, d,
                       (const float*)(d + (size_t)2 * j.p.n), out_dev, j.p);
    HIP_TRY(hipGetLastError());
    return TD_OK;
}

int td_cond_rows(td_engine* e, const float* grid, int grid_rows, int grid_cols, int n, const int32_t* pos_host, const float* means_host, const float* stds_host,
                 const float* hist_host, int n_hist, float noise_level, float* out) {
    if (!e || !out) return fail(TD_ERR_ARG, "td_cond_rows: null argument");
    CondJob j;
    Call c(e);
    int rc;
    if ((rc = cond_prepare(c, j, grid, grid_rows, grid_cols, n, pos_host, means_host, stds_host, hist_host, n_hist, noise_level))) return rc;
    float* dout;
    if ((rc = c.out(out, (size_t)n * (53 + n_hist) * 4, &dout))) return rc;
    if ((rc = cond_enqueue(e, j, dout))) return rc;
    return c.finish();
}

// ---- one window batch of the grid sampler as ONE call: every host preparation and upload first, then noise -> conditioning rows -> the sampler's
// lanes -> blend accumulate enqueued back to back on the engine's stream, and one end of call.  The same kernels on the same inputs in the same order as
// td_noise_patches + td_cond_rows + td_sample_edm + td_blend_windows, which wait for the stream four times and leave the GPU idle in between.
int td_sample_grid_batch(td_unet* u, const td_grid_batch* b) {
    if (!u || !b) return fail(TD_ERR_ARG, "td_sample_grid_batch: null argument");
    td_engine* e = u->eng;
    NoiseJob nj; CondJob cj; BlendJob bj;
    Call c(e);
    if (!u->finalized) return fail(TD_ERR_STATE, "finalize first");
    const int n = b->n, H = b->H, W = b->W, C = u->cfg.out_channels;
    if (n < 1 || H < 1 || W < 1 || !b->origins_host || !b->sigmas_host || b->n_steps < 1) return fail(TD_ERR_ARG, "td_sample_grid_batch: bad batch description");
    if (u->cfg.in_channels != C) return fail(TD_ERR_ARG, "td_sample_grid_batch: models with conditioning-image channels take td_sample_edm_img");
    if (!b->canvas && !b->windows_out) return fail(TD_ERR_ARG, "td_sample_grid_batch: neither a canvas nor a window buffer to write to");
    if ((b->canvas && !is_device_ptr(b->canvas)) || (b->windows_out && !is_device_ptr(b->windows_out))) return fail(TD_ERR_ARG, "td_sample_grid_batch: canvas and window buffer are device buffers");
    if (b->canvas && (H != b->size || W != b->size)) return fail(TD_ERR_ARG, "td_sample_grid_batch: the blend takes square windows of `size`");
    if (u->cond_row_len > 0 && !b->cond_rows && !b->cond_grid) return fail(TD_ERR_ARG, "td_sample_grid_batch: the model takes conditioning rows");
    if (b->cond_grid && !b->cond_rows && 53 + b->n_hist != u->cond_row_len) return fail(TD_ERR_ARG, "td_sample_grid_batch: 53 + n_hist must equal the model's conditioning row length");
    int rc;
    // host preparation and uploads
    if ((rc = noise_prepare(c, nj, b->noise_seed, n, b->origins_host, H, W, C, b->tile_h, b->tile_w))) return rc;
    const float* drows = nullptr;
    float* rows_out = nullptr;
    const bool rows_from_grid = u->cond_row_len > 0 && !b->cond_rows;
    if (rows_from_grid) {
        if ((rc = cond_prepare(c, cj, b->cond_grid, b->grid_rows, b->grid_cols, n, b->cond_pos_host, b->cond_means_host, b->cond_stds_host, b->hist_host, b->n_hist,
                               b->noise_level))) return rc;
        if ((rc = c.scratch((size_t)n * u->cond_row_len * 4, &rows_out))) return rc;
        drows = rows_out;
    } else if ((rc = c.in(b->cond_rows, (size_t)n * u->cond_row_len * 4, &drows))) return rc;   // (rows a model without conditional inputs never reads count too)
    if (b->canvas && (rc = blend_prepare(c, bj, C, b->Hc, b->Wc, b->size, b->n_rows, b->row_starts_host, b->n_cols, b->col_starts_host, n, b->wi_host, b->wj_host))) return rc;
    float* x = b->windows_out;
    if (!x && (rc = c.scratch((size_t)n * C * H * W * 4, &x))) return rc;
    // the GPU work, back to back
    if ((rc = noise_enqueue(e, nj, n, H, W, C, b->tile_h, b->tile_w, b->noise_scale, x))) return rc;
    if (rows_from_grid && (rc = cond_enqueue(e, cj, rows_out))) return rc;
    if ((rc = sample_edm_enqueue(u, edm_args(n, H, W, b->n_steps, b->sigmas_host, b->sigma_data, drows, nullptr, 0, x), c))) return rc;
    if (b->canvas && (rc = blend_enqueue(e, bj, b->canvas, C, b->Hc, b->Wc, b->size, b->n_cols, x, b->accumulate))) return rc;
    return c.finish();
}

// ---- output composition
int td_resample2d(td_engine* e, const float* in, int C, int Hin, int Win, int Hout, int Wout, const int32_t* iy, const float* wy, int Ky,
                  const int32_t* ix, const float* wx, int Kx, float* out) {
    Call c(e);
    if (C < 1 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || Ky < 1 || Kx < 1) return fail(TD_ERR_ARG, "td_resample2d: bad geometry");
    for (int i = 0; i < Hout * Ky; ++i) if (iy[i] < 0 || iy[i] >= Hin) return fail(TD_ERR_ARG, "td_resample2d: row tap out of range");
    for (int i = 0; i < Wout * Kx; ++i) if (ix[i] < 0 || ix[i] >= Win) return fail(TD_ERR_ARG, "td_resample2d: column tap out of range");
    hipStream_t st = e->stream;
    const float *din, *dwy, *dwx;
    const int32_t *diy, *dix;
    float *dout, *tmp;
    int rc;
    if ((rc = c.in(in, (size_t)C * Hin * Win * 4, &din)) || (rc = c.table(iy, (size_t)Hout * Ky * 4, &diy)) || (rc = c.table(wy, (size_t)Hout * Ky * 4, &dwy)) ||
        (rc = c.table(ix, (size_t)Wout * Kx * 4, &dix)) || (rc = c.table(wx, (size_t)Wout * Kx * 4, &dwx)) || (rc = c.out(out, (size_t)C * Hout * Wout * 4, &dout)) ||
        (rc = c.scratch((size_t)C * Hin * Wout * 4, &tmp))) return rc;
    hipLaunchKernelGGL(resample_rows_kernel, grid1((size_t)C * Hin * Wout), dim3(256), 0, st, din, tmp, C, Hin, Win, Wout, dix, dwx, Kx);
    hipLaunchKernelGGL(resample_cols_kernel, grid1((size_t)C * Hout * Wout), dim3(256), 0, st, (const float*)tmp, dout, C, Hin, Hout, Wout, diy, dwy, Ky);
    HIP_TRY(hipGetLastError());
    return c.finish();
}

int td_residual_plus(td_engine* e, const float* packed, const float* lowres_up, int Hp, int Wp, float res_mean, float res_std, float* out) {
    Call c(e);
    if (!is_device_ptr(packed) || !is_device_ptr(lowres_up) || !is_device_ptr(out)) return fail(TD_ERR_ARG, "td_residual_plus: device buffers only");
    hipLaunchKernelGGL(residual_plus_kernel, grid1((size_t)Hp * Wp), dim3(256), 0, e->stream, packed, lowres_up, out, Hp * Wp, res_mean, res_std);
    HIP_TRY(hipGetLastError());
    return c.finish();
}

int td_elev_finish(td_engine* e, const float* packed, const float* lowres_up, int Hp, int Wp, int oi, int oj, int h, int w, float res_mean, float res_std, float* out) {
    Call c(e);
    if (!is_device_ptr(packed) || !is_device_ptr(lowres_up) || !is_device_ptr(out)) return fail(TD_ERR_ARG, "td_elev_finish: device buffers only");
    if (oi < 0 || oj < 0 || oi + h > Hp || oj + w > Wp) return fail(TD_ERR_ARG, "td_elev_finish: crop outside the window");
    hipLaunchKernelGGL(elev_finish_kernel, grid1((size_t)h * w), dim3(256), 0, e->stream, packed, lowres_up, out, Hp, Wp, oi, oj, h, w, res_mean, res_std);
    HIP_TRY(hipGetLastError());
    return c.finish();
}

int td_ddim_cfg_step(td_engine* e, const float* latent, const float* pred_uncond, const float* pred_cond, int64_t n, float guidance_scale, float alpha_t,
                     float alpha_prev, float* out) {
    Call c(e);
    if (n < 1 || !(alpha_t > 0.f) || !(alpha_t <= 1.f) || !(alpha_prev > 0.f) || !(alpha_prev <= 1.f)) return fail(TD_ERR_ARG, "td_ddim_cfg_step: bad arguments");
    if (!is_device_ptr(latent) || !is_device_ptr(pred_uncond) || !is_device_ptr(pred_cond) || !is_device_ptr(out)) return fail(TD_ERR_ARG, "td_ddim_cfg_step: device buffers only");
    // the scheduler's scalars in fp32 from the (fp32) cumulative alphas, as torch computes alpha ** 0.5 on 0-d fp32 tensors
    hipLaunchKernelGGL(ddim_cfg_step_kernel, grid1((size_t)n), dim3(256), 0, e->stream, latent, pred_uncond, pred_cond, out, (size_t)n, guidance_scale,
                       sqrtf(1.f - alpha_t), sqrtf(alpha_t), sqrtf(alpha_prev), sqrtf(1.f - alpha_prev));
    HIP_TRY(hipGetLastError());
    return c.finish();
}

int td_climate_finish(td_engine* e, const float* feats, int Hs, int Ws, const float* elev, int i1, int j1, int h, int w, float S, int ci1, int cj1, float* out) {
    Call c(e);
    if (!is_device_ptr(feats) || !is_device_ptr(elev) || !is_device_ptr(out)) return fail(TD_ERR_ARG, "td_climate_finish: device buffers only");
    if (Hs < 1 || Ws < 1 || h < 1 || w < 1 || !(S > 0.f)) return fail(TD_ERR_ARG, "td_climate_finish: bad geometry");
    hipLaunchKernelGGL(climate_finish_kernel, grid1((size_t)h * w), dim3(256), 0, e->stream, feats, elev, out, Hs, Ws, i1, j1, h, w, S, ci1, cj1);
    HIP_TRY(hipGetLastError());
    return c.finish();
}

// ---- synthetic conditioning map channel
int td_perlin_map(td_engine* e, int rows, int cols, int i1, int j1, int seed, float frequency, int octaves, float lacunarity, float gain,
                  const float* src_quantiles, const float* dst_quantiles, int n_quantiles, float* out) {
    Call c(e);
    if (rows < 1 || cols < 1 || octaves < 1 || octaves > 16 || n_quantiles < 2) return fail(TD_ERR_ARG, "td_perlin_map: bad arguments");
    const float *ds, *dd;
    float* dout;
    int rc;
    if ((rc = c.in(src_quantiles, (size_t)n_quantiles * 4, &ds)) || (rc = c.in(dst_quantiles, (size_t)n_quantiles * 4, &dd)) || (rc = c.out(out, (size_t)rows * cols * 4, &dout))) return rc;
    hipLaunchKernelGGL(perlin_map_kernel, grid1((size_t)rows * cols), dim3(256), 0, e->stream, dout, rows, cols, i1, j1, seed, frequency, octaves, lacunarity, gain, ds, dd, n_quantiles);
    HIP_TRY(hipGetLastError());
    return c.finish(true);
}

// ---- generic attention (row N1): softmax(scale * Q K^T) V on the MFMA kernel
int td_attention(td_engine* e, const float* q, const float* k, const float* v, int B, int H, int Lq, int Lk, int D, float scale, int normalize, float* out) {
    Call c(e);
    if (B < 1 || H < 1 || Lq < 1 || Lk < 1 || D < 1 || D > 160) return fail(TD_ERR_ARG, "td_attention: 1 <= D <= 160, positive sizes");
    hipStream_t st = e->stream;
    const float *dq, *dk, *dv;
    float* dout;
    int rc;
    if ((rc = c.in(q, (size_t)B * H * Lq * D * 4, &dq)) || (rc = c.in(k, (size_t)B * H * Lk * D * 4, &dk)) || (rc = c.in(v, (size_t)B * H * Lk * D * 4, &dv)) ||
        (rc = c.out(out, (size_t)B * H * Lq * D * 4, &dout))) return rc;
    size_t qn, kn, vn;
    const size_t tot = attn_workspace_elems(B, H, Lq, Lk, D, &qn, &kn, &vn);
    Buf ws(new DevBuf());
    HIP_TRY(ws->alloc(tot * 2, false));
    __bf16 *Qp = (__bf16*)ws->p, *Kp = Qp + qn, *Vt = Kp + kn;
    const AttnStrides sq = {(long)H * Lq * D, (long)Lq * D, (long)D, 1L}, sk = {(long)H * Lk * D, (long)Lk * D, (long)D, 1L};
    HIP_TRY(attn_pack<float>(dq, dk, dv, sq, sk, sk, B, H, Lq, Lk, D, normalize, scale, Qp, Kp, Vt, st));
    HIP_TRY(attn_mfma(Qp, Kp, Vt, dout, nullptr, sq, B, H, Lq, Lk, D, st));
    return c.finish(true);
}

}  // extern "C"

// ================================================================================================ EDMAutoencoder
// Two graphs on the U-Net's block machinery (td_unet::kind 1 and 2), one handle, one parameter list under the reference's state-dict names.
struct td_ae {
    td_engine* eng = nullptr;
    td_ae_config cfg;
    std::unique_ptr<td_unet> enc, dec;
    AeDirect dir;
    int L = 0, D = 0, sdown = 1;
};

static td_unet* ae_owner(td_ae* a, const char* name) {
    if (a->enc->pindex.count(name)) return a->enc.get();
    if (a->dec->pindex.count(name)) return a->dec.get();
    return nullptr;
}
// names the reference's state dict carries and inference never reads (unet_block.py:72 with emb_channels = 0; edm_autoencoder.py:105; edm_unet.py:142-143)
static bool ae_ignored(const std::string& n) {
    const std::string eg = ".emb_gain";
    return (n.size() > eg.size() && n.compare(n.size() - eg.size(), eg.size(), eg) == 0) || n == "logvar" || n.rfind("encoder.logvar_", 0) == 0;
}

// (option "profile": the kernels of ae_kernels.hip are timed by a ProfScope under their own labels and counted with the U-Net's non-conv kernels,
// td_engine_profile_read: other_ms)

extern "C" {

int td_ae_create(td_engine* e, const td_ae_config* cfg, int dtype, td_ae** out) {
    if (!e || !cfg || !out) return fail(TD_ERR_ARG, "null argument");
    if (dtype != TD_DTYPE_F32 && dtype != TD_DTYPE_BF16 && dtype != TD_DTYPE_F16) return fail(TD_ERR_ARG, "dtype");
    const td_ae_config& c = *cfg;
    const int L = c.latent_channels, D = c.n_direct_skips;
    if (c.n_levels < 1 || c.n_levels > 8) return fail(TD_ERR_ARG, "n_levels out of range");
    if (L < 1) return fail(TD_ERR_ARG, "latent_channels must be given");
    if (L > 4) return fail(TD_ERR_UNSUPPORTED, "latent_channels must be <= 4 (the encoder's output conv writes 2 * latent_channels <= 8 channels)");
    if (D < 0 || D > 8 || L + D + 1 > 32) return fail(TD_ERR_UNSUPPORTED, "latent_channels + len(direct_skips) + 1 must fit one K chunk (<=32), at most 8 direct skips");
    if (c.in_channels < 1 || c.in_channels + 1 > 32) return fail(TD_ERR_UNSUPPORTED, "in_channels+1 must fit one K chunk (<=32)");
    if (c.out_channels < 1 || c.out_channels > 8) return fail(TD_ERR_UNSUPPORTED, "out_channels must be <= 8");
    for (int d = 0; d < D; ++d)
        if (c.direct_skips[d] < 0 || c.direct_skips[d] >= c.in_channels || c.direct_skips[d] >= c.out_channels) return fail(TD_ERR_ARG, "direct_skips entry outside the input / output channels");
    std::unique_ptr<td_ae> a(new td_ae());
    a->eng = e; a->cfg = c; a->L = L; a->D = D; a->sdown = 1 << (c.n_levels - 1);
    memset(&a->dir, 0, sizeof a->dir);
    a->dir.n = D;
    for (int d = 0; d < D; ++d) a->dir.ch[d] = c.direct_skips[d];
    for (int kind = 1; kind <= 2; ++kind) {
        std::unique_ptr<td_unet> u(new td_unet());
        u->eng = e; u->dt = dtype; u->bf16 = dtype != TD_DTYPE_F32; u->chunk = u->bf16 ? 64 : 32; u->kind = kind;
        memset(&u->cfg, 0, sizeof u->cfg);
        u->cfg.image_size = c.image_size; u->cfg.model_channels = c.model_channels; u->cfg.n_levels = c.n_levels;
        u->cfg.in_channels = kind == 1 ? c.in_channels : L + D;
        u->cfg.out_channels = kind == 1 ? 2 * L : c.out_channels;
        for (int l = 0; l < c.n_levels; ++l) { u->cfg.channel_mults[l] = c.channel_mults[l]; u->cfg.layers_per_block[l] = c.layers_per_block[l]; }
        u->cfg.n_attn_resolutions = std::min(8, std::max(0, c.n_attn_resolutions));
        for (int i = 0; i < u->cfg.n_attn_resolutions; ++i) u->cfg.attn_resolutions[i] = c.attn_resolutions[i];
        u->cfg.midblock_attention = kind == 2 ? c.midblock_attention : 0;   // (the encoder has no mid block: edm_unet.py:128-129)
        u->cfg.concat_balance = 0.5f;
        int rc = init_graph(u.get(), c.layers_per_block_decoder);
        if (rc) return rc;
        (kind == 1 ? a->enc : a->dec) = std::move(u);
    }
    *out = a.release();
    return TD_OK;
}
void td_ae_destroy(td_ae* a) {
    if (!a) return;
    DevGuard dg_(a->eng->device);
    (void)hipStreamSynchronize(a->eng->stream);
    delete a;
}
int td_ae_num_params(td_ae* a) { return (int)(a->enc->params.size() + a->dec->params.size()); }
int td_ae_param_info(td_ae* a, int i, const char** name, int32_t* ndim, int64_t shape[4]) {
    const int ne = (int)a->enc->params.size();
    if (i < 0 || i >= td_ae_num_params(a)) return fail(TD_ERR_ARG, "index");
    return i < ne ? td_unet_param_info(a->enc.get(), i, name, ndim, shape) : td_unet_param_info(a->dec.get(), i - ne, name, ndim, shape);
}
int td_ae_set_param(td_ae* a, const char* name, const float* host_data, int64_t numel) {
    if (!a || !name) return fail(TD_ERR_ARG, "null argument");
    if (ae_ignored(name)) return TD_OK;
    td_unet* u = ae_owner(a, name);
    if (!u) return fail(TD_ERR_ARG, std::string("unknown parameter ") + name);
    return td_unet_set_param(u, name, host_data, numel);
}
int td_ae_set_prefolded(td_ae* a, int prefolded) {
    int rc = td_unet_set_prefolded(a->enc.get(), prefolded);
    return rc ? rc : td_unet_set_prefolded(a->dec.get(), prefolded);
}
int td_ae_finalize(td_ae* a) {
    int rc = td_unet_finalize(a->enc.get());
    return rc ? rc : td_unet_finalize(a->dec.get());
}

int td_ae_preencode(td_ae* a, int n_src, int H, int W, const float* x, float mean, float std, int dihedral, float* means, float* logvars, void* packed_f16) {
    if (!a || !x || !means || !logvars) return fail(TD_ERR_ARG, "td_ae_preencode: null argument");
    td_engine* e = a->eng;
    td_unet* u = a->enc.get();
    Call c(e);
    if (!u->finalized) return fail(TD_ERR_STATE, "finalize first");
    if (n_src < 1 || H < 1 || W < 1) return fail(TD_ERR_ARG, "td_ae_preencode: bad geometry");
    if (dihedral && H != W) return fail(TD_ERR_UNSUPPORTED, "td_ae_preencode: the dihedral form needs H == W");
    const int n = dihedral ? 8 * n_src : n_src, C = a->cfg.in_channels, LD = a->L + a->D, s = a->sdown;
    Plan* pl;
    int rc = build_plan(u, n, H, W, &pl);   // (refuses H, W not divisible by 2^(levels-1))
    if (rc) return rc;
    const int h = H / s, w = W / s;
    hipStream_t st = e->stream;
    const float* dx;
    float *dmeans, *dlogvars;
    void* dpacked = nullptr;
    const size_t lat = (size_t)n * LD * h * w;
    if ((rc = c.in(x, (size_t)n_src * C * H * W * 4, &dx)) || (rc = c.out(means, lat * 4, &dmeans)) || (rc = c.out(logvars, lat * 4, &dlogvars))) return rc;
    if (packed_f16 && (rc = c.out(packed_f16, lat * 2 * 2, &dpacked))) return rc;
    AeSrc src;
    src.x = dx; src.C = C; src.H = H; src.W = W; src.dihedral = dihedral ? 1 : 0; src.mean = mean; src.std = std;
    ProfScope prof(e);
    prof.begin();
    TD_DISPATCH_T(u, hipLaunchKernelGGL(ae_prep_input_kernel<T_>, grid1((size_t)n * H * W), dim3(256), 0, st, src, (T_*)pl->xin, n, u->chunk));
    prof.end("ae_prep_input");
    HIP_TRY(hipGetLastError());
    if ((rc = run_unet(u, *pl, 0))) return rc;
    prof.begin();
    hipLaunchKernelGGL(ae_latent_head_kernel, grid1((size_t)n * h * w), dim3(256), 0, st, (const float*)pl->F, 8, src, a->dir, n, a->L, h, w, s, dmeans, dlogvars, (_Float16*)dpacked);
    prof.end("ae_latent_head");
    HIP_TRY(hipGetLastError());
    return c.finish();
}

int td_ae_postencode(td_ae* a, int64_t numel, const float* means, const float* logvars, const float* eps, float* z) {
    if (!a || !means || !logvars || !eps || !z || numel < 1) return fail(TD_ERR_ARG, "td_ae_postencode: bad arguments");
    td_engine* e = a->eng;
    Call c(e);
    const float *dm, *dl, *de;
    float* dz;
    int rc;
    if ((rc = c.in(means, (size_t)numel * 4, &dm)) || (rc = c.in(logvars, (size_t)numel * 4, &dl)) || (rc = c.in(eps, (size_t)numel * 4, &de)) ||
        (rc = c.out(z, (size_t)numel * 4, &dz))) return rc;
    hipLaunchKernelGGL(ae_postencode_kernel, grid1((size_t)numel), dim3(256), 0, e->stream, dm, dl, de, dz, (size_t)numel);
    HIP_TRY(hipGetLastError());
    return c.finish();
}

int td_ae_decode(td_ae* a, int n, int h, int w, const float* z, float std, float mean, float* out) {
    if (!a || !z || !out) return fail(TD_ERR_ARG, "td_ae_decode: null argument");
    td_engine* e = a->eng;
    td_unet* u = a->dec.get();
    Call c(e);
    if (!u->finalized) return fail(TD_ERR_STATE, "finalize first");
    if (n < 1 || h < 1 || w < 1) return fail(TD_ERR_ARG, "td_ae_decode: bad geometry");
    Plan* pl;
    int rc = build_plan(u, n, h, w, &pl);
    if (rc) return rc;
    const int LD = a->L + a->D, s = a->sdown, H = h * s, W = w * s, Co = a->cfg.out_channels;
    hipStream_t st = e->stream;
    const float* dz;
    float* dout;
    if ((rc = c.in(z, (size_t)n * LD * h * w * 4, &dz)) || (rc = c.out(out, (size_t)n * Co * H * W * 4, &dout))) return rc;
    // z + ones channel -> NHWC storage type (edm_autoencoder.py:137): the U-Net's input staging as it is
    ProfScope prof(e);
    prof.begin();
    TD_DISPATCH_T(u, hipLaunchKernelGGL(prep_input_kernel<T_>, grid1((size_t)n * h * w), dim3(256), 0, st, dz, (T_*)pl->xin, n, LD, h * w, u->chunk, 1.f, LD));
    prof.end("ae_decode_head");
    HIP_TRY(hipGetLastError());
    if ((rc = run_unet(u, *pl, 0))) return rc;
    prof.begin();
    hipLaunchKernelGGL(ae_decode_finish_kernel, grid1((size_t)n * H * W), dim3(256), 0, st, (const float*)pl->F, 8, dz, a->dir, n, Co, a->L, H, W, s,
                       (std != 1.f || mean != 0.f) ? 1 : 0, std, mean, dout);
    prof.end("ae_decode_finish");
    HIP_TRY(hipGetLastError());
    return c.finish();
}

int td_ae_read_activation(td_ae* a, int stack, int n, int H, int W, const char* label, float* out_host, int64_t capacity, int32_t dims[4]) {
    if (!a || !label || !out_host || !dims) return fail(TD_ERR_ARG, "td_ae_read_activation: null argument");
    if (stack != 1 && stack != 2) return fail(TD_ERR_ARG, "td_ae_read_activation: stack is 1 (encoder) or 2 (decoder)");
    if (n < 1 || H < 1 || W < 1) return fail(TD_ERR_ARG, "td_ae_read_activation: bad geometry");
    // a kind != 0 plan has no embedding or cvec buffer (its modulation is d_ones) and 16 bytes of sampler state (build_plan: xbytes)
    for (const char* none : {"@emb", "@cvec", "@emb:rows", "@cvec:rows", "@x", "@m1", "@m2", "@xt"})
        if (!strcmp(label, none)) return fail(TD_ERR_ARG, std::string("td_ae_read_activation: the autoencoder's stacks have no ") + label);
    td_unet* u = stack == 1 ? a->enc.get() : a->dec.get();
    if (!u->finalized) return fail(TD_ERR_STATE, "finalize first");
    return td_unet_read_activation(u, n, H, W, label, out_host, capacity, dims);
}

}  // extern "C"
