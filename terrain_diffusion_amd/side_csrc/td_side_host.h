// Host scaffold of the side libraries (libtd_relief.so, libtd_hydro.so, libtd_mc.so, libtd_explorer.so): status codes, the last-error text,
// pointer and launch helpers, and the common tail of an entry point.  Header-only and in an anonymous namespace: each library is one
// translation unit and keeps its OWN thread-local error string, which its td_<lib>_last_error returns.  The engine (csrc/engine.hip) has its
// own copies: its sources are tied to the build id of the committed profiles.
#pragma once
#include <hip/hip_runtime.h>
#include <string>

namespace {
enum { OK = 0, ERR_ARG = -1, ERR_HIP = -2 };
thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define TD_HIP_TRY(expr)                                                                                         \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) return fail(ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

unsigned blocks(long long n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// the tail of every entry point: frees the scratch (if any) in stream order -- also when `err` is set --, reports the first error,
// synchronises on request
int finish(hipStream_t st, void* scratch, hipError_t err, int synchronize) {
    const hipError_t ferr = scratch ? hipFreeAsync(scratch, st) : hipSuccess;
    TD_HIP_TRY(err);
    TD_HIP_TRY(ferr);
    if (synchronize) TD_HIP_TRY(hipStreamSynchronize(st));
    return OK;
}
}  // namespace
