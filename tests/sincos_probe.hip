// Test-side probe, not product code: the device's fast sine and cosine at the 128 gradient angles of perlin_map_kernel (csrc/compose_kernels.hip:pn_grad), with
// the angle spelled as the kernel spells it.  tests/test_synth_ops_gpu.py builds it with the engine's flags, holds the angles to the twin's bit for bit and measures
// the two intrinsics against float64 (tests/_synth_twin.py: EPS_SINCOS).
#include <hip/hip_runtime.h>

__global__ void sincos_probe_kernel(float* __restrict__ angle, float* __restrict__ c, float* __restrict__ s) {
    const int h = threadIdx.x;
    const float a = (float)(h & 127) * (6.283185307179586f / 128.f) + (3.141592653589793f / 128.f);
    angle[h] = a;
    c[h] = __cosf(a);
    s[h] = __sinf(a);
}

// three device buffers of 128 floats; returns the HIP error code (0: success)
extern "C" int sincos_probe(float* angle, float* c, float* s) {
    hipLaunchKernelGGL(sincos_probe_kernel, dim3(1), dim3(128), 0, 0, angle, c, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)hipDeviceSynchronize();
}
