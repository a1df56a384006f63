// libtd_relief.so: the C-ABI of include/td_relief.h over the two kernels of relief_kernels.hip (the shade kernel without overlays).
#include "../side_csrc/td_side_host.h"
#include "../../include/td_relief.h"
#include "relief_host.h"

using namespace td;

extern "C" {

const char* td_relief_last_error(void) { return g_err.c_str(); }

int td_relief_map(void* hip_stream, const float* elev, int H, int W, const float* lut, const float* wl, int rl, const float* ws, int rs,
                  double azimuth_deg, double resolution, double relief, int has_range, double vmin, double vmax, int has_fill, double fill,
                  float* out, int synchronize) {
    return relief_render<false>("td_relief_map", hip_stream, elev, H, W, lut, wl, rl, ws, rs, azimuth_deg, resolution, relief, has_range, vmin, vmax,
                                has_fill, fill, ReliefOverlay{}, out, synchronize);
}

}  // extern "C"
