// The 16x16x32 wide tile as its own object for tools/conv_bench.hip (see tools/build_bench.sh).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "conv_glds_wide16.hip"
