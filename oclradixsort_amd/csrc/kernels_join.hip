// kernels_join.hip -- the device code of the join of sorted sequences and of the expansion of runs (join_kernels.hpp) for the two key
// widths and the three widths of the values, instantiated here so that it compiles beside primitives.hip (see kernels_perdigit.hip).
#include <hip/hip_runtime.h>

#define ADLHIP_KERNEL static   // the headers' non-template kernels belong to primitives.hip
#include "join_kernels.hpp"

#define X(...) template __global__ __VA_ARGS__;
#include "join_kernels.inc"
#undef X
