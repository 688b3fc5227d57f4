// kernels_reduce.hip -- the device code of the reduce stage of reduce_runs / reduce_by_key (reduce_kernels.hpp) for both key widths,
// both value widths and the three operators, instantiated here so that it compiles beside primitives.hip (see kernels_perdigit.hip).
#include <hip/hip_runtime.h>

#define ADLHIP_KERNEL static   // the headers' non-template kernels belong to primitives.hip
#include "reduce_kernels.hpp"

#define X(...) template __global__ __VA_ARGS__;
#include "reduce_kernels.inc"
#undef X
