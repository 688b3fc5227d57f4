// kernels_unique.hip -- the device code of the run stage of unique / run-length encode (unique_kernels.hpp) for both key widths,
// instantiated here so that it compiles beside primitives.hip (see kernels_perdigit.hip).
#include <hip/hip_runtime.h>

#define ADLHIP_KERNEL static   // the headers' non-template kernels belong to primitives.hip
#include "unique_kernels.hpp"

#define X(...) template __global__ __VA_ARGS__;
#include "unique_kernels.inc"
#undef X
