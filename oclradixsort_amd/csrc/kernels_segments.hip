// kernels_segments.hip -- the device code of the sort within segments (segments_kernels.hpp) for every key type and order,
// instantiated here so that it compiles beside primitives.hip (see kernels_perdigit.hip).
#include <hip/hip_runtime.h>

#define ADLHIP_KERNEL static   // the headers' non-template kernels belong to primitives.hip
#include "segments_kernels.hpp"

#define X(...) template __global__ __VA_ARGS__;
#include "segments_kernels.inc"
#undef X
