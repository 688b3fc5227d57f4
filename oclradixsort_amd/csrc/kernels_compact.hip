// kernels_compact.hip -- the device code of stream compaction (compact_kernels.hpp) for the three predicate sources and the three
// widths of the array that travels along, instantiated here so that it compiles beside primitives.hip (see kernels_perdigit.hip).
#include <hip/hip_runtime.h>

#define ADLHIP_KERNEL static   // the headers' non-template kernels belong to primitives.hip
#include "compact_kernels.hpp"

#define X(...) template __global__ __VA_ARGS__;
#include "compact_kernels.inc"
#undef X
