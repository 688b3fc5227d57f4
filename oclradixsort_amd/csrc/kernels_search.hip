// kernels_search.hip -- the device code of the sorted search (search_kernels.hpp) for the two key widths and the two sides,
// instantiated here so that it compiles beside primitives.hip (see kernels_perdigit.hip).
#include <hip/hip_runtime.h>

#define ADLHIP_KERNEL static   // the headers' non-template kernels belong to primitives.hip
#include "search_kernels.hpp"

#define X(...) template __global__ __VA_ARGS__;
#include "search_kernels.inc"
#undef X
