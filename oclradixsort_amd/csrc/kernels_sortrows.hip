// kernels_sortrows.hip -- the device code of the sort along rows (sortrows_kernels.hpp) for every key type and order, instantiated here
// so that it compiles beside primitives.hip (see kernels_perdigit.hip).
#include <hip/hip_runtime.h>

#define ADLHIP_KERNEL static   // the headers' non-template kernels belong to primitives.hip
#include "sortrows_kernels.hpp"

#define X(...) template __global__ __VA_ARGS__;
#include "sortrows_kernels.inc"
#undef X
