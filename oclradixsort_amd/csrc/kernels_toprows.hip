// kernels_toprows.hip -- the device code of the row-wise top-k (toprows_kernels.hpp) for every key type and order, instantiated here
// so that it compiles beside primitives.hip (see kernels_perdigit.hip).
#include <hip/hip_runtime.h>

#define ADLHIP_KERNEL static   // the headers' non-template kernels belong to primitives.hip
#include "toprows_kernels.hpp"

#define X(...) template __global__ __VA_ARGS__;
#include "toprows_kernels.inc"
#undef X
