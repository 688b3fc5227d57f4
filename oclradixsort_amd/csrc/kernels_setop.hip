// kernels_setop.hip -- the device code of the set operations on sorted sequences (setop_kernels.hpp) for the two key widths and the
// three widths of the values, instantiated here so that it compiles beside primitives.hip (see kernels_perdigit.hip).
#include <hip/hip_runtime.h>

#define ADLHIP_KERNEL static   // the headers' non-template kernels belong to primitives.hip
#include "setop_kernels.hpp"

#define X(...) template __global__ __VA_ARGS__;
#include "setop_kernels.inc"
#undef X
