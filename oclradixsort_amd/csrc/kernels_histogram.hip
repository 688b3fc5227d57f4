// kernels_histogram.hip -- the device code of the histograms (histogram_kernels.hpp) for the two key widths, instantiated here so that
// it compiles beside primitives.hip (see kernels_perdigit.hip).
#include <hip/hip_runtime.h>

#define ADLHIP_KERNEL static   // the headers' non-template kernels belong to primitives.hip
#include "histogram_kernels.hpp"

#define X(...) template __global__ __VA_ARGS__;
#include "histogram_kernels.inc"
#undef X
