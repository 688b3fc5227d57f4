// kernels_scan.hip -- the device code of the scan stage of scan_typed / scan_by_key (scan_kernels.hpp) without keys and for both key
// widths, both value widths and the three operators, instantiated here so that it compiles beside primitives.hip (see
// kernels_perdigit.hip).
#include <hip/hip_runtime.h>

#define ADLHIP_KERNEL static   // the headers' non-template kernels belong to primitives.hip
#include "scan_kernels.hpp"

#define X(...) template __global__ __VA_ARGS__;
#include "scan_kernels.inc"
#undef X
