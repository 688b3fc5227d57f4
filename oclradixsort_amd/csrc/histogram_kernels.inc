// histogram_kernels.inc -- the instantiations of histogram_kernels.hpp (adlhip_histogram_range_typed / adlhip_bincount_typed), compiled
// in a translation unit of their own (kernels_histogram.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip,
// explicit instantiation in kernels_histogram.hip.  Per key width: the count kernel in range and in bincount mode, and the two boundary
// kernels of the sorted path.  The key's kind and include_upper are run-time arguments.
#define HIST_COUNT(U, MODE)                                                                                                              \
    X(void adlhip::hist_count_kernel<U, MODE>(U const*, unsigned int, unsigned int, unsigned int, U const*, adlhip::HistArgs, unsigned int*))
#define HIST_WIDTH(U)                                                                                \
    HIST_COUNT(U, adlhip::kHistRange) HIST_COUNT(U, adlhip::kHistBincount)                           \
    X(void adlhip::hist_heads_kernel<U>(U const*, unsigned int, unsigned int, unsigned int*))        \
    X(void adlhip::hist_tails_kernel<U>(U const*, unsigned int, unsigned int, unsigned int*))
HIST_WIDTH(uint32_t)
HIST_WIDTH(uint64_t)
#undef HIST_WIDTH
#undef HIST_COUNT
