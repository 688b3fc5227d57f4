// unique_kernels.inc -- the instantiations of unique_kernels.hpp (run stage of unique / run-length encode), compiled in a translation
// unit of their own (kernels_unique.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip, explicit instantiation in
// kernels_unique.hip.
#define RUNS_EMIT(U, HAS_INDEX)                                                                                                      \
    X(void adlhip::runs_emit_kernel<U, HAS_INDEX>(U const*, unsigned int const*, unsigned int, unsigned int, unsigned int,            \
                                                  unsigned int const*, U*, unsigned int*, unsigned int*, unsigned int*))
#define RUNS_WIDTH(U)                                                                                                                 \
    X(void adlhip::runs_count_kernel<U>(U const*, unsigned int, unsigned int, unsigned int, unsigned int*))                           \
    RUNS_EMIT(U, 0) RUNS_EMIT(U, 1)
RUNS_WIDTH(uint32_t)
RUNS_WIDTH(uint64_t)
#undef RUNS_WIDTH
#undef RUNS_EMIT
