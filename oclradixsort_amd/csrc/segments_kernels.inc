// segments_kernels.inc -- the instantiations of segments_kernels.hpp (sort within segments), compiled in a translation unit of their
// own (kernels_segments.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip, explicit instantiation in
// kernels_segments.hip.
#define SEGMENTS_TYPED(U, KIND, DESC)                                                                                                 \
    X(void adlhip::segments_sort_kernel<U, KIND, DESC>(U const*, unsigned int, unsigned int const*, unsigned int, unsigned int const*, \
                                                       unsigned int const*, unsigned int, U*, unsigned int*))
#define SEGMENTS_WIDTH(U)                                                                                                             \
    SEGMENTS_TYPED(U, 0, 0) SEGMENTS_TYPED(U, 0, 1) SEGMENTS_TYPED(U, 1, 0) SEGMENTS_TYPED(U, 1, 1) SEGMENTS_TYPED(U, 2, 0)           \
    SEGMENTS_TYPED(U, 2, 1)                                                                                                           \
    X(void adlhip::segments_emit_kernel<U>(U const*, unsigned int const*, unsigned int const*, unsigned int, unsigned int const*,    \
                                           unsigned int, unsigned int, U*, unsigned int*))
SEGMENTS_WIDTH(uint32_t)
SEGMENTS_WIDTH(uint64_t)
#undef SEGMENTS_WIDTH
#undef SEGMENTS_TYPED
