// sortrows_kernels.inc -- the instantiations of sortrows_kernels.hpp (sort along rows), compiled in a translation unit of their own
// (kernels_sortrows.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip, explicit instantiation in kernels_sortrows.hip.
#define SORTROWS_TYPED(U, KIND, DESC)                                                                                                 \
    X(void adlhip::sort_rows_kernel<U, KIND, DESC>(U const*, size_t, unsigned int, size_t, unsigned int, uint64_t, U*, unsigned int*))
#define SORTROWS_WIDTH(U)                                                                                                             \
    SORTROWS_TYPED(U, 0, 0) SORTROWS_TYPED(U, 0, 1) SORTROWS_TYPED(U, 1, 0) SORTROWS_TYPED(U, 1, 1) SORTROWS_TYPED(U, 2, 0)           \
    SORTROWS_TYPED(U, 2, 1)                                                                                                           \
    X(void adlhip::rows_pack_kernel<U>(U const*, size_t, unsigned int, size_t, U*))                                                   \
    X(void adlhip::rows_emit_kernel<U>(U const*, unsigned int const*, unsigned int const*, size_t, unsigned int, size_t, U*, unsigned int*))
SORTROWS_WIDTH(uint32_t)
SORTROWS_WIDTH(uint64_t)
#undef SORTROWS_WIDTH
#undef SORTROWS_TYPED
