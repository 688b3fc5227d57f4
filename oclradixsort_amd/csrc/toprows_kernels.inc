// toprows_kernels.inc -- the instantiations of toprows_kernels.hpp (row-wise top-k), compiled in a translation unit of their own
// (kernels_toprows.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip, explicit instantiation in kernels_toprows.hip.
#define ROWS_TYPED(U, KIND, DESC)                                                                                                     \
    X(void adlhip::topk_rows_kernel<U, KIND, DESC>(U const*, size_t, unsigned int, size_t, unsigned int, U*, unsigned int*, adlhip::RowPlan))
#define ROWS_WIDTH(U) ROWS_TYPED(U, 0, 0) ROWS_TYPED(U, 0, 1) ROWS_TYPED(U, 1, 0) ROWS_TYPED(U, 1, 1) ROWS_TYPED(U, 2, 0) ROWS_TYPED(U, 2, 1)
ROWS_WIDTH(uint32_t)
ROWS_WIDTH(uint64_t)
#undef ROWS_WIDTH
#undef ROWS_TYPED
