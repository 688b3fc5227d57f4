// join_kernels.inc -- the instantiations of join_kernels.hpp (adlhip_join_sorted_typed, adlhip_expand_runs), compiled in a translation
// unit of their own (kernels_join.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip, explicit
// instantiation in kernels_join.hip.  One bounds kernel per key width; one row kernel per width of the values (none, 4, 8 bytes).  The
// key's kind, the order and the kind of join are run-time arguments.  (The sum, scan, starts and partition kernels are no templates.)
#define JOIN_BOUNDS(K)                                                                                                             \
    X(void adlhip::join_bounds_kernel<K>(K const*, unsigned int, K const*, adlhip::SearchArgs, adlhip::RedCodec, unsigned int,    \
                                         unsigned int, unsigned int, unsigned int*, unsigned int*, unsigned long*))
#define EXPAND_ROWS(V)                                                                                                             \
    X(void adlhip::expand_rows_kernel<V>(unsigned int const*, unsigned int, unsigned long const*, unsigned int, unsigned int const*, \
                                         unsigned int, unsigned int, unsigned int const*, V const*, unsigned int*, unsigned int*, V*))
JOIN_BOUNDS(uint32_t)
JOIN_BOUNDS(uint64_t)
EXPAND_ROWS(adlhip::MergeNone)
EXPAND_ROWS(uint32_t)
EXPAND_ROWS(uint64_t)
#undef EXPAND_ROWS
#undef JOIN_BOUNDS
