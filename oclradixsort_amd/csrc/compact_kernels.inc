// compact_kernels.inc -- the instantiations of compact_kernels.hpp (adlhip_compact_flagged / adlhip_compact_if_typed), compiled in a
// translation unit of their own (kernels_compact.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip,
// explicit instantiation in kernels_compact.hip.  Per predicate source (flag bytes, 4-byte keys, 8-byte keys): one count kernel, and
// one emit kernel per width of the array that travels along (none, 4, 8 bytes: the flagged form's items, the if form's values).  The
// key's kind, cmp and partition are run-time arguments.
#define COMPACT_COUNT(P) \
    X(void adlhip::compact_count_kernel<P>(P const*, unsigned int, unsigned int, unsigned int, adlhip::CompactPred, unsigned int*))
#define COMPACT_EMIT(P, V)                                                                                                          \
    X(void adlhip::compact_emit_kernel<P, V>(P const*, V const*, unsigned int, unsigned int, unsigned int, adlhip::CompactPred,    \
                                             unsigned int const*, unsigned int const*, unsigned int, P*, V*, unsigned int*))
#define COMPACT_SOURCE(P) \
    COMPACT_COUNT(P) COMPACT_EMIT(P, adlhip::CompactNone) COMPACT_EMIT(P, uint32_t) COMPACT_EMIT(P, uint64_t)
COMPACT_SOURCE(uint8_t)
COMPACT_SOURCE(uint32_t)
COMPACT_SOURCE(uint64_t)
#undef COMPACT_SOURCE
#undef COMPACT_EMIT
#undef COMPACT_COUNT
