// setop_kernels.inc -- the instantiations of setop_kernels.hpp (adlhip_set_op_typed), compiled in a translation unit of their own
// (kernels_setop.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip, explicit instantiation in
// kernels_setop.hip.  Per key width: one count kernel, and one emit kernel per width of the values (none, 4, 8 bytes).  The key's
// kind, the order and the operation are run-time arguments.  (The partition kernel is the merge's: merge_kernels.inc.)
#define SETOP_COUNT(K)                                                                                                          \
    X(void adlhip::setop_count_kernel<K>(K const*, unsigned int, K const*, unsigned int, adlhip::RedCodec, unsigned int,       \
                                         unsigned int const*, unsigned int, unsigned int, unsigned int*))
#define SETOP_EMIT(K, V)                                                                                                         \
    X(void adlhip::setop_emit_kernel<K, V>(K const*, V const*, unsigned int, K const*, V const*, unsigned int, adlhip::RedCodec, \
                                           unsigned int, unsigned int const*, unsigned int, unsigned int, unsigned int const*,   \
                                           unsigned int, unsigned int*, K*, V*, unsigned int*))
#define SETOP_KEY(K) SETOP_COUNT(K) SETOP_EMIT(K, adlhip::MergeNone) SETOP_EMIT(K, uint32_t) SETOP_EMIT(K, uint64_t)
SETOP_KEY(uint32_t)
SETOP_KEY(uint64_t)
#undef SETOP_KEY
#undef SETOP_EMIT
#undef SETOP_COUNT
