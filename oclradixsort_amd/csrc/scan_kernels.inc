// scan_kernels.inc -- the instantiations of scan_kernels.hpp (scan stage of scan_typed / scan_by_key), compiled in a translation unit
// of their own (kernels_scan.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip, explicit instantiation in
// kernels_scan.hip.  Per (no key / key width, value width): wrapping sum (signed and unsigned share it), float sum, max on codes (min,
// and the value's kind, at run time).  The keyed partial kernel and the carry kernel are those of reduce_kernels.inc.
#define SCAN_PARTIAL(W, OP)                                                                                                           \
    X(void adlhip::scan_partial_kernel<W, OP>(W const*, unsigned int, unsigned int, unsigned int, adlhip::RedCodec, unsigned int*,    \
                                              unsigned int*, W*))
#define SCAN_EMIT(K, W, OP)                                                                                                           \
    X(void adlhip::scan_emit_kernel<K, W, OP>(K const*, W const*, unsigned int, unsigned int, unsigned int, adlhip::RedCodec,         \
                                              unsigned int const*, W const*, W const*, unsigned int, W, W*))
#define SCAN_OPS(M, ...) M(__VA_ARGS__, adlhip::kRedSum) M(__VA_ARGS__, adlhip::kRedFloatSum) M(__VA_ARGS__, adlhip::kRedMax)
SCAN_OPS(SCAN_PARTIAL, uint32_t)
SCAN_OPS(SCAN_PARTIAL, uint64_t)
SCAN_OPS(SCAN_EMIT, adlhip::ScanNoKey, uint32_t)
SCAN_OPS(SCAN_EMIT, adlhip::ScanNoKey, uint64_t)
SCAN_OPS(SCAN_EMIT, uint32_t, uint32_t)
SCAN_OPS(SCAN_EMIT, uint32_t, uint64_t)
SCAN_OPS(SCAN_EMIT, uint64_t, uint32_t)
SCAN_OPS(SCAN_EMIT, uint64_t, uint64_t)
#undef SCAN_OPS
#undef SCAN_EMIT
#undef SCAN_PARTIAL
