// reduce_kernels.inc -- the instantiations of reduce_kernels.hpp (reduce stage of reduce_runs / reduce_by_key), compiled in a
// translation unit of their own (kernels_reduce.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip, explicit
// instantiation in kernels_reduce.hip.  Per (key width, value width): wrapping sum (signed and unsigned share it), float sum, max on
// codes (min, and the value's kind, at run time).
#define RED_CARRY(W, OP)                                                                                                              \
    X(void adlhip::reduce_carry_kernel<W, OP>(unsigned int*, unsigned int const*, W const*, W*, unsigned int, unsigned int*))
#define RED_PAIR(K, W, OP)                                                                                                            \
    X(void adlhip::reduce_partial_kernel<K, W, OP>(K const*, W const*, unsigned int, unsigned int, unsigned int, adlhip::RedCodec,    \
                                                   unsigned int*, unsigned int*, W*))                                                 \
    X(void adlhip::reduce_emit_kernel<K, W, OP>(K const*, W const*, unsigned int, unsigned int, unsigned int, adlhip::RedCodec,       \
                                                unsigned int const*, W const*, K*, W*, unsigned int*))
#define RED_OPS(M, ...) M(__VA_ARGS__, adlhip::kRedSum) M(__VA_ARGS__, adlhip::kRedFloatSum) M(__VA_ARGS__, adlhip::kRedMax)
RED_OPS(RED_CARRY, uint32_t)
RED_OPS(RED_CARRY, uint64_t)
RED_OPS(RED_PAIR, uint32_t, uint32_t)
RED_OPS(RED_PAIR, uint32_t, uint64_t)
RED_OPS(RED_PAIR, uint64_t, uint32_t)
RED_OPS(RED_PAIR, uint64_t, uint64_t)
#undef RED_OPS
#undef RED_PAIR
#undef RED_CARRY
