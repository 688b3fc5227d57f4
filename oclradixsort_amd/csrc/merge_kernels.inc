// merge_kernels.inc -- the instantiations of merge_kernels.hpp (adlhip_merge_typed), compiled in a translation unit of their own
// (kernels_merge.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip, explicit instantiation in
// kernels_merge.hip.  Per key width: one partition kernel, and one tile kernel per width of the values (none, 4, 8 bytes).  The
// key's kind and the order are run-time arguments.
#define MERGE_PARTITION(K) \
    X(void adlhip::merge_partition_kernel<K>(K const*, unsigned int, K const*, unsigned int, adlhip::RedCodec, unsigned int, unsigned int*))
#define MERGE_TILES(K, V)                                                                                                          \
    X(void adlhip::merge_tiles_kernel<K, V>(K const*, V const*, unsigned int, K const*, V const*, unsigned int, adlhip::RedCodec, \
                                            unsigned int const*, unsigned int, K*, V*, unsigned int*))
#define MERGE_KEY(K) MERGE_PARTITION(K) MERGE_TILES(K, adlhip::MergeNone) MERGE_TILES(K, uint32_t) MERGE_TILES(K, uint64_t)
MERGE_KEY(uint32_t)
MERGE_KEY(uint64_t)
#undef MERGE_KEY
#undef MERGE_TILES
#undef MERGE_PARTITION
