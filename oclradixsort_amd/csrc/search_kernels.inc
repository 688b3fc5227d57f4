// search_kernels.inc -- the instantiations of search_kernels.hpp (adlhip_search_sorted_typed), compiled in a translation unit of their
// own (kernels_search.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip, explicit instantiation in
// kernels_search.hip.  Per key width one kernel per side.  The key's kind and the order are run-time arguments.
#define SEARCH_SORTED(U, SIDE)                                                                                                        \
    X(void adlhip::search_sorted_kernel<U, SIDE>(U const*, adlhip::SearchArgs, U const*, unsigned int, unsigned int, unsigned int, \
                                                 adlhip::RedCodec, unsigned int*))
#define SEARCH_KEY(U) SEARCH_SORTED(U, adlhip::kSearchLeft) SEARCH_SORTED(U, adlhip::kSearchRight)
SEARCH_KEY(uint32_t)
SEARCH_KEY(uint64_t)
#undef SEARCH_KEY
#undef SEARCH_SORTED
