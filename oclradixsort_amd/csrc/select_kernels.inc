// select_kernels.inc -- the instantiations of select_kernels.hpp (top-k selection), compiled in a translation unit of their own
// (kernels_select.hip) beside primitives.hip.  X(signature): `extern template` in primitives.hip, explicit instantiation in kernels_select.hip.
#define SEL_TYPED(U, KIND, DESC)                                                                                                      \
    X(void adlhip::select_hist_kernel<U, KIND, DESC>(U const*, unsigned int, adlhip::SelState*, adlhip::SelDigit))                    \
    X(void adlhip::select_filter_kernel<U, KIND, DESC, 1>(U const*, unsigned int const*, U*, unsigned int*, unsigned int*,           \
                                                          adlhip::SelState*, unsigned int, unsigned int, unsigned int, adlhip::SelDigit, \
                                                          adlhip::SelDigit))
#define SEL_WIDTH(U)                                                                                                                  \
    SEL_TYPED(U, 0, 0) SEL_TYPED(U, 0, 1) SEL_TYPED(U, 1, 0) SEL_TYPED(U, 1, 1) SEL_TYPED(U, 2, 0) SEL_TYPED(U, 2, 1)                 \
    X(void adlhip::select_filter_kernel<U, 0, 0, 0>(U const*, unsigned int const*, U*, unsigned int*, unsigned int*, adlhip::SelState*, \
                                                    unsigned int, unsigned int, unsigned int, adlhip::SelDigit, adlhip::SelDigit))   \
    X(void adlhip::select_gather_kernel<U>(U const*, unsigned int const*, U*, unsigned int))
SEL_WIDTH(uint32_t)
SEL_WIDTH(uint64_t)
#undef SEL_WIDTH
#undef SEL_TYPED
