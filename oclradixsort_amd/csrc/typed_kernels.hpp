// typed_kernels.hpp -- signed, floating-point and descending keys on top of the unsigned ascending sorts
// (adlhip_key_encode / _decode, adlhip_sort_keys_typed / _pairs_typed, adlhip_argsort_typed).  No reference counterpart: the
// reference sorts u32 bit patterns, ascending (Tahoe/ParallelPrimitives/Pprims.h:38-41).
//
// The codec is an order-preserving bijection between a typed key and an unsigned key of the same width, in integer
// instructions only:
//   unsigned     identity
//   signed       flip the sign bit
//   float        bits ^ (sign set ? all ones : sign bit) -- IEEE-754 totalOrder:
//                -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN (NaNs among themselves by payload)
//   descending   complement of the above: a stable ascending sort of complemented keys is a stable descending sort
// Decoding is the exact inverse, so every bit pattern round-trips (NaN payloads, -0).
//
// Keys-only sorts encode in place, sort, decode in place: two streaming sweeps.  Pairs and argsort pay no sweep: they sort
// {32 encoded key bits, source index} pairs like soa_wide_kernels.hpp, and the codec sits inside the pack, repack and gather
// kernels that path runs anyway.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "soa_wide_kernels.hpp"

namespace adlhip {

// KIND: ADLHIP_KEY_* % 3
constexpr int kKeyUnsigned = 0, kKeySigned = 1, kKeyFloat = 2;

template <typename U, int KIND, int DESC>
__host__ __device__ __forceinline__ U key_enc(U b)
{
    using S = typename std::make_signed<U>::type;
    constexpr int W = 8 * (int)sizeof(U);
    constexpr U SIGN = (U)1 << (W - 1);
    if (KIND == kKeySigned) b ^= SIGN;
    if (KIND == kKeyFloat) b ^= (U)((S)b >> (W - 1)) | SIGN;
    return DESC ? (U)~b : b;
}

template <typename U, int KIND, int DESC>
__host__ __device__ __forceinline__ U key_dec(U e)
{
    using S = typename std::make_signed<U>::type;
    constexpr int W = 8 * (int)sizeof(U);
    constexpr U SIGN = (U)1 << (W - 1);
    if (DESC) e = (U)~e;
    if (KIND == kKeySigned) e ^= SIGN;
    if (KIND == kKeyFloat) e ^= (U)((S)(U)~e >> (W - 1)) | SIGN;   // encoded positives carry the sign bit
    return e;
}

template <typename U>
struct alignas(16) KeyVec {
    U v[16 / sizeof(U)];
};

// dst[i] = enc(src[i]) (DECODE: dec) for i < n: 16-byte loads and stores on the body, the n % (16 / sizeof(U)) keys behind
// it one by one.  dst may equal src (every thread writes what it alone has read); both are 16-byte aligned.
template <typename U, int KIND, int DESC, int DECODE>
__global__ __launch_bounds__(kSoaNT) void key_codec_kernel(U* dst, const U* src, size_t n)
{
    constexpr size_t PER = 16 / sizeof(U);
    const size_t nvec = n / PER;
    const size_t stride = (size_t)gridDim.x * kSoaNT;
    const KeyVec<U>* vs = reinterpret_cast<const KeyVec<U>*>(src);
    KeyVec<U>* vd = reinterpret_cast<KeyVec<U>*>(dst);
    auto code = [](KeyVec<U> x) {
#pragma unroll
        for (size_t k = 0; k < PER; ++k) x.v[k] = DECODE ? key_dec<U, KIND, DESC>(x.v[k]) : key_enc<U, KIND, DESC>(x.v[k]);
        return x;
    };
    size_t i = (size_t)blockIdx.x * kSoaNT + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {   // four loads in flight per thread, as the copy probe has
        const KeyVec<U> a = vs[i], b = vs[i + stride], c = vs[i + 2 * stride], e = vs[i + 3 * stride];
        vd[i] = code(a); vd[i + stride] = code(b); vd[i + 2 * stride] = code(c); vd[i + 3 * stride] = code(e);
    }
    for (; i < nvec; i += stride) vd[i] = code(vs[i]);
    if (blockIdx.x == 0) {
        const size_t i = nvec * PER + threadIdx.x;
        if (threadIdx.x < PER && i < n) dst[i] = DECODE ? key_dec<U, KIND, DESC>(src[i]) : key_enc<U, KIND, DESC>(src[i]);
    }
}

// pairs[i] = {low dword of enc(keys[i]), i}
template <typename U, int KIND, int DESC>
__global__ __launch_bounds__(kSoaNT) void typed_pack_index_kernel(const U* __restrict__ keys, uint64_t* __restrict__ pairs, uint32_t n)
{
    const uint32_t stride = gridDim.x * (uint32_t)kSoaNT;
    for (uint32_t i = blockIdx.x * (uint32_t)kSoaNT + threadIdx.x; i < n; i += stride)
        __builtin_nontemporal_store((uint64_t)(uint32_t)key_enc<U, KIND, DESC>(keys[i]) | ((uint64_t)i << 32), pairs + i);
}

// second round of 8-byte keys: out[j] = {high dword of enc(keys[idx]), idx}, idx = the index in[j] carries
template <int KIND, int DESC>
__global__ __launch_bounds__(kSoaNT) void typed_repack_high_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ in,
                                                                   uint64_t* __restrict__ out, uint32_t n)
{
    const uint32_t stride = gridDim.x * (uint32_t)kSoaNT;
    for (uint32_t j = blockIdx.x * (uint32_t)kSoaNT + threadIdx.x; j < n; j += stride) {
        const uint32_t idx = (uint32_t)(__builtin_nontemporal_load(in + j) >> 32);
        out[j] = (key_enc<uint64_t, KIND, DESC>(keys[idx]) >> 32) | ((uint64_t)idx << 32);
    }
}

// keys_out[j] = the key of the pair's index idx_j -- 4-byte keys: dec(the pair's own low dword), keys_in is not read; 8-byte keys:
// keys_in[idx_j] (KIND, DESC unused) --, vals_out[j] = vals_in[idx_j], index_out[j] = idx_j; each where the pointer is given
template <typename U, typename V, int KIND, int DESC>
__global__ __launch_bounds__(kSoaNT) void typed_gather_kernel(const uint64_t* __restrict__ pairs, const U* __restrict__ keys_in,
                                                              U* __restrict__ keys_out, const V* __restrict__ vals_in,
                                                              V* __restrict__ vals_out, uint32_t* __restrict__ index_out, uint32_t n)
{
    const uint32_t stride = gridDim.x * (uint32_t)kSoaNT;
    for (uint32_t j = blockIdx.x * (uint32_t)kSoaNT + threadIdx.x; j < n; j += stride) {
        const uint64_t p = __builtin_nontemporal_load(pairs + j);
        const uint32_t idx = (uint32_t)(p >> 32);
        if (keys_out) {
            if constexpr (sizeof(U) == 4) keys_out[j] = key_dec<uint32_t, KIND, DESC>((uint32_t)p);
            else keys_out[j] = keys_in[idx];
        }
        if (vals_out) vals_out[j] = vals_in[idx];
        if (index_out) index_out[j] = idx;
    }
}

}  // namespace adlhip
