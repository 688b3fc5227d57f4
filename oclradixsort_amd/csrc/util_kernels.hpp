// util_kernels.hpp -- gfx950 device code of the handle's own entry points (handle.hip): the bandwidth probes, the fills and the key
// generator.  Self-contained: nothing here knows of the sorts, and no sort header includes it.
#pragma once
// non-template kernels: external linkage in the translation unit that launches them (handle.hip)
#ifndef ADLHIP_KERNEL
#define ADLHIP_KERNEL
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adlhip {

// ------------------------------------------------------------------------------------------
// bandwidth probes + fill
// ------------------------------------------------------------------------------------------
ADLHIP_KERNEL __global__ __launch_bounds__(256) void probe_copy_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src,
                                                         size_t nvec)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        uint4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
        dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
    }
    for (; i < nvec; i += stride) dst[i] = src[i];
}

// The same two probes with cache-policy hints: NTL = non-temporal loads, NTS = non-temporal stores (bench.py reports the plain and
// the hinted rates side by side; which one is the honest ceiling for a sweep depends on whether the sweep's data will be read again)
template <bool NTL, bool NTS>
__global__ __launch_bounds__(256) void probe_copy_hint_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t nvec)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u* s = reinterpret_cast<const v4u*>(src);
    v4u* d = reinterpret_cast<v4u*>(dst);
    auto ld = [&](size_t i) -> v4u { return NTL ? __builtin_nontemporal_load(s + i) : s[i]; };
    auto st = [&](size_t i, v4u v) {
        if (NTS) __builtin_nontemporal_store(v, d + i);
        else d[i] = v;
    };
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        const v4u a = ld(i), b = ld(i + stride), c = ld(i + 2 * stride), e = ld(i + 3 * stride);
        st(i, a); st(i + stride, b); st(i + 2 * stride, c); st(i + 3 * stride, e);
    }
    for (; i < nvec; i += stride) st(i, ld(i));
}
template <bool NTL>
__global__ __launch_bounds__(256) void probe_read_hint_kernel(const uint4* __restrict__ src, size_t nvec, unsigned long long* __restrict__ sink)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u* s = reinterpret_cast<const v4u*>(src);
    auto ld = [&](size_t i) -> v4u { return NTL ? __builtin_nontemporal_load(s + i) : s[i]; };
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t acc = 0u;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        const v4u a = ld(i), b = ld(i + stride), c = ld(i + 2 * stride), e = ld(i + 3 * stride);
        acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ e.x ^ e.y ^ e.z ^ e.w;
    }
    for (; i < nvec; i += stride) { const v4u a = ld(i); acc ^= a.x ^ a.y ^ a.z ^ a.w; }
    if (acc == 0x9e3779b9u) atomicAdd(sink, 1ull);   // practically never; keeps the loads alive
}

ADLHIP_KERNEL __global__ __launch_bounds__(256) void probe_read_kernel(const uint4* __restrict__ src, size_t nvec,
                                                         unsigned long long* __restrict__ sink)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t acc = 0u;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        uint4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
        acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ d.x ^ d.y ^ d.z ^ d.w;
    }
    for (; i < nvec; i += stride) { uint4 a = src[i]; acc ^= a.x ^ a.y ^ a.z ^ a.w; }
    if (acc == 0x9e3779b9u) atomicAdd(sink, 1ull);   // practically never; keeps the loads alive
}

ADLHIP_KERNEL __global__ __launch_bounds__(256) void fill_u32_kernel(uint32_t* __restrict__ dst, uint32_t pattern, size_t count)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) dst[i] = pattern;
}

// count copies of a 16-byte pattern (8-byte patterns are doubled by the host: count is then in 16-byte units
// plus an optional 8-byte tail written by thread 0)
ADLHIP_KERNEL __global__ __launch_bounds__(256) void fill_pattern16_kernel(uint4* __restrict__ dst, uint4 pattern, size_t count,
                                                             uint2* __restrict__ tail8, uint2 tail_pattern)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) dst[i] = pattern;
    if (tail8 && blockIdx.x == 0 && threadIdx.x == 0) *tail8 = tail_pattern;
}

// Synthetic inputs, reproducible by index (same function as the oracle's generator).
__device__ __forceinline__ uint64_t splitmix64_at(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// kind: 0 = u32 keys, 1 = {key32, index} pairs, 2 = u64 keys
ADLHIP_KERNEL __global__ __launch_bounds__(256) void generate_keys_kernel(void* __restrict__ dst, size_t n, uint64_t base,
                                                            uint64_t first_index, int kind)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t r = splitmix64_at(base + i);
        if (kind == 0) reinterpret_cast<uint32_t*>(dst)[i] = (uint32_t)(r >> 32);
        else if (kind == 1) reinterpret_cast<uint64_t*>(dst)[i] = (r >> 32) | ((uint64_t)(uint32_t)(first_index + i) << 32);
        else reinterpret_cast<uint64_t*>(dst)[i] = r;
    }
}

}  // namespace adlhip
