// search_kernels.hpp -- the vectorised binary search of typed keys (adlhip_search_sorted_typed): for every needle its lower or upper
// bound in a sorted sequence.  thrust lower_bound / upper_bound, numpy.searchsorted, torch.searchsorted / bucketize.  No reference
// counterpart.
//
// The order is that of the typed sorts: unsigned comparison of enc(key) = red_enc<U, kRedMax>(key, {kind, descending}), as the merge
// and the histogram compare.  LEFT: pos = the number of elements whose code is below the needle's; RIGHT: below or equal.
//
//   search_sorted_kernel  workgroup w takes a chunk of whole tiles of kRedTile = 2048 needles.  Once per workgroup the table goes to
//                         LDS as codes: table[i] = enc(sorted[min((i + 1) * stride, m) - 1]) for i < S = ceil(m / stride), the LAST
//                         element of every block of `stride` elements.  stride = 1 while m <= C (kSearchLdsKeys = 4096, or what
//                         "debug.search_lds_keys" lowers it to): the table is then the sequence itself and the search ends in LDS.
//                         Per tile a thread takes 8 consecutive needles with 16-byte loads (red_load) and keeps the 8 searches side
//                         by side in registers, so every step issues 8 independent reads (the loop of hist_count_kernel; the step
//                         is search_step below).  Level 1 finds j = the number of table entries below (or equal to) the needle:
//                         every block in front of block j ends below the needle, so lies below it wholly; block j ends at or
//                         above it, or j == S.  Level 2 (stride > 1 only) counts inside block j with the same branch-free steps
//                         on global memory, 8 loads in flight per thread and step.  pos = j * stride + that count.  The 8 positions
//                         leave as two 16-byte stores.
//
// C = 4096 codes: 16 KiB of LDS for 4-byte keys (51 VGPRs: 8 workgroups = 8 waves per SIMD, the most a SIMD holds), 32 KiB for 8-byte
// keys (77 VGPRs allow 6 waves per SIMD, the LDS 5 workgroups = 5 waves per SIMD).  Twice the table saves one global step of 12 to
// 26 and would leave the 8-byte kernel 2 waves per SIMD to hide the latency of the others; half the table adds a global step for no
// wave gained by the 4-byte kernel.  The LDS is dynamic and sized for S, so a short sequence does not pay for C.  No scratch.
// Against a plain clamped search over global memory from the top (no table) the table won the one A/B by 1.07 to 1.87 x from 64 Ki
// keys up; the plain form is gone, there is one path per size class and no knob.
//
// One launch.  No workgroup waits on another, no atomics to global memory, nothing data-dependent reaches the host; the grid depends
// on n and m alone.
//
// BOUNDS, for ANY contents of sorted and needles (sorted or not).  Write len1 = S, T = top_s, and for level 2 base, len2, top_g.
//  (0) The host passes stride >= 1, S = ceil(m / stride) <= C (S = 0 exactly when m = 0) and top_s = the largest power of two <= S
//      (0 when S = 0), top_g = the largest power of two <= stride.  Thread i < S gathers sorted[g] with g = m - 1 for i = S - 1
//      and (i + 1) * stride - 1 otherwise; (i + 1) * stride <= (S - 1) * stride < m, so g < m, and the product does not wrap.
//  (1) search_step reads entry min(t, len) - 1 of a table of len >= 1 entries with t = pos + step >= 1: an index in [0, len).  It
//      moves pos to t only when t <= len.  So pos <= len after every step, whatever the comparison answered.  With len = 0 the
//      top step is 0 and no step runs: pos = 0 and nothing is read.  Level 1: j in [0, S], every read an LDS slot below S.
//  (2) Level 2: base = min(j * stride, m) (a 64-bit product), len2 = min(stride, m - base), so base + len2 <= m.  A step reads
//      sorted[g], g = base + min(t, len2) - 1 in 32-bit arithmetic, then lowered to m - 1 when it is not below m: g is CLAMPED to
//      [0, m - 1] explicitly, and m >= 1 here because stride > 1 implies m > C' >= 2.  (Unclamped, g already lies in
//      [base, base + len2 - 1] when len2 >= 1; len2 = 0 means base = m >= 1, and g = m - 1.)  pos2 moves to t only when t <= len2, so
//      pos2 <= len2.
//  (3) pos = base + pos2 <= base + len2 <= m; with stride == 1, pos = j <= S = m.  So every position lies in [0, m].
//  (4) Needles are read by red_load: elements first .. first + cnt - 1 < n only.  Positions are written to the same elements of
//      pos_out: a full thread's 8 as two 16-byte stores, the last thread's cnt < 8 one by one.  Nothing beyond n is written.
//  For a sorted sequence (1) and (2) are the textbook lower / upper bound: the steps from top down add up to 2 * top - 1 >= len.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reduce_kernels.hpp"

namespace adlhip {

constexpr int kSearchLeft = 0, kSearchRight = 1;   // SIDE of the kernel (ADLHIP_SEARCH_LEFT / _RIGHT)
constexpr uint32_t kSearchLdsKeys = 4096;          // C: codes of the table in LDS at most

struct SearchArgs {
    uint32_t m;        // elements of the sequence
    uint32_t stride;   // elements per block (1: the table is the sequence)
    uint32_t samples;  // S: entries of the table
    uint32_t top_s;    // the largest power of two <= S (0: S == 0)
    uint32_t top_g;    // the largest power of two <= stride
};

// One step of the branch-free search for the number of entries of a non-decreasing table of len codes that are <= x (SIDE LEFT: < x):
// pos moves to pos + step when that many entries qualify.  entry(i) is asked for i in [0, len) only; pos <= len stays true.  The
// step of hist_search and of the loop in hist_count_kernel (histogram_kernels.hpp), with the table behind a function.
template <typename U, int SIDE, typename F>
__device__ __forceinline__ uint32_t search_step(F entry, uint32_t len, uint32_t step, U x, uint32_t pos)
{
    const uint32_t t = pos + step;
    const U ev = entry((t < len ? t : len) - 1u);
    const bool below = SIDE == kSearchLeft ? ev < x : ev <= x;
    return (t <= len && below) ? t : pos;
}

// pos[e] = the bound of the code x[e] in sorted[0 .. a.m), the kRedItems searches side by side; s_tab: the table of a.samples codes in
// LDS that search_table_load filled.  BOUNDS (1) .. (3).  The join's bounds kernel (join_kernels.hpp) runs it for both sides.
template <typename U, int SIDE>
__device__ __forceinline__ void search_bounds(const U* s_tab, const U* sorted, const SearchArgs a, const RedCodec codec, const U (&x)[kRedItems],
                                              uint32_t (&pos)[kRedItems])
{
    const uint32_t m = a.m, S = a.samples, stride = a.stride;
#pragma unroll
    for (int e = 0; e < kRedItems; ++e) pos[e] = 0u;
    for (uint32_t step = a.top_s; step; step >>= 1) {   // level 1, the 8 searches side by side: 8 independent LDS reads per step
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) pos[e] = search_step<U, SIDE>([&](uint32_t i) { return s_tab[i]; }, S, step, x[e], pos[e]);
    }
    if (stride > 1u) {   // level 2 inside block pos[e]: 8 independent global loads per step.  BOUNDS (2)
        uint32_t base[kRedItems], len[kRedItems];
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            const uint64_t b = (uint64_t)pos[e] * (uint64_t)stride;
            base[e] = b < (uint64_t)m ? (uint32_t)b : m;
            len[e] = m - base[e] < stride ? m - base[e] : stride;
            pos[e] = 0u;
        }
        for (uint32_t step = a.top_g; step; step >>= 1) {
#pragma unroll
            for (int e = 0; e < kRedItems; ++e)
                pos[e] = search_step<U, SIDE>(
                    [&](uint32_t i) {
                        const uint32_t g = base[e] + i;   // (len 0: i = 2^32 - 1 and g = base - 1 = m - 1)
                        return red_enc<U, kRedMax>(sorted[g < m ? g : m - 1u], codec);   // the clamp: [0, m - 1] whatever came before
                    },
                    len[e], step, x[e], pos[e]);
        }
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) pos[e] += base[e];   // <= base + len <= m.  BOUNDS (3)
    }
}

// the table of the search to LDS: BOUNDS (0).  Every thread calls it; the caller passes a barrier before it searches.
template <typename U>
__device__ __forceinline__ void search_table_load(U* s_tab, const U* sorted, const SearchArgs a, const RedCodec codec)
{
    for (uint32_t i = threadIdx.x; i < a.samples; i += (uint32_t)kSelNT) {
        const uint32_t g = i + 1u < a.samples ? (i + 1u) * a.stride - 1u : a.m - 1u;   // BOUNDS (0)
        s_tab[i] = red_enc<U, kRedMax>(sorted[g], codec);
    }
}

// pos_out[i] = the bound of needles[i] in sorted[0 .. a.m) for every i < n.  needles and pos_out are 16-byte aligned; sorted needs its
// element's alignment only and may overlap needles.  Dynamic LDS: a.samples codes, rounded up to 16 bytes.
template <typename U, int SIDE>
__global__ __launch_bounds__(kSelNT) void search_sorted_kernel(const U* sorted, SearchArgs a, const U* needles, uint32_t n, uint32_t tiles,
                                                              uint32_t tiles_per_wg, RedCodec codec, uint32_t* __restrict__ pos_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_search[];
    U* s_tab = reinterpret_cast<U*>(s_search);
    search_table_load<U>(s_tab, sorted, a, codec);
    __syncthreads();
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const size_t first = (size_t)tile * kRedTile + (size_t)threadIdx.x * kRedItems;
        const uint32_t cnt = first >= (size_t)n ? 0u : ((size_t)n - first < (size_t)kRedItems ? (uint32_t)((size_t)n - first) : (uint32_t)kRedItems);
        U x[kRedItems];
        red_load<U>(needles, first, cnt, x);
        uint32_t pos[kRedItems];
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) x[e] = red_enc<U, kRedMax>(x[e], codec);
        search_bounds<U, SIDE>(s_tab, sorted, a, codec, x, pos);
        if (cnt == (uint32_t)kRedItems) {
#pragma unroll
            for (int u = 0; u < kRedItems / 4; ++u) {
                RedVec<uint32_t> t;
#pragma unroll
                for (int e = 0; e < 4; ++e) t.v[e] = pos[u * 4 + e];
                *reinterpret_cast<RedVec<uint32_t>*>(pos_out + first + u * 4) = t;
            }
        } else {
#pragma unroll
            for (int e = 0; e < kRedItems; ++e)
                if ((uint32_t)e < cnt) pos_out[first + e] = pos[e];
        }
    }
}

}  // namespace adlhip
