// merge_kernels.hpp -- the stable merge of two sorted sequences of typed keys (adlhip_merge_typed): keys, optionally a value per key
// and the element's position in the concatenation A || B.  No reference counterpart.  It is a merge path: the output is cut into
// tiles along diagonals of the (A, B) grid, so that every tile reads one range of A and one range of B and writes one range of the
// output.
//
// The order is that of the typed sorts: unsigned comparison of enc(key) = red_enc<K, kRedMax>(key, {kind, descending}), which is
// key_enc of typed_kernels.hpp with the kind and the order at run time.  Where codes are equal A goes first, so the output is what
// the stable typed sort gives for A || B.
//
//   merge_partition_kernel  thread t = 0 .. tiles: on the diagonal d = min(t * kRedTile, na + nb) a binary search for the number of
//                           elements of A among the first d outputs                                              -> split[t]
//   merge_tiles_kernel      persistent grid, workgroup w takes tiles w, w + grid, ...: the tile's share of A and of B goes to LDS as
//                           codes (thread t loads slots t, t + 256, ...: coalesced at any element offset, which is why the inputs
//                           need no more than their element's alignment); every thread finds the diagonal of its kRedItems = 8
//                           consecutive outputs by the same search in LDS and merges them serially, keeping {code, slot in the
//                           tile's LDS image}; the tile is put in output order in LDS -- codes and 16-bit slots, a thread's 8 of
//                           each as 16-byte words -- and stored densely, thread t the elements t, t + 256, ... (as
//                           compact_kernels.hpp does, and for its reason).  Keys are decoded on the way out
//                           (enc is a bijection: every bit pattern comes back), values are fetched from global memory by slot --
//                           two ascending streams -- and the position is computed from the slot
//
// A launch reads only what EARLIER launches wrote: no workgroup waits on another, no atomics to global memory, nothing
// data-dependent reaches the host.
//
// BOUNDS, for ANY contents of A and B (sorted or not).  Write n = na + nb, T = kRedTile, d_t = min(t T, n).
//  (1) The search on diagonal d keeps lo <= hi inside [L, H] = [max(0, d - nb), min(d, na)], and L <= H because d <= na + nb.  A step
//      reads A[mid] and B[d - 1 - mid] with lo <= mid < hi: mid < H <= na, and d - 1 - mid >= d - H >= 0, d - 1 - mid <= d - 1 - L
//      <= nb - 1.  It ends with lo == hi, so split[t] lies in [L, H] whatever the comparisons answered.  Every split[0 .. tiles] is
//      written by the partition launch before the tile launch reads it: the work buffer's contents on entry never matter.
//  (2) Tile t takes a_lo = split[t], s = split[t + 1], a_hi = min(max(s, a_lo), a_lo + T), b_lo = d_t - a_lo, b_hi = d_{t+1} - a_hi.
//      a_lo <= a_hi <= a_lo + T by the clamp.  a_hi <= na: s <= na and a_lo <= na by (1), and the min only lowers.  b_lo lies in
//      [0, nb] because a_lo lies in [d_t - nb, d_t].  b_hi <= nb: max(s, a_lo) >= s >= d_{t+1} - nb, and a_lo + T >= d_t - nb + T
//      >= d_{t+1} - nb.  b_hi >= b_lo, that is a_hi - a_lo <= d_{t+1} - d_t: in a full tile the right side is T; the last tile has
//      d_{t+1} = n, so s = na exactly (its range is one point) and a_hi - a_lo <= na - a_lo <= na - (d_t - nb) = n - d_t.
//      So a_cnt = a_hi - a_lo and b_cnt = b_hi - b_lo are both in [0, T], a_cnt + b_cnt = d_{t+1} - d_t = the tile's element count,
//      and every global read of the tile is of A[a_lo + i], i < a_cnt, or B[b_lo + i], i < b_cnt: inside [A, A + na) and
//      [B, B + nb).  For sorted inputs the clamp changes nothing (split is then monotone with steps of at most d_{t+1} - d_t).
//  (3) Inside the tile the thread's search is (1) again with (a_cnt, b_cnt, the LDS image) for (na, nb, A and B), so it reads LDS
//      slots below a_cnt + b_cnt only; the serial merge reads a slot only after comparing its index with a_cnt or b_cnt, and a
//      thread's outputs dd + e < cnt always find an element left on one side at least (ai + bi = dd + e < a_cnt + b_cnt).
//      A kept slot is therefore < cnt, and the value and position derived from it are those of an element of (2).
//  (4) Every global write is to element d_t + i of an output with i < cnt, so below n.  On unsorted inputs the threads' ranges need
//      not fit together -- some elements may appear twice, others not at all -- but that changes WHAT is written, never WHERE.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "reduce_kernels.hpp"

namespace adlhip {

struct MergeNone {};   // V of a tile kernel that carries no values

// the number of elements of A among the first d of the merge of (A: na codes through codeA(i)) and (B: nb codes through codeB(i));
// ties take A first.  d <= na + nb.  See BOUNDS (1)
template <typename FA, typename FB>
__device__ __forceinline__ uint32_t merge_diagonal(uint32_t d, uint32_t na, uint32_t nb, FA codeA, FB codeB)
{
    uint32_t lo = d > nb ? d - nb : 0u;
    uint32_t hi = d < na ? d : na;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (codeB(d - 1u - mid) < codeA(mid)) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

__device__ __forceinline__ uint32_t merge_diag_of_tile(uint32_t t, uint32_t n)
{
    const uint64_t d = (uint64_t)t * (uint64_t)kRedTile;
    return d < (uint64_t)n ? (uint32_t)d : n;
}

// split[t] for t = 0 .. tiles; a and b need only their element's alignment and may be the same array
template <typename K>
__global__ __launch_bounds__(kSelNT) void merge_partition_kernel(const K* a, uint32_t na, const K* b, uint32_t nb, RedCodec codec, uint32_t tiles,
                                                                 uint32_t* __restrict__ split)
{
    const uint32_t t = blockIdx.x * (uint32_t)kSelNT + threadIdx.x;
    if (t > tiles) return;
    const uint32_t d = merge_diag_of_tile(t, na + nb);
    split[t] = merge_diagonal(d, na, nb, [&](uint32_t i) { return red_enc<K, kRedMax>(a[i], codec); },
                              [&](uint32_t i) { return red_enc<K, kRedMax>(b[i], codec); });
}

// keys_out, vals_out (V not MergeNone) and index_out are written where given, na + nb elements each; they are 16-byte aligned and
// overlap no input.  a, b, va, vb need only their element's alignment.
template <typename K, typename V>
__global__ __launch_bounds__(kSelNT) void merge_tiles_kernel(const K* a, const V* va, uint32_t na, const K* b, const V* vb, uint32_t nb,
                                                             RedCodec codec, const uint32_t* __restrict__ split, uint32_t tiles,
                                                             K* __restrict__ keys_out, V* __restrict__ vals_out,
                                                             uint32_t* __restrict__ index_out)
{
    constexpr bool has_vals = !std::is_same<V, MergeNone>::value;
    static_assert(kRedTile <= 65536 && kRedItems == 8, "a slot fits 16 bits; a thread's 8 slots are one 16-byte word");
    __shared__ __attribute__((aligned(16))) K s_code[kRedTile];
    __shared__ __attribute__((aligned(16))) uint16_t s_slot[kRedTile];
    const uint32_t n = na + nb;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t d0 = merge_diag_of_tile(tile, n), d1 = merge_diag_of_tile(tile + 1u, n);
        const uint32_t a_lo = split[tile], s1 = split[tile + 1u];
        const uint32_t a_cap = na - a_lo < (uint32_t)kRedTile ? na : a_lo + (uint32_t)kRedTile;   // min(na, a_lo + T) without a wrap
        const uint32_t a_max = s1 > a_lo ? s1 : a_lo;
        const uint32_t a_hi = a_max < a_cap ? a_max : a_cap;   // (s1 <= na: the same as min(max(s1, a_lo), a_lo + T))
        const uint32_t b_lo = d0 - a_lo, b_hi = d1 - a_hi;
        const uint32_t a_cnt = a_hi - a_lo, b_cnt = b_hi - b_lo, cnt = d1 - d0;   // BOUNDS (2): a_cnt + b_cnt == cnt <= kRedTile
        __syncthreads();   // the stage may still be read from the tile before
        for (uint32_t i = threadIdx.x; i < cnt; i += (uint32_t)kSelNT)
            s_code[i] = red_enc<K, kRedMax>(i < a_cnt ? a[a_lo + i] : b[b_lo + (i - a_cnt)], codec);
        __syncthreads();
        const uint32_t dd = threadIdx.x * (uint32_t)kRedItems < cnt ? threadIdx.x * (uint32_t)kRedItems : cnt;
        uint32_t ai = merge_diagonal(dd, a_cnt, b_cnt, [&](uint32_t i) { return s_code[i]; }, [&](uint32_t i) { return s_code[a_cnt + i]; });
        uint32_t bi = dd - ai;
        K c[kRedItems];
        uint32_t s[kRedItems];
        K ka = ai < a_cnt ? s_code[ai] : (K)0, kb = bi < b_cnt ? s_code[a_cnt + bi] : (K)0;
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            const bool take_a = bi >= b_cnt || (ai < a_cnt && !(kb < ka));   // a tie takes A
            c[e] = take_a ? ka : kb;
            s[e] = take_a ? ai : a_cnt + bi;
            if (take_a) {
                ++ai;
                ka = ai < a_cnt ? s_code[ai] : (K)0;
            } else {
                ++bi;
                kb = bi < b_cnt ? s_code[a_cnt + bi] : (K)0;
            }
        }
        __syncthreads();   // every thread has read what it needs of the input image
        const uint32_t o0 = threadIdx.x * (uint32_t)kRedItems;
        if (o0 + (uint32_t)kRedItems <= cnt) {
            // a whole thread (all of them but in the last tile): its 8 codes and 8 slots are 16-byte aligned runs of LDS, stored
            // with 16-byte writes -- element by element the threads' stride of 8 elements puts 32 lanes on 4 banks
#pragma unroll
            for (int e = 0; e < kRedItems; ++e) {
                s_code[o0 + (uint32_t)e] = c[e];
                s_slot[o0 + (uint32_t)e] = (uint16_t)s[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < kRedItems; ++e) {
                if (dd + (uint32_t)e < cnt) {
                    s_code[dd + (uint32_t)e] = c[e];
                    s_slot[dd + (uint32_t)e] = (uint16_t)s[e];
                }
            }
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < cnt; i += (uint32_t)kSelNT) {
            const uint32_t slot = s_slot[i];        // < cnt: BOUNDS (3)
            const bool from_a = slot < a_cnt;
            const uint32_t src = from_a ? a_lo + slot : b_lo + (slot - a_cnt);
            if (keys_out) keys_out[d0 + i] = red_dec<K, kRedMax>(s_code[i], codec);
            if constexpr (has_vals) vals_out[d0 + i] = from_a ? va[src] : vb[src];
            if (index_out) index_out[d0 + i] = from_a ? src : na + src;
        }
    }
}

}  // namespace adlhip
