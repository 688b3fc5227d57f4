// compact_kernels.hpp -- stream compaction (adlhip_compact_flagged / adlhip_compact_if_typed): the selected elements of an array, in
// input order, and optionally the rejected ones behind them (a stable partition).  No reference counterpart.  It is the run stage of
// unique_kernels.hpp with the caller's predicate in the place of "is a run head".
//
// Element i is selected when flags[i] != 0 (P = uint8_t), or when key_enc(keys[i]) cmp key_enc(threshold) as unsigned numbers (P =
// uint32_t / uint64_t; the key's kind and cmp at run time, the threshold's code computed on the host).
//
//   compact_count_kernel  workgroup w counts the selected elements of its chunk             -> chunk_count[w]
//   scan_single_kernel    (radix_kernels.hpp) one workgroup: exclusive scan of the chunk counts in place, the total S -> the caller's word
//   compact_emit_kernel   workgroup w walks its chunk again, tile by tile, with a running base that starts at chunk_count[w]: a
//                         workgroup scan of the threads' counts ranks every element; the r-th selected element goes to out[r], with
//                         `partition` the element at position j with s selected ones in front of it goes to out[S + j - s] (S is read
//                         from the caller's word, which the launch before wrote).  The tile is put in rank order in LDS first --
//                         its selected elements, then its rejected ones -- and stored from there in dense order
//
// The tile is the reduce stage's: kRedTile = 2048 ELEMENTS whatever the widths, kRedItems = 8 consecutive elements per thread, so that
// flags, 4- and 8-byte keys, items and values share one geometry and a thread ranks its own items without an exchange.  A thread's 8
// flags are one 8-byte load; its keys, items and values come with red_load's 16-byte loads.  The selected elements of a tile form one
// dense range of the output, its rejected ones another: the tile is staged in LDS in that order (at most 2048 x (8 + 8 + 4) bytes) and
// thread t stores elements t, t + 256, ..., so a wave's store instruction covers 256 or 512 contiguous bytes.  Storing straight from
// the registers, where a wave's instruction is scattered over up to 512 ranks, was measured and lost by up to 1.8 x.
// A chunk is a contiguous range of whole tiles, split on the host as in unique_kernels.hpp.  A launch reads only what EARLIER launches
// wrote: no workgroup waits on another, no atomics to global memory, nothing data-dependent reaches the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "reduce_kernels.hpp"

namespace adlhip {

struct CompactNone {};   // V of an emit kernel that carries no second array
constexpr uint32_t kCmpLT = 0, kCmpLE = 1, kCmpGT = 2, kCmpGE = 3, kCmpEQ = 4, kCmpNE = 5;   // ADLHIP_CMP_*

// the comparison of the if form: the key's kind (kKey*), cmp (kCmp*), the threshold's code; unused by the flagged form
struct CompactPred {
    uint32_t kind, cmp;
    uint64_t threshold;
};

// the number of this thread's items of one tile (elements first .. first + cnt - 1); x = the items where P is a key type; bit e of
// *sel: item e is selected
template <typename P>
__device__ __forceinline__ uint32_t compact_load_pred(const P* __restrict__ pred, uint32_t n, size_t first, const CompactPred pr,
                                                      P (&x)[kRedItems], uint32_t* sel)
{
    const uint32_t cnt = first >= (size_t)n ? 0u : ((size_t)n - first < (size_t)kRedItems ? (uint32_t)((size_t)n - first) : (uint32_t)kRedItems);
    uint32_t s = 0;
    if constexpr (sizeof(P) == 1) {
        static_assert(kRedItems == 8, "a thread's flags are one 8-byte word");
        if (cnt == (uint32_t)kRedItems) {
            const uint64_t w = *reinterpret_cast<const uint64_t*>(pred + first);   // (first is a multiple of 8, pred 16-byte aligned)
#pragma unroll
            for (int e = 0; e < kRedItems; ++e) s |= (((w >> (8 * e)) & 0xffu) ? 1u : 0u) << e;
        } else {
#pragma unroll
            for (int e = 0; e < kRedItems; ++e) s |= ((uint32_t)e < cnt && pred[first + e] ? 1u : 0u) << e;
        }
    } else {
        red_load<P>(pred, first, cnt, x);
        const RedCodec codec = {pr.kind, 0u};
        const P t = (P)pr.threshold;
        const bool want_lt = pr.cmp == kCmpLT || pr.cmp == kCmpLE || pr.cmp == kCmpNE;
        const bool want_eq = pr.cmp == kCmpLE || pr.cmp == kCmpGE || pr.cmp == kCmpEQ;
        const bool want_gt = pr.cmp == kCmpGT || pr.cmp == kCmpGE || pr.cmp == kCmpNE;
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            const P c = red_enc<P, kRedMax>(x[e], codec);
            const bool in = c < t ? want_lt : (c == t ? want_eq : want_gt);
            s |= ((uint32_t)e < cnt && in ? 1u : 0u) << e;
        }
    }
    *sel = s;
    return cnt;
}

// chunk_count[blockIdx.x] = the selected elements among this workgroup's tiles.  pred is 16-byte aligned.
template <typename P>
__global__ __launch_bounds__(kSelNT) void compact_count_kernel(const P* __restrict__ pred, uint32_t n, uint32_t tiles, uint32_t tiles_per_wg,
                                                               CompactPred pr, uint32_t* __restrict__ chunk_count)
{
    __shared__ uint32_t s_wave[kSelNT / 64];
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    uint32_t mine = 0;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const size_t first = (size_t)tile * kRedTile + (size_t)threadIdx.x * kRedItems;
        P x[kRedItems];
        uint32_t sel;
        (void)compact_load_pred<P>(pred, n, first, pr, x, &sel);
        mine += (uint32_t)__popc(sel);
    }
    uint32_t total;
    (void)sel_block_scan(mine, s_wave, &total);
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
}

// chunk_base[w] = the selected elements in front of workgroup w's chunk (the scanned counts); *num_selected = S.  pred_out (P a key
// type: the keys themselves), vals_out (V not CompactNone: vals[i] travels with element i) and index_out (the element's position)
// are written where given.  Without `partition` nothing at S and beyond is written; with it every element of every given output is.
// pred, vals and the outputs are 16-byte aligned.
template <typename P, typename V>
__global__ __launch_bounds__(kSelNT) void compact_emit_kernel(const P* __restrict__ pred, const V* __restrict__ vals, uint32_t n, uint32_t tiles,
                                                              uint32_t tiles_per_wg, CompactPred pr, const uint32_t* __restrict__ chunk_base,
                                                              const uint32_t* __restrict__ num_selected, uint32_t partition,
                                                              P* __restrict__ pred_out, V* __restrict__ vals_out,
                                                              uint32_t* __restrict__ index_out)
{
    constexpr bool has_vals = !std::is_same<V, CompactNone>::value;
    using VV = typename std::conditional<has_vals, V, uint32_t>::type;
    __shared__ uint32_t s_wave[kSelNT / 64];
    __shared__ P s_keys[sizeof(P) != 1 ? kRedTile : 1];
    __shared__ VV s_vals[has_vals ? kRedTile : 1];
    __shared__ uint32_t s_idx[kRedTile];
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    const uint32_t total_sel = *num_selected < n ? *num_selected : n;   // (never more than n)
    uint32_t base = chunk_base[blockIdx.x];   // selected elements in front of the current tile
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const size_t first = (size_t)tile * kRedTile + (size_t)threadIdx.x * kRedItems;
        P x[kRedItems];
        VV v[kRedItems];
        uint32_t sel;
        const uint32_t cnt = compact_load_pred<P>(pred, n, first, pr, x, &sel);
        if constexpr (has_vals) {
            if (vals_out) red_load<V>(vals, first, cnt, v);
        }
        const uint32_t mine = (uint32_t)__popc(sel);
        uint32_t total;
        const uint32_t incl = sel_block_scan(mine, s_wave, &total);
        uint32_t ls = incl - mine;                                  // selected in front of this thread's item 0, inside the tile
        const uint32_t tile_first = tile * (uint32_t)kRedTile;
        const uint32_t tile_cnt = (n - tile_first) < (uint32_t)kRedTile ? (n - tile_first) : (uint32_t)kRedTile;
        __syncthreads();                                            // the stage may still be read from the tile before
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            if ((uint32_t)e >= cnt) continue;
            const bool in = (sel >> e) & 1u;
            const uint32_t lj = threadIdx.x * (uint32_t)kRedItems + (uint32_t)e;
            const uint32_t slot = in ? ls : total + (lj - ls);
            ls += in ? 1u : 0u;
            if constexpr (sizeof(P) != 1) s_keys[slot] = x[e];
            if constexpr (has_vals) s_vals[slot] = v[e];
            s_idx[slot] = tile_first + lj;
        }
        __syncthreads();
        const uint32_t lim = partition ? tile_cnt : total;
        const uint32_t rej0 = total_sel + (tile_first - base);      // where this tile's rejected elements start
        for (uint32_t i = threadIdx.x; i < lim; i += (uint32_t)kSelNT) {
            const uint32_t dst = i < total ? base + i : rej0 + (i - total);
            if (dst < n) {
                if constexpr (sizeof(P) != 1) {
                    if (pred_out) pred_out[dst] = s_keys[i];
                }
                if constexpr (has_vals) {
                    if (vals_out) vals_out[dst] = s_vals[i];
                }
                if (index_out) index_out[dst] = s_idx[i];
            }
        }
        base += total;
    }
}

}  // namespace adlhip
