// scan_kernels.hpp -- the scan stage of adlhip_scan_typed / adlhip_scan_by_key: an inclusive or exclusive segmented scan (sum, min,
// max) of values, over the runs of grouped keys or over one segment.  No reference counterpart (Pprims::scan keeps its own kernels).
//
// It is the reduce stage of reduce_kernels.hpp with an emit kernel that writes every element instead of the run tails; the state, the
// operators, the loads, the tile (kRedTile = 2048 elements, kRedItems = 8 per thread) and the chunks of whole tiles are that file's.
//
//   reduce_partial_kernel  (keyed scans; reduce_kernels.hpp)  chunk_flag[w], chunk_agg[w]; its head counts are not used
//   scan_partial_kernel    (the plain scan: no keys, the only head is position 0)  the same two, chunk_agg[w] = the whole chunk
//   reduce_carry_kernel    (reduce_kernels.hpp)  chunk_carry[w]: the aggregate in front of chunk w of the segment open at its start
//   scan_emit_kernel       workgroup w walks its chunk tile by tile with a running carry: the per-thread inclusive segmented scan,
//                          red_block_scan, then every item writes out[i]
//
// inc[i], the inclusive value, is `open ? op(p.a, x[e]) : x[e]` (p: what red_block_scan returns, x[e]: the thread's own inclusive
// scan) -- but for the LAST element of every chunk, which is chunk_flag[w] ? chunk_agg[w] : op(chunk_carry[w], chunk_agg[w]): the
// same value for the exact operators, another association of the same elements for float sums.  That is what lets the exclusive scan
// of chunk w + 1 start from inc of the element in front of it without reading what another workgroup writes: it recomputes it from
// the three words of chunk w.  Inside a chunk the value in front of an item comes from the thread's own registers, from the lane below
// (one shuffle), from the wave below or the tile before (one LDS word per wave).  So the exclusive result is a function of the
// inclusive one: out[i] = init at a head, inc[i - 1] (no init) or op(init, inc[i - 1]) (one operation) elsewhere.
//
// IN PLACE: a thread reads only its own items of vals and writes only its own items of out, after it has read them; what it needs of
// its neighbours travels through registers and LDS; the partial launch has read vals before the emit launch starts.  So out == vals
// (exactly equal, not a partial overlap) works, and neither pointer is __restrict__.  out must not overlap the keys: a thread reads
// the key in front of its items, which belongs to another thread.
//
// As in the reduce stage: validity flags instead of identity elements (a segment's first element comes back bit for bit), float sums
// are plain IEEE adds in an association that depends on n and the grid alone, MIN / MAX work on the order-preserving code; no
// workgroup waits on another, no atomics to global memory, nothing data-dependent reaches the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "reduce_kernels.hpp"

namespace adlhip {

struct ScanNoKey {};   // K of the plain scan
constexpr uint32_t kScanInclusive = 0, kScanExclusive = 1, kScanExclusiveInit = 2;   // `mode` of scan_emit_kernel

// the number of this thread's items of one tile (elements first .. first + cnt - 1); bit e of *heads: item e is a head
template <typename K>
__device__ __forceinline__ uint32_t scan_load_heads(const K* __restrict__ keys, uint32_t n, size_t first, uint32_t* heads)
{
    if constexpr (std::is_same<K, ScanNoKey>::value) {
        const uint32_t cnt = first >= (size_t)n ? 0u : ((size_t)n - first < (size_t)kRedItems ? (uint32_t)((size_t)n - first) : (uint32_t)kRedItems);
        *heads = first == 0 && cnt ? 1u : 0u;
        return cnt;
    } else {
        K k[kRedItems];
        return red_load_keys<K>(keys, n, first, k, heads);
    }
}

// The partial launch of the plain scan: what reduce_partial_kernel writes for keys that are all equal, without loading any.  vals is
// 16-byte aligned.
template <typename W, int OP>
__global__ __launch_bounds__(kSelNT) void scan_partial_kernel(const W* __restrict__ vals, uint32_t n, uint32_t tiles, uint32_t tiles_per_wg,
                                                              RedCodec codec, uint32_t* __restrict__ chunk_heads,
                                                              uint32_t* __restrict__ chunk_flag, W* __restrict__ chunk_agg)
{
    __shared__ RedState<W> s_wave[kSelNT / 64];
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    RedState<W> acc = red_identity<W>();   // this thread's elements; the operators commute, so thread order does not matter
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const size_t first = (size_t)tile * kRedTile + (size_t)threadIdx.x * kRedItems;
        W x[kRedItems];
        uint32_t heads;
        const uint32_t cnt = scan_load_heads<ScanNoKey>(nullptr, n, first, &heads);
        red_load<W>(vals, first, cnt, x);
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            if ((uint32_t)e < cnt) {
                const W c = red_enc<W, OP>(x[e], codec);
                acc.a = acc.v ? red_op<W, OP>(acc.a, c) : c;
                acc.v = 1u;
            }
        }
    }
    RedState<W> total;
    (void)red_block_scan<W, OP>(acc, red_identity<W>(), s_wave, &total);
    if (threadIdx.x == 0) {
        chunk_heads[blockIdx.x] = blockIdx.x == 0 ? 1u : 0u;
        chunk_flag[blockIdx.x] = blockIdx.x == 0 ? 1u : 0u;
        chunk_agg[blockIdx.x] = total.a;   // codes for MIN / MAX (no chunk is empty)
    }
}

// See the head of this file.  keys (unless K is ScanNoKey), vals and out are 16-byte aligned; out may be vals.  init is read in mode
// kScanExclusiveInit alone.
template <typename K, typename W, int OP>
__global__ __launch_bounds__(kSelNT) void scan_emit_kernel(const K* __restrict__ keys, const W* vals, uint32_t n, uint32_t tiles,
                                                           uint32_t tiles_per_wg, RedCodec codec, const uint32_t* __restrict__ chunk_flag,
                                                           const W* __restrict__ chunk_agg, const W* __restrict__ chunk_carry, uint32_t mode,
                                                           W init, W* out)
{
    constexpr int PER = 16 / (int)sizeof(W);
    __shared__ RedState<W> s_wave[kSelNT / 64];
    __shared__ W s_last[kSelNT / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, b = blockIdx.x;
    const uint32_t t0 = b * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    const size_t chunk_end = (size_t)t1 * kRedTile < (size_t)n ? (size_t)t1 * kRedTile : (size_t)n;
    // the elements of this chunk in front of the current tile, behind everything in front of the chunk
    RedState<W> carry;
    carry.f = 0u;
    carry.v = b > 0 ? 1u : 0u;
    carry.cnt = 0u;
    carry.a = b > 0 ? chunk_carry[b] : (W)0;
    // inc of the chunk's last element (chunk 0 holds position 0, so its flag is set), and of the element in front of the chunk
    const W chunk_last = chunk_flag[b] ? chunk_agg[b] : red_op<W, OP>(carry.a, chunk_agg[b]);
    W prev_tile = (W)0;   // inc (a code for MIN / MAX) of the element in front of the current tile
    if (mode != kScanInclusive && b > 0)
        prev_tile = chunk_flag[b - 1] ? chunk_agg[b - 1] : red_op<W, OP>(chunk_carry[b - 1], chunk_agg[b - 1]);
    const W init_code = red_enc<W, OP>(init, codec);
    // what a head gets: the init, or the operator's identity pattern (zero bits for sums; the first pattern in the order of MAX)
    const W head_out = mode == kScanExclusiveInit ? init : red_dec<W, OP>((W)0, codec);
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const size_t first = (size_t)tile * kRedTile + (size_t)threadIdx.x * kRedItems;
        W x[kRedItems];
        uint32_t heads;
        const uint32_t cnt = scan_load_heads<K>(keys, n, first, &heads);
        red_load<W>(vals, first, cnt, x);
        // inclusive segmented scan of this thread's items, in place
        RedState<W> mine = red_identity<W>();
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            if ((uint32_t)e >= cnt) continue;
            const bool head = (heads >> e) & 1u;
            const W c = red_enc<W, OP>(x[e], codec);
            x[e] = (head || !mine.v) ? c : red_op<W, OP>(mine.a, c);
            mine.a = x[e];
            mine.v = 1u;
            mine.f |= head ? 1u : 0u;
        }
        RedState<W> total;
        const RedState<W> p = red_block_scan<W, OP>(mine, carry, s_wave, &total);
        bool open = p.v;   // the segment of the item began in front of this thread, and p.a holds its elements so far
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            if ((uint32_t)e >= cnt) continue;
            if ((heads >> e) & 1u) open = false;
            if (open) x[e] = red_op<W, OP>(p.a, x[e]);
            if (first + e + 1 == chunk_end) x[e] = chunk_last;
        }
        if (mode != kScanInclusive) {
            // x[e] = inc of the element in front of item e.  A thread that holds fewer than kRedItems items is the last one with any.
            const W last = x[kRedItems - 1];
            W prev = __shfl_up(last, 1);
            if (lane == 63u) s_last[wave] = last;   // (the reads of the tile before lie in front of red_block_scan's barriers)
            __syncthreads();
            if (lane == 0u) prev = wave ? s_last[wave - 1] : prev_tile;
            prev_tile = s_last[kSelNT / 64 - 1];
#pragma unroll
            for (int e = kRedItems - 1; e > 0; --e) x[e] = x[e - 1];
            x[0] = prev;
#pragma unroll
            for (int e = 0; e < kRedItems; ++e) {
                const W v = mode == kScanExclusiveInit ? red_op<W, OP>(init_code, x[e]) : x[e];
                x[e] = ((heads >> e) & 1u) ? head_out : red_dec<W, OP>(v, codec);
            }
        } else {
#pragma unroll
            for (int e = 0; e < kRedItems; ++e) x[e] = red_dec<W, OP>(x[e], codec);
        }
        if (cnt == (uint32_t)kRedItems) {
#pragma unroll
            for (int u = 0; u < kRedItems / PER; ++u) {
                RedVec<W> t;
#pragma unroll
                for (int e = 0; e < PER; ++e) t.v[e] = x[u * PER + e];
                *reinterpret_cast<RedVec<W>*>(out + first + u * PER) = t;
            }
        } else {
#pragma unroll
            for (int e = 0; e < kRedItems; ++e)
                if ((uint32_t)e < cnt) out[first + e] = x[e];
        }
        carry = total;
        carry.f = 0u;
    }
}

}  // namespace adlhip
