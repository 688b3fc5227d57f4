// join_kernels.hpp -- the expansion of runs (adlhip_expand_runs: run-length decode, torch.repeat_interleave, thrust's "expand") and
// the join of two sorted sequences of typed keys built on it (adlhip_join_sorted_typed: inner, left, semi and anti join, as pairs of
// positions).  No reference counterpart.
//
// The expansion turns n counts into T = their sum rows: row o belongs to the element i with start[i] <= o < start[i] + count[i],
// start = the exclusive scan of the counts.  It is a merge path (merge_kernels.hpp) of the n starts with the R = min(T, cap) row numbers
// 0 .. R - 1, an element in front of a row where start[i] <= o: in that merged order the owner of a row is the last element in front
// of it.  Tiles of kRedTile = 2048 ITEMS of the merged order -- elements plus rows -- bound the LDS and the work of a tile whatever the
// counts: ten thousand elements without a row are five tiles of elements alone, one element with a million rows is 489 tiles of rows
// alone that each read one start.
//
// The join's counts come from two sorted searches of every element of A in B (search_kernels.hpp, both sides from one LDS table):
// lo = the codes of B below A[i]'s, hi = those below or equal, m = hi > lo ? hi - lo : 0 its matches; `kind` turns m into the rows of
// A[i], and a row of A[i] is (i, lo + rank), or (i, kJoinNone) where the element has no match and still a row.
//
//   join_bounds_kernel      workgroup w takes a chunk of whole tiles of A, thread t the elements t, t + 256, ... of a tile (coalesced
//                           at any element offset): lo and hi of each, 8 searches side by side          -> base[i], count[i], chunk_total[w]
//   expand_sum_kernel       (adlhip_expand_runs instead of the above) the sum of a chunk's counts                  -> chunk_total[w]
//   expand_scan_kernel      one workgroup: the exclusive scan of the 64-bit chunk totals in place, the total T -> the caller's word
//   expand_starts_kernel    the same chunks: start[i] = min(chunk_total[w] + the counts in front of i in the chunk, cap), in place
//                           over the join's counts.  Saturating at cap keeps what follows in 32 bits: a row below cap is owned by an
//                           element whose start is below cap, so exact
//   expand_partition_kernel thread t: the elements among the first min(t * kRedTile, n + R) items                       -> split[t]
//   expand_rows_kernel      workgroup w walks its chunk of tiles: the tile's starts go to LDS, every thread finds the diagonal of its
//                           8 items and walks them, a row notes the number of the tile's elements in front of it (16 bits, 0 = the
//                           element in front of the tile); then thread t stores rows t, t + 256, ... densely: the owner, the rank
//                           o - start[owner] (plus base[owner] for the join), the owner's value
//
// A launch reads only what EARLIER launches wrote: no workgroup waits on another, no atomics to global memory, nothing
// data-dependent reaches the host.  The grids depend on n (na), nb and cap alone: the row kernel's is sized for n + cap items, and
// its tiles beyond n + R are empty.
//
// BOUNDS, for ANY contents of A, B and the counts (sorted or not).  Write n for the elements (na, num_runs), R = min(T, cap).
//  (1) join_bounds_kernel reads A[i] only for i < na; its searches are search_bounds: BOUNDS (0) .. (3) of search_kernels.hpp keep
//      every read of B inside [B, B + nb) and lo, hi in [0, nb].  m is CLAMPED to hi > lo ? hi - lo : 0, so lo + m <= nb whatever
//      the comparisons answered.  base[i] is lo or kJoinNone, count[i] is m, or 0 or 1 where kind says so; both are written for
//      i < na only.
//  (2) start[] is the library's own exclusive scan of count[], saturated at cap: non-decreasing, start[0] = 0, every read and write
//      of it at an index below n.  (The scan is exact in 64 bits: n < 2^32 counts below 2^32.)
//  (3) expand_partition_kernel and a tile's geometry are (1) and (2) of merge_kernels.hpp with (n, R) for (na, nb): split[t] lies in
//      [max(0, d_t - R), min(d_t, n)], a tile reads start[a_lo + i], i < a_cnt <= kRedTile, a_lo + a_cnt <= n, and holds the rows
//      b_lo .. b_lo + b_cnt - 1 with b_lo + b_cnt <= R.  The thread's search and walk are (3) there: LDS slots below a_cnt only.
//  (4) A row o of the tile is below R <= cap, and it is the only place o is written: rows at cap or beyond, and at T or beyond,
//      are never written.  Its owner is g - 1 with g = a_lo + (the tile's elements in front of it) in [1, n] -- g >= 1 because
//      start[0] = 0 <= o puts element 0 in front of every row, and the code lowers g = 0 to owner 0 regardless -- so the owner is
//      below n: every written run_out / index_a is below n, and vals_in, base[] are read below n.
//  (5) rank = o - start[owner].  start[owner] <= o < cap, so it is unsaturated and exact; the next element's start is above o (it
//      is behind the row in the merged order), and it is min(start[owner] + count[owner], cap), or the owner is the last element
//      and o < T: either way rank < count[owner].  For the join that is rank < m, so base + rank < lo + m <= nb by (1): every written
//      index_b is below nb, or it is kJoinNone (base == kJoinNone is passed on as it is, never added to).
//  (6) Every loop has a fixed trip count, halves a range or walks a chunk of tiles; what the comparisons answer changes values,
//      never an address outside (1) .. (5).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "merge_kernels.hpp"
#include "search_kernels.hpp"

#ifndef ADLHIP_KERNEL
#define ADLHIP_KERNEL
#endif

namespace adlhip {

constexpr uint32_t kJoinInner = 0, kJoinLeft = 1, kJoinSemi = 2, kJoinAnti = 3;   // ADLHIP_JOIN_*
constexpr uint32_t kJoinNone = 0xFFFFFFFFu;                                        // ADLHIP_JOIN_NONE
// the table of B in LDS: 16 KiB whatever the key width (4096 or 2048 codes), so that 8 workgroups share a CU's LDS
constexpr uint32_t kJoinTableBytes = 16384;

// inclusive sum of v over the workgroup's threads in thread order; *total = the sum over all of them.  Every thread calls it.
// (sel_block_scan in 64 bits)
__device__ __forceinline__ uint64_t expand_block_scan(uint64_t v, uint64_t* s_wave, uint64_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(v, o);
        if (lane >= (uint32_t)o) v += t;
    }
    __syncthreads();   // s_wave may still be read from the call before
    if (lane == 63u) s_wave[w] = v;
    __syncthreads();
    uint64_t add = 0, sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kSelNT / 64; ++j) {
        const uint64_t t = s_wave[j];
        if (j < w) add += t;
        sum += t;
    }
    *total = sum;
    return v + add;
}

// base_out[i], count_out[i] for i < na and chunk_total[blockIdx.x] = the rows of this workgroup's tiles.  a and b need only their
// element's alignment and may overlap.  Dynamic LDS: sa.samples codes, rounded up to 16 bytes (at most kJoinTableBytes).  BOUNDS (1)
template <typename U>
__global__ __launch_bounds__(kSelNT) void join_bounds_kernel(const U* a, uint32_t na, const U* b, SearchArgs sa, RedCodec codec, uint32_t kind,
                                                            uint32_t tiles, uint32_t tiles_per_wg, uint32_t* __restrict__ base_out,
                                                            uint32_t* __restrict__ count_out, uint64_t* __restrict__ chunk_total)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_join[];
    __shared__ uint64_t s_wave[kSelNT / 64];
    U* s_tab = reinterpret_cast<U*>(s_join);
    search_table_load<U>(s_tab, b, sa, codec);
    __syncthreads();
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    uint64_t mine = 0;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const size_t first = (size_t)tile * kRedTile + (size_t)threadIdx.x;
        U x[kRedItems];
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            const size_t i = first + (size_t)e * kSelNT;
            x[e] = i < (size_t)na ? red_enc<U, kRedMax>(a[i], codec) : (U)0;   // (a slot behind A searches for nothing and is dropped)
        }
        uint32_t lo[kRedItems], hi[kRedItems];
        search_bounds<U, kSearchLeft>(s_tab, b, sa, codec, x, lo);
        search_bounds<U, kSearchRight>(s_tab, b, sa, codec, x, hi);
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            const size_t i = first + (size_t)e * kSelNT;
            if (i >= (size_t)na) continue;
            const uint32_t m = hi[e] > lo[e] ? hi[e] - lo[e] : 0u;   // the clamp of BOUNDS (1)
            uint32_t rows = m, base = lo[e];
            if (kind == kJoinLeft) {
                rows = m ? m : 1u;
                base = m ? lo[e] : kJoinNone;
            } else if (kind == kJoinSemi) {
                rows = m ? 1u : 0u;
            } else if (kind == kJoinAnti) {
                rows = m ? 0u : 1u;
                base = kJoinNone;
            }
            base_out[i] = base;
            count_out[i] = rows;
            mine += rows;
        }
    }
    uint64_t total;
    (void)expand_block_scan(mine, s_wave, &total);
    if (threadIdx.x == 0) chunk_total[blockIdx.x] = total;
}

// chunk_total[blockIdx.x] = the sum of the counts of this workgroup's tiles; counts needs only 4-byte alignment
ADLHIP_KERNEL __global__ __launch_bounds__(kSelNT) void expand_sum_kernel(const uint32_t* __restrict__ counts, uint32_t n, uint32_t tiles,
                                                                          uint32_t tiles_per_wg, uint64_t* __restrict__ chunk_total)
{
    __shared__ uint64_t s_wave[kSelNT / 64];
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    uint64_t mine = 0;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const size_t first = (size_t)tile * kRedTile + (size_t)threadIdx.x;
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            const size_t i = first + (size_t)e * kSelNT;
            if (i < (size_t)n) mine += counts[i];
        }
    }
    uint64_t total;
    (void)expand_block_scan(mine, s_wave, &total);
    if (threadIdx.x == 0) chunk_total[blockIdx.x] = total;
}

// one workgroup: chunk_total[0 .. wgs) becomes its exclusive scan, *num_out = T
ADLHIP_KERNEL __global__ __launch_bounds__(kSelNT) void expand_scan_kernel(uint64_t* __restrict__ chunk_total, uint32_t wgs, uint64_t* __restrict__ num_out)
{
    __shared__ uint64_t s_wave[kSelNT / 64];
    uint64_t carry = 0;
    for (uint32_t first = 0; first < wgs; first += (uint32_t)kSelNT) {
        const uint32_t i = first + threadIdx.x;
        const uint64_t v = i < wgs ? chunk_total[i] : 0u;
        uint64_t total;
        const uint64_t inc = expand_block_scan(v, s_wave, &total);
        if (i < wgs) chunk_total[i] = carry + inc - v;
        carry += total;
    }
    if (threadIdx.x == 0) *num_out = carry;
}

// start[i] = min(chunk_base[w] + the counts in front of i in workgroup w's chunk, cap).  counts needs only 4-byte alignment and may
// BE start (the join's counts are scanned in place): a tile's counts are all in LDS before its first start is written, and no other
// tile or workgroup touches its elements.  start is 16-byte aligned.  BOUNDS (2)
ADLHIP_KERNEL __global__ __launch_bounds__(kSelNT) void expand_starts_kernel(const uint32_t* counts, uint32_t n, uint32_t cap, uint32_t tiles,
                                                                             uint32_t tiles_per_wg, const uint64_t* __restrict__ chunk_base,
                                                                             uint32_t* start)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[kRedTile];
    __shared__ uint64_t s_wave[kSelNT / 64];
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    uint64_t carry = chunk_base[blockIdx.x];
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const size_t tile0 = (size_t)tile * kRedTile;
        __syncthreads();   // s_cnt may still be read from the tile before
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            const uint32_t l = threadIdx.x + (uint32_t)e * kSelNT;
            s_cnt[l] = tile0 + l < (size_t)n ? counts[tile0 + l] : 0u;
        }
        __syncthreads();
        uint32_t c[kRedItems];
        red_load<uint32_t>(s_cnt, (size_t)threadIdx.x * kRedItems, (uint32_t)kRedItems, c);
        uint64_t mine = 0;
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) mine += c[e];
        uint64_t total;
        uint64_t run = carry + expand_block_scan(mine, s_wave, &total) - mine;   // the rows in front of this thread's first element
        uint32_t s[kRedItems];
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            s[e] = run < (uint64_t)cap ? (uint32_t)run : cap;
            run += c[e];
        }
        const size_t first = tile0 + (size_t)threadIdx.x * kRedItems;
        if (first + kRedItems <= (size_t)n) {
#pragma unroll
            for (int u = 0; u < kRedItems / 4; ++u) {
                RedVec<uint32_t> t;
#pragma unroll
                for (int e = 0; e < 4; ++e) t.v[e] = s[u * 4 + e];
                *reinterpret_cast<RedVec<uint32_t>*>(start + first + u * 4) = t;
            }
        } else {
#pragma unroll
            for (int e = 0; e < kRedItems; ++e)
                if (first + e < (size_t)n) start[first + e] = s[e];
        }
        carry += total;
    }
}

// split[t] for t = 0 .. tiles: the elements among the first min(t * kRedTile, n + R) items of the merged order of the n starts and
// the rows 0 .. R - 1, R = min(*total, cap); an element goes first where start[i] <= o.  BOUNDS (3)
ADLHIP_KERNEL __global__ __launch_bounds__(kSelNT) void expand_partition_kernel(const uint32_t* __restrict__ start, uint32_t n,
                                                                                const uint64_t* __restrict__ total, uint32_t cap, uint32_t tiles,
                                                                                uint32_t* __restrict__ split)
{
    const uint32_t t = blockIdx.x * (uint32_t)kSelNT + threadIdx.x;
    if (t > tiles) return;
    const uint64_t T = *total;
    const uint32_t R = T < (uint64_t)cap ? (uint32_t)T : cap;
    const uint32_t d = merge_diag_of_tile(t, n + R);
    split[t] = merge_diagonal(d, n, R, [&](uint32_t i) { return start[i]; }, [&](uint32_t o) { return o; });
}

// The rows below R = min(*total, cap) of whichever outputs are given: run_out[o] = the owner, rank_out[o] = o - start[owner], plus
// base_in[owner] where base_in is given (kJoinNone is passed on as it is), vals_out[o] = vals_in[owner] (V not MergeNone).  The
// outputs are 16-byte aligned and overlap nothing; vals_in needs only its element's alignment.  BOUNDS (3) .. (5)
template <typename V>
__global__ __launch_bounds__(kSelNT) void expand_rows_kernel(const uint32_t* __restrict__ start, uint32_t n, const uint64_t* __restrict__ total,
                                                            uint32_t cap, const uint32_t* __restrict__ split, uint32_t tiles, uint32_t tiles_per_wg,
                                                            const uint32_t* __restrict__ base_in, const V* __restrict__ vals_in,
                                                            uint32_t* __restrict__ run_out, uint32_t* __restrict__ rank_out, V* __restrict__ vals_out)
{
    constexpr bool has_vals = !std::is_same<V, MergeNone>::value;
    static_assert(kRedTile < 65536 && kRedItems == 8, "the elements of a tile in front of a row fit 16 bits");
    __shared__ __attribute__((aligned(16))) uint32_t s_start[kRedTile];
    __shared__ __attribute__((aligned(16))) uint16_t s_own[kRedTile];
    __shared__ uint32_t s_front;
    const uint64_t T = *total;
    const uint32_t R = T < (uint64_t)cap ? (uint32_t)T : cap;
    const uint32_t items = n + R;
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const uint32_t d0 = merge_diag_of_tile(tile, items), d1 = merge_diag_of_tile(tile + 1u, items);
        if (d0 == d1) break;   // (the grid is sized for n + cap items: the tiles behind n + R are empty, and so are all that follow)
        const uint32_t a_lo = split[tile], s1 = split[tile + 1u];
        const uint32_t a_cap = n - a_lo < (uint32_t)kRedTile ? n : a_lo + (uint32_t)kRedTile;
        const uint32_t a_max = s1 > a_lo ? s1 : a_lo;
        const uint32_t a_hi = a_max < a_cap ? a_max : a_cap;
        const uint32_t b_lo = d0 - a_lo, b_hi = d1 - a_hi;
        const uint32_t a_cnt = a_hi - a_lo, b_cnt = b_hi - b_lo, cnt = d1 - d0;   // BOUNDS (3): a_cnt + b_cnt == cnt <= kRedTile
        __syncthreads();   // the image may still be read from the tile before
        for (uint32_t i = threadIdx.x; i < a_cnt; i += (uint32_t)kSelNT) s_start[i] = start[a_lo + i];
        if (threadIdx.x == 0) s_front = a_lo ? start[a_lo - 1u] : 0u;   // the start of the element that owns the tile's first rows
        __syncthreads();
        const uint32_t dd = threadIdx.x * (uint32_t)kRedItems < cnt ? threadIdx.x * (uint32_t)kRedItems : cnt;
        uint32_t ai = merge_diagonal(dd, a_cnt, b_cnt, [&](uint32_t i) { return s_start[i]; }, [&](uint32_t j) { return b_lo + j; });
        uint32_t bi = dd - ai;
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            if (dd + (uint32_t)e < cnt) {
                const bool take_a = bi >= b_cnt || (ai < a_cnt && !(b_lo + bi < s_start[ai]));   // a tie takes the element
                if (take_a) {
                    ++ai;
                } else {
                    s_own[bi] = (uint16_t)ai;   // bi < b_cnt; ai <= a_cnt
                    ++bi;
                }
            }
        }
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < b_cnt; j += (uint32_t)kSelNT) {
            const uint32_t o = b_lo + j;   // < R: BOUNDS (4)
            const uint32_t l = s_own[j];
            const uint32_t g = a_lo + l;
            const uint32_t owner = g ? g - 1u : 0u;
            const uint32_t rank = o - (l ? s_start[l - 1u] : s_front);
            if (run_out) run_out[o] = owner;
            if (rank_out) {
                uint32_t r = rank;
                if (base_in) {
                    const uint32_t base = base_in[owner];
                    r = base == kJoinNone ? kJoinNone : base + rank;   // BOUNDS (5)
                }
                rank_out[o] = r;
            }
            if constexpr (has_vals) vals_out[o] = vals_in[owner];
        }
    }
}

}  // namespace adlhip
