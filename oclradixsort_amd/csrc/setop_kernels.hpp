// setop_kernels.hpp -- set operations on two sorted sequences of typed keys (adlhip_set_op_typed): thrust's set_intersection,
// set_union, set_difference and set_symmetric_difference with their multiset semantics, keys, optionally a value per key and the
// element's position in A || B.  No reference counterpart.  The result is a subsequence of the stable merge (merge_kernels.hpp), so
// it is the merge path with a keep bit per element and the count / scan / emit pattern of compact_kernels.hpp around it.
//
// For a key x that occurs m times in A and n times in B, and an element's rank r inside its own input's run of x:
//   an element of A is kept by intersection when r < n, by difference and symmetric difference when r >= n, by union always;
//   an element of B is kept by union and symmetric difference when r >= m, never otherwise.
// Both tests are one look at the other input.  Take an element of A with code x, `ai` elements of A and `bi` of B in front of it
// in the merge.  Ties take A, so the bi elements of B are exactly those below x: B's run of x starts at bi, and r < n says no more
// than B[bi + r] == x.  Take an element of B, `ai` of A in front of it: they are exactly the elements of A at or below x, A's run of
// x ends at ai, and r < m says A[ai - 1 - r] == x.  What is left to find is r, that is the start of the element's run in its OWN
// input.  Inside a tile's share that is carried along the serial merge (a run starts where the code changes); a thread searches the
// LDS image only for the run its first element of A and of B continue, and only when the element before has the same code.  A run
// that reaches the front of the share may start in an earlier tile: one thread per input looks at the element in front of the share
// and, where it has the same code, searches [0, a_lo) or [0, b_lo) of global memory.  The look at the other input stays in the LDS
// image where the position falls into the tile's share, and is a global read otherwise (long runs only).
//
//   merge_partition_kernel  (merge_kernels.hpp) the split per boundary of the kRedTile-element tiles of the merged order -> split[t]
//   setop_count_kernel      workgroup w walks its chunk of whole tiles: the merge of merge_tiles_kernel, the keep bits, their
//                           number                                                                         -> chunk_count[w]
//   scan_single_kernel      (radix_kernels.hpp) exclusive scan of the chunk counts in place, the total S -> the caller's word
//   setop_emit_kernel       the same walk with a running base that starts at chunk_count[w]: a workgroup scan of the threads'
//                           counts ranks the kept elements, their {code, 16-bit slot} go to LDS in rank order and are stored
//                           densely, thread t the elements t, t + 256, ...; keys are decoded on the way out, values fetched from
//                           global memory by slot, the position computed from the slot -- as the merge does
//
// A launch reads only what EARLIER launches wrote: no workgroup waits on another, no atomics to global memory, nothing
// data-dependent reaches the host.
//
// BOUNDS, for ANY contents of A and B (sorted or not); (1) .. (3) are those of merge_kernels.hpp, whose geometry, searches and serial
// merge are repeated here unchanged.
//  (4) setop_run_front reads A[a_lo - 1] only when a_lo > 0 and then searches [0, a_lo - 1): every index is below a_lo <= na; its
//      result lies in [0, a_lo].  The same for B.
//  (5) setop_local_start searches the share's slots [0, pos) and returns l <= pos, so the run start -- s_front (4) where l == 0,
//      lo + l otherwise -- is at most lo + pos, and r = lo + pos - start lies in [0, lo + pos] <= [0, na] (or nb): no wrap.  A run
//      start carried along the walk is an index the walk has passed, with the same bound.
//  (6) The look at B is at p = b_lo + bi + r, read only when p < nb: from LDS where p - b_lo < b_cnt (a slot of the share), from
//      b[p] otherwise.  p cannot wrap: b_lo + bi <= nb, r <= na, na + nb < 2^32.  The look at A is at p = a_lo + ai - 1 - r, read
//      only when a_lo + ai > r, so 0 <= p < a_lo + ai <= a_hi <= na: from LDS where p >= a_lo (slot p - a_lo < ai <= a_cnt).
//  (7) Every loop has a fixed trip count or halves a range; what the comparisons answer changes the keep bits, never an address
//      outside (4) .. (6).  The emit kernel writes element base + i of an output only when that is below `cap` (na or na + nb, the
//      capacity the contract gives every output), and lowers the count word to cap where the total exceeds it.  For sorted inputs
//      neither ever happens: the kept elements are a subsequence of na (intersection, difference) or na + nb elements.  On unsorted
//      inputs the tiles' shares of A can overlap (a non-monotone split), which is why the clamp is there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "merge_kernels.hpp"

namespace adlhip {

constexpr uint32_t kSetIntersection = 0, kSetUnion = 1, kSetDifference = 2, kSetSymmetricDifference = 3;   // ADLHIP_SETOP_*

// the geometry of a tile: BOUNDS (2) of merge_kernels.hpp
struct SetopTile {
    uint32_t d0, cnt, a_lo, b_lo, a_cnt, b_cnt;
};

// the start of the run of the share's first code in its whole input: x = enc(in[lo]); BOUNDS (4)
template <typename K>
__device__ __forceinline__ uint32_t setop_run_front(const K* in, uint32_t lo, const RedCodec codec)
{
    if (lo == 0u) return 0u;
    const K x = red_enc<K, kRedMax>(in[lo], codec);
    if (red_enc<K, kRedMax>(in[lo - 1u], codec) != x) return lo;
    uint32_t l = 0u, h = lo - 1u;
    while (l < h) {
        const uint32_t mid = l + ((h - l) >> 1);
        if (red_enc<K, kRedMax>(in[mid], codec) < x) l = mid + 1u;
        else h = mid;
    }
    return l;
}

// the first slot of s[0 .. pos] that holds s[pos]'s code, for a sorted s; at most pos.  BOUNDS (5)
template <typename K>
__device__ __forceinline__ uint32_t setop_local_start(const K* s, uint32_t pos)
{
    if (pos == 0u || s[pos - 1u] != s[pos]) return pos;
    const K x = s[pos];
    uint32_t l = 0u, h = pos - 1u;
    while (l < h) {
        const uint32_t mid = l + ((h - l) >> 1);
        if (s[mid] < x) l = mid + 1u;
        else h = mid;
    }
    return l;
}

// One tile: its shares of A and B to LDS as codes, this thread's kRedItems outputs of the merge (c: code, s: slot in the LDS image,
// below g->a_cnt for an element of A) and the keep bits of `op` (bit e: output e belongs to the result).  Every thread calls it; it
// starts with a barrier, and the caller must pass one before it overwrites s_code.
template <typename K>
__device__ __forceinline__ uint32_t setop_tile_keep(const K* a, uint32_t na, const K* b, uint32_t nb, const RedCodec codec,
                                                    const uint32_t* __restrict__ split, uint32_t tile, uint32_t op, K* s_code,
                                                    uint32_t* s_front, K (&c)[kRedItems], uint32_t (&s)[kRedItems], SetopTile* g)
{
    const uint32_t n = na + nb;
    const uint32_t d0 = merge_diag_of_tile(tile, n), d1 = merge_diag_of_tile(tile + 1u, n);
    const uint32_t a_lo = split[tile], s1 = split[tile + 1u];
    const uint32_t a_cap = na - a_lo < (uint32_t)kRedTile ? na : a_lo + (uint32_t)kRedTile;
    const uint32_t a_max = s1 > a_lo ? s1 : a_lo;
    const uint32_t a_hi = a_max < a_cap ? a_max : a_cap;
    const uint32_t b_lo = d0 - a_lo, b_hi = d1 - a_hi;
    const uint32_t a_cnt = a_hi - a_lo, b_cnt = b_hi - b_lo, cnt = d1 - d0;
    *g = SetopTile{d0, cnt, a_lo, b_lo, a_cnt, b_cnt};
    __syncthreads();   // the stage and s_front may still be read from the tile before
    for (uint32_t i = threadIdx.x; i < cnt; i += (uint32_t)kSelNT)
        s_code[i] = red_enc<K, kRedMax>(i < a_cnt ? a[a_lo + i] : b[b_lo + (i - a_cnt)], codec);
    const bool look_a = op != kSetUnion;                                   // an element of A needs B
    const bool look_b = op == kSetUnion || op == kSetSymmetricDifference;  // an element of B needs A (it is dropped otherwise)
    // where the runs that reach the front of the shares start, for the inputs whose ranks the operation asks for: one thread of two
    // different waves each
    if (threadIdx.x == 0u && a_cnt && look_a) s_front[0] = setop_run_front<K>(a, a_lo, codec);
    if (threadIdx.x == 64u && b_cnt && look_b) s_front[1] = setop_run_front<K>(b, b_lo, codec);
    __syncthreads();
    const K* sa = s_code;
    const K* sb = s_code + a_cnt;
    const uint32_t dd = threadIdx.x * (uint32_t)kRedItems < cnt ? threadIdx.x * (uint32_t)kRedItems : cnt;
    uint32_t ai = merge_diagonal(dd, a_cnt, b_cnt, [&](uint32_t i) { return sa[i]; }, [&](uint32_t i) { return sb[i]; });
    uint32_t bi = dd - ai;
    // the local starts of the runs the thread's first elements continue; a start of 0 stands for s_front
    uint32_t ra = look_a && ai < a_cnt ? setop_local_start<K>(sa, ai) : ai;
    uint32_t rb = look_b && bi < b_cnt ? setop_local_start<K>(sb, bi) : bi;
    const uint32_t fa = a_cnt && look_a ? s_front[0] : a_lo, fb = b_cnt && look_b ? s_front[1] : b_lo;
    K ka = ai < a_cnt ? sa[ai] : (K)0, kb = bi < b_cnt ? sb[bi] : (K)0;
    uint32_t keep = 0u;
#pragma unroll
    for (int e = 0; e < kRedItems; ++e) {
        const bool take_a = bi >= b_cnt || (ai < a_cnt && !(kb < ka));   // a tie takes A
        const bool live = dd + (uint32_t)e < cnt;
        bool k;
        if (take_a) {
            c[e] = ka;
            s[e] = ai;
            k = true;
            if (look_a && live) {
                const uint32_t r = a_lo + ai - (ra ? a_lo + ra : fa);   // BOUNDS (5)
                const uint32_t p = b_lo + bi + r;                        // BOUNDS (6)
                bool in_b = false;
                if (p < nb) in_b = (p - b_lo < b_cnt ? sb[p - b_lo] : red_enc<K, kRedMax>(b[p], codec)) == ka;
                k = op == kSetIntersection ? in_b : !in_b;
            }
            ++ai;
            const K next = ai < a_cnt ? sa[ai] : (K)0;
            if (next != ka) ra = ai;
            ka = next;
        } else {
            c[e] = kb;
            s[e] = a_cnt + bi;
            k = false;
            if (look_b && live) {
                const uint32_t r = b_lo + bi - (rb ? b_lo + rb : fb);
                const uint32_t top = a_lo + ai;                          // the end of A's run of kb
                bool in_a = false;
                if (top > r) {
                    const uint32_t p = top - 1u - r;
                    in_a = (p >= a_lo ? sa[p - a_lo] : red_enc<K, kRedMax>(a[p], codec)) == kb;
                }
                k = !in_a;
            }
            ++bi;
            const K next = bi < b_cnt ? sb[bi] : (K)0;
            if (next != kb) rb = bi;
            kb = next;
        }
        keep |= (k && live ? 1u : 0u) << e;
    }
    return keep;
}

// chunk_count[blockIdx.x] = the kept elements among this workgroup's tiles
template <typename K>
__global__ __launch_bounds__(kSelNT) void setop_count_kernel(const K* a, uint32_t na, const K* b, uint32_t nb, RedCodec codec, uint32_t op,
                                                             const uint32_t* __restrict__ split, uint32_t tiles, uint32_t tiles_per_wg,
                                                             uint32_t* __restrict__ chunk_count)
{
    __shared__ __attribute__((aligned(16))) K s_code[kRedTile];
    __shared__ uint32_t s_front[2];
    __shared__ uint32_t s_wave[kSelNT / 64];
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    uint32_t mine = 0;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        K c[kRedItems];
        uint32_t s[kRedItems];
        SetopTile g;
        mine += (uint32_t)__popc(setop_tile_keep<K>(a, na, b, nb, codec, split, tile, op, s_code, s_front, c, s, &g));
    }
    uint32_t total;
    (void)sel_block_scan(mine, s_wave, &total);
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
}

// chunk_base[w] = the kept elements in front of workgroup w's chunk (the scanned counts); *num_out = S, lowered to cap here where it
// exceeds it (unsorted inputs only).  keys_out, vals_out (V not MergeNone) and index_out are written where given, elements below
// min(S, cap) only; they are 16-byte aligned and overlap no input.  a, b, va, vb need only their element's alignment.
template <typename K, typename V>
__global__ __launch_bounds__(kSelNT) __attribute__((amdgpu_waves_per_eu(8, 8))) void setop_emit_kernel(const K* a, const V* va, uint32_t na, const K* b, const V* vb, uint32_t nb,
                                                            RedCodec codec, uint32_t op, const uint32_t* __restrict__ split, uint32_t tiles,
                                                            uint32_t tiles_per_wg, const uint32_t* __restrict__ chunk_base, uint32_t cap,
                                                            uint32_t* num_out, K* __restrict__ keys_out, V* __restrict__ vals_out,
                                                            uint32_t* __restrict__ index_out)
{
    constexpr bool has_vals = !std::is_same<V, MergeNone>::value;
    static_assert(kRedTile <= 65536, "a slot fits 16 bits");
    __shared__ __attribute__((aligned(16))) K s_code[kRedTile];
    __shared__ __attribute__((aligned(16))) uint16_t s_slot[kRedTile];
    // the two run fronts and the scan's wave totals live in the last words of s_slot, which the stage may need: with 8-byte keys the
    // two arrays are 20 KiB, exactly what lets 8 workgroups share a CU's LDS as the merge's do
    uint32_t* s_front = reinterpret_cast<uint32_t*>(s_slot + kRedTile) - 2;
    uint32_t* s_wave = s_front - kSelNT / 64;
    if (blockIdx.x == 0 && threadIdx.x == 0 && *num_out > cap) *num_out = cap;   // (no workgroup reads it: BOUNDS (7))
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    uint32_t base = chunk_base[blockIdx.x];   // kept elements in front of the current tile
    for (uint32_t tile = t0; tile < t1; ++tile) {
        K c[kRedItems];
        uint32_t s[kRedItems];
        SetopTile g;
        const uint32_t keep = setop_tile_keep<K>(a, na, b, nb, codec, split, tile, op, s_code, s_front, c, s, &g);
        const uint32_t mine = (uint32_t)__popc(keep);
        uint32_t total;
        uint32_t ls = sel_block_scan(mine, s_wave, &total) - mine;   // (its barriers: every thread has read what it needs of the image)
        __syncthreads();                                             // ... and now of s_wave, which the slots may overwrite
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            if ((keep >> e) & 1u) {
                s_code[ls] = c[e];
                s_slot[ls] = (uint16_t)s[e];
                ++ls;
            }
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < total; i += (uint32_t)kSelNT) {
            const uint32_t dst = base + i;
            if (dst >= cap) break;                  // BOUNDS (7)
            const uint32_t slot = s_slot[i];        // < cnt: BOUNDS (3)
            const bool from_a = slot < g.a_cnt;
            const uint32_t src = from_a ? g.a_lo + slot : g.b_lo + (slot - g.a_cnt);
            if (keys_out) keys_out[dst] = red_dec<K, kRedMax>(s_code[i], codec);
            if constexpr (has_vals) vals_out[dst] = from_a ? va[src] : vb[src];
            if (index_out) index_out[dst] = from_a ? src : na + src;
        }
        base += total;
    }
}

}  // namespace adlhip
