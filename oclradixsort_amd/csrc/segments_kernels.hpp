// segments_kernels.hpp -- sort and argsort within variable-length segments of typed keys (adlhip_sort_segments_typed).  No reference
// counterpart.  The contract, per segment s < S with elements [off[s], off[s + 1]): the stable typed argsort of those elements, that is
// their composites (key_enc(key), position inside the segment) in unsigned ascending order.  All composites of a segment are distinct,
// so arrival order in LDS never matters.  It is sortrows_kernels.hpp with the row replaced by a segment of any length.
//
//   the plan        segments_classify_kernel, one thread per segment: len(s) from the clamped offsets, and its class
//                     0       len == 0
//                     k       1 .. 12: the smallest power of two >= len is P = 2^k, at least 2 (len 1 has k = 1)
//                     13      len > kRowCap, which a correct max_segment excludes
//                   It writes (class, s).  The host sorts these pairs stably on 4 bits (adlhip_radix_sort_soa32), which leaves the
//                   segment ids grouped by class and ascending inside every class.  segments_counts_kernel, one workgroup, finds the
//                   14 class starts in the sorted class array by binary search and writes the 14 counts (and the number of class-13
//                   segments to the caller's word).  The ids of class 0 lie in front of the list and are never read again.  No
//                   atomics, no workgroup waits on another.
//   the sort        segments_sort_kernel, one launch.  Every workgroup derives from the counts the tiles of every class: classes
//                   k = 1 .. 12 have ceil(count_k / G_k) tiles of G_k = kRowCap >> k listed segments each, class 13 one tile per
//                   segment.  Workgroups of 256 threads take the tiles of all classes in turns over one concatenated tile index
//                   (blockIdx.x, blockIdx.x + gridDim.x, ...).  A tile of class k is the kRowCap LDS slots of toprows_kernels.hpp
//                   (RowItems<U>): listed segment b of the tile in slots [b P, b P + len_b), the slots up to (b + 1) P padded with the
//                   all-ones composite; slot (b << k) + c is loaded from keys[start_b + c].  The bitonic network of
//                   sort_rows_kernel -- merge phases up to length P only, direction from the index inside the block -- sorts all
//                   blocks at once, and slot (b << k) + c goes to element start_b + c of the outputs.  The blocks behind the last
//                   listed segment of a class's last tile are neither loaded, sorted nor stored.  A tile of class 13 copies its
//                   segment in input order with identity indices.  Every key is read once, every output written once; no atomics
//                   to global memory, no fence, and no workgroup depends on another.
//   the flat path   the flat argsort, the sorted search of every position in the offsets (search_kernels.hpp) and the stable (segment,
//                   position) sort, see primitives.hip; segments_emit_kernel writes the indices and gathers the keys.
//
// BOUNDS, for ANY contents of off[0 .. S] (not ascending, beyond n, anything), n >= 1, S >= 1.
//  (0) seg_span(off, s, n) is asked for s in [0, S - 1] only and reads off[s] and off[s + 1], both inside the S + 1 entries.  It
//      returns lo = min(off[s], n) and len = min(max(off[s + 1], lo), n) - lo: the offset clamped to [previous, n].  So lo <= n,
//      lo + len <= n, whatever the offsets hold.
//  (1) segments_classify_kernel: thread s < S writes cls[s], ids[s]; the class is a pure function of len, in [0, 13].
//  (2) segments_counts_kernel searches cls[0 .. S) with indices clamped to [0, S - 1] (seg_class_start) and writes counts[0 .. 13] and
//      the caller's word.  Every start lies in [0, S] and they ascend because they are lower bounds of ascending targets in one array
//      by one procedure -- and where the array is not sorted (it always is: the library wrote it) the kernel still orders them, start_k =
//      max(start_k, start_(k - 1)), so every count is in [0, S] and the counts add up to at most S.
//  (3) segments_sort_kernel: a tile of class k, 1 <= k <= 12, lists entries j0 + b of ids with j0 + b < start_k + count_k <= S, reads
//      each id and clamps it to [0, S - 1], takes its span by (0) and lowers len to P = 2^k (a no-op when the plan classified it).
//      Slot (b << k) + c with b < g <= G_k, c < P is below kRowCap.  It reads keys[lo + c] and writes element lo + c of the outputs
//      only for c < len, and lo + len <= n.  A tile of class 13 does the same over c < len without the LDS tile.
//      The tile count ceil(c / G_k) is computed as (c + G_k - 1) >> (12 - k) in 32 bits: it relies on the host's limit S <= kMaxElems =
//      0xFFF00000 (the entry refuses more), which keeps c + 2047 below 2^32.
//  (4) segments_emit_kernel: thread j < n reads pos[j] and seg[j], both lowered to n - 1 and S - 1; it reads keys[p], off[s] and
//      writes element j of the outputs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "toprows_kernels.hpp"

namespace adlhip {

constexpr int kSegClasses = 14;                      // 0: empty, 1 .. 12: P = 2^k, 13: longer than kRowCap
constexpr int kSegMaxBlocks = kRowCap >> 1;          // listed segments of a tile at most (class 1)
constexpr int kSegIndexLocal = 0, kSegIndexGlobal = 1;   // ADLHIP_SEGMENT_INDEX_*
static_assert(kRowCap == 1 << (kSegClasses - 2), "class 12 fills the tile");

struct SegSpan {
    uint32_t lo, len;
};

// BOUNDS (0)
__device__ __forceinline__ SegSpan seg_span(const uint32_t* __restrict__ off, uint32_t s, uint32_t n)
{
    const uint32_t a = off[s], b = off[s + 1u];
    const uint32_t lo = a < n ? a : n;
    const uint32_t hi0 = b > lo ? b : lo;
    const uint32_t hi = hi0 < n ? hi0 : n;
    return SegSpan{lo, hi - lo};
}

__device__ __forceinline__ uint32_t seg_class(uint32_t len)
{
    if (len == 0u) return 0u;
    if (len > (uint32_t)kRowCap) return (uint32_t)kSegClasses - 1u;
    uint32_t k = 1u;
    while ((1u << k) < len) ++k;
    return k;
}

// cls[s] = the class of segment s, ids[s] = s
ADLHIP_KERNEL __global__ __launch_bounds__(kSelNT) void segments_classify_kernel(const uint32_t* __restrict__ off, uint32_t S, uint32_t n,
                                                                                 uint32_t* __restrict__ cls, uint32_t* __restrict__ ids)
{
    const size_t stride = (size_t)gridDim.x * kSelNT;
    for (size_t s = (size_t)blockIdx.x * kSelNT + threadIdx.x; s < (size_t)S; s += stride) {
        cls[s] = seg_class(seg_span(off, (uint32_t)s, n).len);
        ids[s] = (uint32_t)s;
    }
}

// the number of entries of cls[0 .. S) below k, for an ascending cls; every index read lies in [0, S - 1].  BOUNDS (2)
__device__ __forceinline__ uint32_t seg_class_start(const uint32_t* __restrict__ cls, uint32_t S, uint32_t k)
{
    uint32_t lo = 0u, hi = S;   // cls[i] < k for i < lo, cls[i] >= k for i >= hi
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);   // lo <= mid < hi <= S
        if (cls[mid] < k) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// counts[k] = the number of segments of class k, from the sorted class array; *oversized = counts[13].  One workgroup.
ADLHIP_KERNEL __global__ __launch_bounds__(64) void segments_counts_kernel(const uint32_t* __restrict__ cls, uint32_t S,
                                                                           uint32_t* __restrict__ counts, uint32_t* __restrict__ oversized)
{
    __shared__ uint32_t s_start[kSegClasses + 1];
    const uint32_t k = threadIdx.x;
    if (k <= (uint32_t)kSegClasses) s_start[k] = k == (uint32_t)kSegClasses ? S : seg_class_start(cls, S, k);
    __syncthreads();
    if (k == 0u) {   // ascending whatever the array held
        for (int c = 1; c <= kSegClasses; ++c)
            if (s_start[c] < s_start[c - 1]) s_start[c] = s_start[c - 1];
    }
    __syncthreads();
    if (k < (uint32_t)kSegClasses) counts[k] = s_start[k + 1u] - s_start[k];
    if (k == (uint32_t)kSegClasses - 1u && oversized) *oversized = s_start[k + 1u] - s_start[k];
}

template <typename U, int KIND, int DESC>
__global__ __launch_bounds__(kSelNT) void segments_sort_kernel(const U* __restrict__ keys, uint32_t n, const uint32_t* __restrict__ off,
                                                               uint32_t S, const uint32_t* __restrict__ ids,
                                                               const uint32_t* __restrict__ counts, uint32_t global_index,
                                                               U* __restrict__ keys_out, uint32_t* __restrict__ index_out)
{
    __shared__ RowItems<U> s;
    __shared__ uint32_t s_lo[kSegMaxBlocks];
    __shared__ uint16_t s_len[kSegMaxBlocks];   // (<= kRowCap)
    __shared__ uint32_t s_first[kSegClasses + 1];   // s_first[k]: the first tile of class k in the concatenated index; [14]: all tiles
    __shared__ uint32_t s_list[kSegClasses];        // the first entry of class k in ids
    const uint32_t tid = threadIdx.x;

    if (tid == 0u) {
        uint32_t tile = 0u, entry = 0u;
        for (uint32_t k = 0u; k < (uint32_t)kSegClasses; ++k) {
            uint32_t c = counts[k];
            if (c > S - entry) c = S - entry;   // entry + c <= S whatever counts held.  BOUNDS (3)
            s_first[k] = tile;
            s_list[k] = entry;
            entry += c;
            if (k == (uint32_t)kSegClasses - 1u) tile += c;
            else if (k > 0u) tile += (c + ((uint32_t)kRowCap >> k) - 1u) >> (12u - k);   // ceil(c / G_k), G_k = 2^(12 - k)
        }
        s_first[kSegClasses] = tile;
    }
    __syncthreads();
    const uint32_t tiles = s_first[kSegClasses];

    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t k = 1u;
        while (k + 1u < (uint32_t)kSegClasses && t >= s_first[k + 1u]) ++k;   // (uniform over the workgroup)
        const uint32_t tt = t - s_first[k];
        const uint32_t listed = (k + 1u < (uint32_t)kSegClasses ? s_list[k + 1u] : S) - s_list[k];   // count_k, within S
        if (k == (uint32_t)kSegClasses - 1u) {   // a wrong bound: the segment as it came, identity indices
            uint32_t seg = ids[s_list[k] + tt];
            if (seg >= S) seg = S - 1u;
            const SegSpan sp = seg_span(off, seg, n);
            const uint32_t base = global_index ? sp.lo : 0u;
            for (uint32_t c = tid; c < sp.len; c += kSelNT) {
                if (keys_out) keys_out[(size_t)sp.lo + c] = keys[(size_t)sp.lo + c];
                if (index_out) index_out[(size_t)sp.lo + c] = base + c;
            }
            continue;
        }
        const uint32_t P = 1u << k, G = (uint32_t)kRowCap >> k;
        const uint32_t j0 = s_list[k] + tt * G;                          // (tt G < listed)
        const uint32_t g = listed - tt * G < G ? listed - tt * G : G;   // listed segments of this tile
        const uint32_t slots = g << k;
        __syncthreads();   // the tile before has been written out: s, s_lo and s_len are free
        for (uint32_t b = tid; b < g; b += kSelNT) {
            uint32_t seg = ids[j0 + b];
            if (seg >= S) seg = S - 1u;
            const SegSpan sp = seg_span(off, seg, n);
            s_lo[b] = sp.lo;
            s_len[b] = (uint16_t)(sp.len < P ? sp.len : P);
        }
        __syncthreads();
        for (uint32_t i = tid; i < slots; i += kSelNT) {
            const uint32_t b = i >> k, c = i & (P - 1u);
            if (c < (uint32_t)s_len[b]) s.put(i, key_enc<U, KIND, DESC>(keys[(size_t)s_lo[b] + c]), c);
            else s.pad(i);
        }
        __syncthreads();
        for (uint32_t kk = 2; kk <= P; kk <<= 1) {
            for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < slots / 2; i += kSelNT) {
                    const uint32_t l = ((i & ~(j - 1u)) << 1) | (i & (j - 1u));   // (l and l | j lie in one block: j < P)
                    s.cswap(l, l | j, ((l & (P - 1u)) & kk) == 0u);
                }
                __syncthreads();
            }
        }
        for (uint32_t i = tid; i < slots; i += kSelNT) {
            const uint32_t b = i >> k, c = i & (P - 1u);
            if (c < (uint32_t)s_len[b]) {
                const uint32_t lo = s_lo[b];
                if (keys_out) keys_out[(size_t)lo + c] = key_dec<U, KIND, DESC>(s.code(i));
                if (index_out) index_out[(size_t)lo + c] = s.col(i) + (global_index ? lo : 0u);
            }
        }
    }
}

// the flat path's last kernel: element j of the outputs is position pos[j] of the input, which lies in segment seg[j].  BOUNDS (4)
template <typename U>
__global__ __launch_bounds__(kSelNT) void segments_emit_kernel(const U* __restrict__ keys, const uint32_t* __restrict__ pos,
                                                               const uint32_t* __restrict__ seg, uint32_t n,
                                                               const uint32_t* __restrict__ off, uint32_t S, uint32_t global_index,
                                                               U* __restrict__ keys_out, uint32_t* __restrict__ index_out)
{
    const size_t stride = (size_t)gridDim.x * kSelNT;
    for (size_t j = (size_t)blockIdx.x * kSelNT + threadIdx.x; j < (size_t)n; j += stride) {
        uint32_t p = pos[j], sg = seg[j];
        if (p >= n) p = n - 1u;
        if (sg >= S) sg = S - 1u;
        if (index_out) {
            const uint32_t a = off[sg];
            index_out[j] = global_index ? p : p - (a < n ? a : n);
        }
        if (keys_out) keys_out[j] = keys[p];
    }
}

}  // namespace adlhip
