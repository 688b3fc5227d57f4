// unique_kernels.hpp -- the run stage of adlhip_run_length_encode / adlhip_unique_typed: one streaming stage over keys that are already
// grouped (sorted, for unique) that flags run heads, ranks them, compacts them and scatters the inverse.  No reference counterpart.
//
// A head is position 0 or a position j with key[j] != key[j - 1] (bits).  Run r starts at the r-th head.
//
//   runs_count_kernel   workgroup w counts the heads of its chunk                      -> chunk_heads[w]
//   scan_single_kernel  (radix_kernels.hpp) one workgroup: exclusive scan of the chunk counts in place, the total R -> the caller's word
//   runs_emit_kernel    workgroup w walks its chunk again, tile by tile, with a running base that starts at chunk_heads[w]:
//                       every element gets the rank of its run; heads write unique[r], offsets[r], first_index[r]; every element
//                       writes inverse[P[j]] = r; the last workgroup writes offsets[R] = n
//   runs_counts_kernel  counts[r] = offsets[r + 1] - offsets[r] for r < R (R read from the device word)
//
// A chunk is a contiguous range of whole tiles (the selection kernels' tile: kSelNT threads x kSelVecs 16-byte vectors), split on the
// host: workgroup w owns tiles [w * tiles_per_wg, min((w + 1) * tiles_per_wg, tiles)), and the host launches no workgroup without a
// tile.  A launch reads only what EARLIER launches wrote, so no workgroup waits on another: no look-back, no spinning, no residency
// assumption.  Nothing data-dependent reaches the host: grids depend on n alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "select_kernels.hpp"

namespace adlhip {

static_assert(kSelVecs <= 4, "runs_tile_heads packs one 16-bit head count per vector into 64 bits");

// sel_block_scan on four 16-bit fields at once (a field's total is at most kSelNT * 4 heads, so no field carries into the next)
__device__ __forceinline__ uint64_t runs_block_scan(uint64_t v, uint64_t* s_wave, uint64_t* total)
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

// bit j of the result: item j of this thread (sel_load_tile's numbering) is valid and a head.  The key in front of a vector's first
// item belongs to another thread, vector or tile: one scalar load (a line the neighbour's vector load fetches anyway).
template <typename U>
__device__ __forceinline__ uint32_t runs_tile_heads(const U* __restrict__ keys, uint32_t n, size_t tile, const U (&x)[kSelVecs * (16 / sizeof(U))],
                                                    uint32_t valid)
{
    constexpr int PER = 16 / (int)sizeof(U);
    uint32_t heads = 0;
#pragma unroll
    for (int u = 0; u < kSelVecs; ++u) {
        const size_t first = ((tile * kSelVecs + u) * kSelNT + threadIdx.x) * PER;
        U prev = (U)0;
        if (first > 0 && first < (size_t)n) prev = keys[first - 1];
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const bool in = (valid >> (u * PER + e)) & 1u;
            const bool head = in && (first + e == 0 || x[u * PER + e] != (e ? x[u * PER + e - 1] : prev));
            heads |= (head ? 1u : 0u) << (u * PER + e);
        }
    }
    return heads;
}

// chunk_heads[blockIdx.x] = the heads among the keys of this workgroup's tiles.  keys is 16-byte aligned.
template <typename U>
__global__ __launch_bounds__(kSelNT) void runs_count_kernel(const U* __restrict__ keys, uint32_t n, uint32_t tiles, uint32_t tiles_per_wg,
                                                            uint32_t* __restrict__ chunk_heads)
{
    constexpr int IT = kSelVecs * (16 / (int)sizeof(U));
    __shared__ uint32_t s_wave[kSelNT / 64];
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    uint32_t mine = 0;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        U x[IT];
        uint32_t pos[IT];
        const uint32_t valid = sel_load_tile<U, 0>(keys, nullptr, n, tile, x, pos);
        mine += (uint32_t)__popc(runs_tile_heads<U>(keys, n, tile, x, valid));
    }
    uint32_t total;
    (void)sel_block_scan(mine, s_wave, &total);
    if (threadIdx.x == 0) chunk_heads[blockIdx.x] = total;
}

// chunk_base[w] = the heads in front of workgroup w's chunk (the scanned counts).  HAS_INDEX: perm[j] = the input position of keys[j]
// (the argsort's index), read for first_index and inverse; else both are null.  unique_out is required; offsets, first_index and
// inverse are written where given.  Elements at R and beyond (offsets: R + 1) are never written.
template <typename U, int HAS_INDEX>
__global__ __launch_bounds__(kSelNT) void runs_emit_kernel(const U* __restrict__ keys, const uint32_t* __restrict__ perm, uint32_t n, uint32_t tiles,
                                                           uint32_t tiles_per_wg, const uint32_t* __restrict__ chunk_base,
                                                           U* __restrict__ unique_out, uint32_t* __restrict__ offsets,
                                                           uint32_t* __restrict__ first_index, uint32_t* __restrict__ inverse)
{
    constexpr int PER = 16 / (int)sizeof(U);
    constexpr int IT = kSelVecs * PER;
    __shared__ uint64_t s_wave[kSelNT / 64];
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    uint32_t base = chunk_base[blockIdx.x];   // heads in front of the current tile
    for (uint32_t tile = t0; tile < t1; ++tile) {
        U x[IT];
        uint32_t pos[IT];
        const uint32_t valid = sel_load_tile<U, HAS_INDEX>(keys, perm, n, tile, x, pos);
        const uint32_t heads = runs_tile_heads<U>(keys, n, tile, x, valid);
        // element order inside a tile is (vector u, thread, item e): one scanned field per vector
        uint64_t mine = 0;
#pragma unroll
        for (int u = 0; u < kSelVecs; ++u) mine |= (uint64_t)__popc((heads >> (u * PER)) & ((1u << PER) - 1u)) << (16 * u);
        uint64_t total;
        const uint64_t excl = runs_block_scan(mine, s_wave, &total) - mine;
        uint32_t before = base;   // heads in front of vector u of thread 0
#pragma unroll
        for (int u = 0; u < kSelVecs; ++u) {
            const size_t first = ((size_t)(tile * (uint32_t)kSelVecs + u) * kSelNT + threadIdx.x) * PER;
            uint32_t h = before + (uint32_t)((excl >> (16 * u)) & 0xffffu);   // heads in front of this thread's item (u, 0)
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                const int j = u * PER + e;
                if (!((valid >> j) & 1u)) continue;
                const bool head = (heads >> j) & 1u;
                const uint32_t r = head ? h : h - 1u;   // (position 0 is a head, so h >= 1 wherever an item is not)
                h += head ? 1u : 0u;
                if (head && r < n) {   // (never false: there are at most n heads)
                    unique_out[r] = x[j];
                    if (offsets) offsets[r] = (uint32_t)(first + e);
                    if (HAS_INDEX && first_index) first_index[r] = pos[j];
                }
                if (HAS_INDEX && inverse && pos[j] < n) inverse[pos[j]] = r;   // (never false: perm is a permutation of 0 .. n - 1)
            }
            before += (uint32_t)((total >> (16 * u)) & 0xffffu);
        }
        base = before;
    }
    // the last workgroup holds position n - 1: base is R now
    if (offsets && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && base <= n) offsets[base] = n;
}

// counts[r] = offsets[r + 1] - offsets[r] for r < *num_runs.  The grid depends on n alone -- one workgroup per kRunsCountsPerWg possible
// runs --; workgroups with nothing to do leave at once.  (A fixed trip count: a grid-stride loop has the compiler divide by the stride.)
constexpr int kRunsCountsPerWg = kSelNT * 8;
ADLHIP_KERNEL __global__ __launch_bounds__(kSelNT) void runs_counts_kernel(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ num_runs,
                                                                           uint32_t n, uint32_t* __restrict__ counts)
{
    const uint32_t runs = *num_runs < n ? *num_runs : n;   // (never more than n)
    const size_t first = (size_t)blockIdx.x * kRunsCountsPerWg + threadIdx.x;
    if ((size_t)blockIdx.x * kRunsCountsPerWg >= runs) return;
#pragma unroll
    for (int k = 0; k < kRunsCountsPerWg / kSelNT; ++k) {
        const size_t r = first + (size_t)k * kSelNT;
        if (r < runs) counts[r] = offsets[r + 1] - offsets[r];
    }
}

}  // namespace adlhip
