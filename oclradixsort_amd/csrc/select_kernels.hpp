// select_kernels.hpp -- top-k selection of typed keys (adlhip_topk_typed).  No reference counterpart.
//
// Radix select, most significant digit first, on the composite ordinal (key_enc(key), input position): unsigned ascending order of
// the code is the requested order (descending included), positions ascend in both orders, so the composite order IS the stable
// order and all composites are distinct -- the k-th one is unique and ties at the k-th key need no mechanism of their own.  Digits
// are 11 bits (2048 u32 bins = 8 KiB of LDS); when the key's digits are used up the next ones come from the position.
//
//   level 0      select_hist_kernel: histogram of digit 0 over the input
//   level i >= 1 select_filter_kernel (one launch each): every workgroup finds the bin of histogram i-1 that holds the wanted rank
//                (a 2048-entry scan), then streams its source -- the input at level 1, the survivor list of level i-1 afterwards:
//                  digit i-1 before the chosen bin  -> selected: the position goes to the result list
//                  digit i-1 in the chosen bin      -> survives: {code, position} goes to the next list, digit i is counted
//                  anything else                    -> dropped
//                When the chosen bin holds exactly the rank still wanted, its keys are selected as well and selection is complete:
//                the level writes rem = 0 and every later level leaves at once.  That is certain to happen at the last level, where
//                every non-empty bin holds one composite.
// Nothing data-dependent reaches the host: grids are fixed by n, the trip counts are read from SelState, which lives in the caller's
// work buffer and is cleared in stream order by the entry point.  A level reads only words that EARLIER launches wrote (rem[i-1],
// survivors[i-1], hist[i-1]) and writes only its own (rem[i], survivors[i], hist[i], selected), so no workgroup depends on another
// workgroup of its launch: no barrier across the grid, no residency assumption.
// Cursors are bumped once per workgroup and tile (the selected / surviving items of a tile are counted by a workgroup scan first), the
// histogram is flushed with one device-scope atomic per non-empty bin and workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "typed_kernels.hpp"

namespace adlhip {

constexpr int kSelNT = 256;        // threads per workgroup
constexpr int kSelVecs = 4;        // 16-byte vectors per thread and tile: a tile is kSelNT * kSelVecs * (16 / key bytes) items
constexpr int kSelDigitBits = 11;
constexpr int kSelBins = 1 << kSelDigitBits;
constexpr int kSelMaxLevels = 9;   // 64 key bits + 32 position bits in 11-bit digits: 6 + 3

// digit = ((from_pos ? position : code) >> shift) & mask
struct SelDigit {
    uint32_t from_pos, shift, mask;
};

struct SelState {
    uint32_t hist[kSelMaxLevels + 1][kSelBins];   // [i]: digit i of the survivors of level i (level 0: of every key)
    uint32_t rem[kSelMaxLevels + 1];              // [i]: rank still wanted inside the bin level i chose; 0 = selection complete
    uint32_t survivors[kSelMaxLevels + 1];        // [i]: length of the list level i wrote (its cursor)
    uint32_t selected;                            // cursor of the result list
    uint32_t pad[43];                             // (a multiple of 256 bytes)
};
static_assert(sizeof(SelState) % 256 == 0, "what follows SelState in the work buffer is 256-byte aligned");

template <typename U>
__device__ __forceinline__ uint32_t sel_digit(const SelDigit g, U code, uint32_t pos)
{
    return (g.from_pos ? pos >> g.shift : (uint32_t)(code >> g.shift)) & g.mask;
}

// inclusive sum of v over the workgroup's threads in thread order; *total = the sum over all of them.  Every thread calls it.
__device__ __forceinline__ uint32_t sel_block_scan(uint32_t v, uint32_t* s_wave, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= (uint32_t)o) v += t;
    }
    __syncthreads();   // s_wave may still be read from the call before
    if (lane == 63u) s_wave[w] = v;
    __syncthreads();
    uint32_t add = 0, sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kSelNT / 64; ++j) {
        const uint32_t t = s_wave[j];
        if (j < w) add += t;
        sum += t;
    }
    *total = sum;
    return v + add;
}

// h[dg] += 1 for every lane with pred; one add of the lane count where the whole wave has the same digit (all keys equal would
// otherwise serialise 64 lanes on one LDS word).  Called in uniform control flow.
__device__ __forceinline__ void sel_hist_add(uint32_t* h, bool pred, uint32_t dg)
{
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dg);
    if (__all(pred && dg == d0)) {
        if ((threadIdx.x & 63u) == 0u) atomicAdd(&h[d0], 64u);
    } else if (pred) {
        atomicAdd(&h[dg], 1u);
    }
}

template <typename U>
struct alignas(4 * (16 / sizeof(U))) SelPosVec {
    uint32_t v[16 / sizeof(U)];
};

// This thread's items of one tile: item (u, e) is element ((tile * kSelVecs + u) * kSelNT + thread) * PER + e of the source, so that a
// wave's 16-byte loads are contiguous.  Whole vectors take one 16-byte load, the cnt % PER items behind the last whole vector (and a
// source shorter than one vector) are loaded one by one; items past cnt are 0 and their bit in the returned mask is clear.
// HAS_POS: positions come from src_pos, else an item's position is its index.
template <typename U, int HAS_POS>
__device__ __forceinline__ uint32_t sel_load_tile(const U* __restrict__ src, const uint32_t* __restrict__ src_pos, size_t cnt, size_t tile,
                                                  U (&x)[kSelVecs * (16 / sizeof(U))], uint32_t (&pos)[kSelVecs * (16 / sizeof(U))])
{
    constexpr int PER = 16 / (int)sizeof(U);
    uint32_t valid = 0;
#pragma unroll
    for (int u = 0; u < kSelVecs; ++u) {
        const size_t first = ((tile * kSelVecs + u) * kSelNT + threadIdx.x) * PER;
        if (first + PER <= cnt) {
            const KeyVec<U> kv = *reinterpret_cast<const KeyVec<U>*>(src + first);
            SelPosVec<U> pv;
            if (HAS_POS) pv = *reinterpret_cast<const SelPosVec<U>*>(src_pos + first);
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                x[u * PER + e] = kv.v[e];
                pos[u * PER + e] = HAS_POS ? pv.v[e] : (uint32_t)(first + e);
            }
            valid |= ((1u << PER) - 1u) << (u * PER);
        } else {
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                const bool in = first + e < cnt;
                x[u * PER + e] = in ? src[first + e] : (U)0;
                pos[u * PER + e] = in ? (HAS_POS ? src_pos[first + e] : (uint32_t)(first + e)) : 0u;
                valid |= (in ? 1u : 0u) << (u * PER + e);
            }
        }
    }
    return valid;
}

__device__ __forceinline__ void sel_hist_flush(const uint32_t* h, uint32_t* __restrict__ out)
{
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < (uint32_t)kSelBins; b += kSelNT) {
        const uint32_t c = h[b];
        if (c) atomicAdd(&out[b], c);   // device scope: the workgroups of a launch sit on every XCD
    }
}

// level 0: st->hist[0][digit 0 of enc(keys[i])] += 1 for i < n.  keys is 16-byte aligned; st->hist[0] is zero on entry.
template <typename U, int KIND, int DESC>
__global__ __launch_bounds__(kSelNT) void select_hist_kernel(const U* __restrict__ keys, uint32_t n, SelState* __restrict__ st, SelDigit cd)
{
    constexpr int IT = kSelVecs * (16 / (int)sizeof(U));
    __shared__ uint32_t h[kSelBins];
    for (uint32_t b = threadIdx.x; b < (uint32_t)kSelBins; b += kSelNT) h[b] = 0u;
    __syncthreads();
    const size_t tiles = ((size_t)n + (size_t)IT * kSelNT - 1) / ((size_t)IT * kSelNT);
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        U x[IT];
        uint32_t pos[IT];
        const uint32_t valid = sel_load_tile<U, 0>(keys, nullptr, n, tile, x, pos);
#pragma unroll
        for (int j = 0; j < IT; ++j) sel_hist_add(h, (valid >> j) & 1u, sel_digit<U>(cd, key_enc<U, KIND, DESC>(x[j]), pos[j]));
    }
    sel_hist_flush(h, st->hist[0]);
}

// level >= 1 (see the head of this file).  FIRST: level 1 -- the source is the input (src_codes = the typed keys, encoded here;
// src_pos unused; n of them; the rank wanted is k); else the source is the list of level - 1 (codes, positions,
// st->survivors[level - 1] of them; the rank wanted is st->rem[level - 1]; KIND and DESC are unused).  fd = digit level - 1 (the one the
// chosen bin is about), cd = digit level (counted for the next level).  result holds k positions, the lists n items.
template <typename U, int KIND, int DESC, int FIRST>
__global__ __launch_bounds__(kSelNT) void select_filter_kernel(const U* __restrict__ src_codes, const uint32_t* __restrict__ src_pos,
                                                               U* __restrict__ dst_codes, uint32_t* __restrict__ dst_pos,
                                                               uint32_t* __restrict__ result, SelState* __restrict__ st, uint32_t level,
                                                               uint32_t n, uint32_t k, SelDigit fd, SelDigit cd)
{
    constexpr int IT = kSelVecs * (16 / (int)sizeof(U));
    __shared__ uint32_t h[kSelBins];
    __shared__ uint32_t s_wave[kSelNT / 64];
    __shared__ uint32_t s_pick[3];   // chosen bin, keys before it, keys in it
    __shared__ uint32_t s_base[2];
    const uint32_t tid = threadIdx.x;

    const uint32_t rem_in = FIRST ? k : st->rem[level - 1];
    if (rem_in == 0u) {   // selection was complete before this level (uniform over the grid)
        if (blockIdx.x == 0 && tid == 0) st->rem[level] = 0u;
        return;
    }
    const size_t cnt = FIRST ? n : (st->survivors[level - 1] < n ? st->survivors[level - 1] : n);   // (never more than n: the lists hold n)

    // the bin of histogram level - 1 that holds the rem_in-th of its keys: thread t owns bins 8 t .. 8 t + 7
    {
        const uint32_t* hp = st->hist[level - 1] + tid * 8u;
        uint32_t c[8], s = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += c[j] = hp[j];
        if (tid < 3u) s_pick[tid] = 0u;
        uint32_t total;
        const uint32_t incl = sel_block_scan(s, s_wave, &total);   // (its barriers order the clearing of s_pick before the write below)
        uint32_t run = incl - s;
        if (run < rem_in && rem_in <= incl) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (run < rem_in && rem_in <= run + c[j]) {
                    s_pick[0] = tid * 8u + j;
                    s_pick[1] = run;
                    s_pick[2] = c[j];
                }
                run += c[j];
            }
        }
        for (uint32_t b = tid; b < (uint32_t)kSelBins; b += kSelNT) h[b] = 0u;
        __syncthreads();
    }
    const uint32_t bin = s_pick[0];
    const uint32_t rem_out = rem_in - s_pick[1];
    const bool all = s_pick[2] == rem_out;   // the chosen bin is wanted whole: selection ends here
    if (blockIdx.x == 0 && tid == 0) st->rem[level] = all ? 0u : rem_out;

    const size_t tiles = (cnt + (size_t)IT * kSelNT - 1) / ((size_t)IT * kSelNT);
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        U x[IT];
        uint32_t pos[IT];
        const uint32_t valid = sel_load_tile<U, !FIRST>(src_codes, src_pos, cnt, tile, x, pos);
        uint32_t selm = 0, surm = 0;
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            if (FIRST) x[j] = key_enc<U, KIND, DESC>(x[j]);
            const uint32_t dg = sel_digit<U>(fd, x[j], pos[j]);
            const bool in = (valid >> j) & 1u;
            selm |= (in && (dg < bin || (all && dg == bin)) ? 1u : 0u) << j;
            surm |= (in && !all && dg == bin ? 1u : 0u) << j;
        }
        // one bump of each cursor per workgroup and tile: selected count in the low half, survivor count in the high half (<= 4096 each)
        const uint32_t mine = (uint32_t)__popc(selm) | ((uint32_t)__popc(surm) << 16);
        uint32_t total;
        const uint32_t excl = sel_block_scan(mine, s_wave, &total) - mine;
        if (tid == 0) {
            s_base[0] = (total & 0xffffu) ? atomicAdd(&st->selected, total & 0xffffu) : 0u;
            s_base[1] = (total >> 16) ? atomicAdd(&st->survivors[level], total >> 16) : 0u;
        }
        __syncthreads();
        uint32_t so = s_base[0] + (excl & 0xffffu), vo = s_base[1] + (excl >> 16);
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            const bool sel = (selm >> j) & 1u, sur = (surm >> j) & 1u;
            if (sel) {
                if (so < k) result[so] = pos[j];   // (never false: the bins before the chosen one hold fewer than rem_in keys)
                ++so;
            }
            if (sur) {
                if (vo < n) {
                    dst_codes[vo] = x[j];
                    dst_pos[vo] = pos[j];
                }
                ++vo;
            }
            sel_hist_add(h, sur, sel_digit<U>(cd, x[j], pos[j]));
        }
    }
    sel_hist_flush(h, st->hist[level]);
}

// out[j] = keys[pos[j]] for j < k
template <typename U>
__global__ __launch_bounds__(kSelNT) void select_gather_kernel(const U* __restrict__ keys, const uint32_t* __restrict__ pos,
                                                               U* __restrict__ out, uint32_t k)
{
    const uint32_t stride = gridDim.x * (uint32_t)kSelNT;
    for (uint32_t j = blockIdx.x * (uint32_t)kSelNT + threadIdx.x; j < k; j += stride) out[j] = keys[pos[j]];
}

}  // namespace adlhip
