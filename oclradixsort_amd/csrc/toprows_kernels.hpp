// toprows_kernels.hpp -- row-wise top-k of typed keys (adlhip_topk_rows_typed, the row kernel).  No reference counterpart.
//
// One workgroup of 256 threads per row, rows taken in turns (blockIdx.x, blockIdx.x + gridDim.x, ...).  The contract is the one of
// select_kernels.hpp, per row: the first k entries of the stable typed argsort of the row, that is the k smallest composites
// (key_enc(key), column) in unsigned order.  All composites of a row are distinct, so arrival order in LDS never matters.
//
//   direct form  cols <= kRowCap: the row is read once into LDS, padded with the all-ones composite to a power of two, sorted by a
//                bitonic network, and its first k items are written.  No histogram.
//   select form  cols >  kRowCap: radix select on the composite, most significant digit first, in the digit plan of topk_digit
//                (11-bit digits of the code, then of the column).  A level streams the row (plain loads: the row is re-read and
//                should stay in L2), counts the digit of the items whose higher digits equal the chosen prefix into the LDS
//                histogram and scans the 2048 bins for the one that holds the wanted rank.  S = items strictly before the chosen
//                prefix (certainly selected, S < k), C = population of the chosen bin.  As soon as S + C <= kRowCap -- at the
//                latest at the last level, where C == 1; also when C is exactly the rank still wanted -- one collect sweep puts
//                those S + C items into LDS through an LDS cursor, and the direct form's pad, sort and write follow.
//
// A row may start at any element (row_stride and cols may be odd; only the base pointer is 16-byte aligned): every sweep takes the
// elements before the row's first 16-byte boundary and those behind its last whole vector one by one and the body in 16-byte
// loads.  Elements between cols and row_stride are never read.  Nothing but keys_out / index_out is written: no global scratch, no
// atomics to global memory, no fence, and no workgroup depends on another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "select_kernels.hpp"

namespace adlhip {

constexpr int kRowCap = 4096;    // items a workgroup holds and sorts in LDS
constexpr int kRowMaxK = 2048;   // the row kernel serves k up to this

struct RowPlan {
    SelDigit d[kSelMaxLevels];   // topk_digit(level, key bits, position bits of cols)
    uint32_t levels;
};

// the composites in LDS: 4-byte keys packed code << 32 | column (32 KiB), 8-byte keys as a code and a column array (48 KiB)
template <typename U>
struct RowItems;

template <>
struct RowItems<uint32_t> {
    uint64_t item[kRowCap];
    __device__ __forceinline__ void put(uint32_t i, uint32_t code, uint32_t col) { item[i] = ((uint64_t)code << 32) | col; }
    __device__ __forceinline__ void pad(uint32_t i) { item[i] = ~(uint64_t)0; }
    __device__ __forceinline__ uint32_t code(uint32_t i) const { return (uint32_t)(item[i] >> 32); }
    __device__ __forceinline__ uint32_t col(uint32_t i) const { return (uint32_t)item[i]; }
    // orders items l < r ascending (up) or descending
    __device__ __forceinline__ void cswap(uint32_t l, uint32_t r, bool up)
    {
        const uint64_t a = item[l], b = item[r];
        if ((a > b) == up) {
            item[l] = b;
            item[r] = a;
        }
    }
};

template <>
struct RowItems<uint64_t> {
    uint64_t codes[kRowCap];
    uint32_t cols[kRowCap];
    __device__ __forceinline__ void put(uint32_t i, uint64_t code, uint32_t col)
    {
        codes[i] = code;
        cols[i] = col;
    }
    __device__ __forceinline__ void pad(uint32_t i) { put(i, ~(uint64_t)0, ~0u); }   // (a real column is at most 2^32 - 2)
    __device__ __forceinline__ uint64_t code(uint32_t i) const { return codes[i]; }
    __device__ __forceinline__ uint32_t col(uint32_t i) const { return cols[i]; }
    __device__ __forceinline__ void cswap(uint32_t l, uint32_t r, bool up)
    {
        const uint64_t a = codes[l], b = codes[r];
        const uint32_t pa = cols[l], pb = cols[r];
        const bool gt = a > b || (a == b && pa > pb);
        if (gt == up) {
            codes[l] = b;
            codes[r] = a;
            cols[l] = pb;
            cols[r] = pa;
        }
    }
};

// f(code, column, in) for every element of the row, in uniform control flow: every thread of the workgroup makes the same calls,
// `in` is false where a thread has no element (code and column are then arbitrary).  Reads row[0 .. cols) and nothing else.
template <typename U, int KIND, int DESC, typename F>
__device__ __forceinline__ void row_sweep(const U* __restrict__ row, uint32_t cols, F&& f)
{
    constexpr uint32_t PER = 16 / (uint32_t)sizeof(U);
    const uint32_t tid = threadIdx.x;
    uint32_t head = (uint32_t)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) / (uint32_t)sizeof(U));
    if (head > cols) head = cols;
    const uint32_t nvec = (cols - head) / PER;
    const uint32_t tail0 = head + nvec * PER;
    const uint32_t ntail = cols - tail0;   // < PER
    {   // thread t < head: element t; thread head + j, j < ntail: element tail0 + j
        const bool in = tid < head + ntail;
        const uint32_t col = tid < head ? tid : tail0 + (tid - head);
        const U x = in ? row[col] : (U)0;
        f(key_enc<U, KIND, DESC>(x), col, in);
    }
    const KeyVec<U>* vp = reinterpret_cast<const KeyVec<U>*>(row + head);
    for (uint32_t v0 = 0; v0 < nvec; v0 += (uint32_t)(kSelNT * kSelVecs)) {
        KeyVec<U> kv[kSelVecs];
#pragma unroll
        for (int u = 0; u < kSelVecs; ++u) {
            const uint32_t v = v0 + (uint32_t)u * kSelNT + tid;
            if (v < nvec) {
                kv[u] = vp[v];
            } else {
#pragma unroll
                for (uint32_t e = 0; e < PER; ++e) kv[u].v[e] = (U)0;
            }
        }
#pragma unroll
        for (int u = 0; u < kSelVecs; ++u) {
            const uint32_t v = v0 + (uint32_t)u * kSelNT + tid;
#pragma unroll
            for (uint32_t e = 0; e < PER; ++e) f(key_enc<U, KIND, DESC>(kv[u].v[e]), head + v * PER + e, v < nvec);
        }
    }
}

template <typename U, int KIND, int DESC>
__global__ __launch_bounds__(kSelNT) void topk_rows_kernel(const U* __restrict__ keys, size_t rows, uint32_t cols, size_t row_stride,
                                                           uint32_t k, U* __restrict__ keys_out, uint32_t* __restrict__ index_out,
                                                           RowPlan plan)
{
    __shared__ RowItems<U> s;
    __shared__ uint32_t h[kSelBins];
    __shared__ uint32_t s_wave[kSelNT / 64];
    __shared__ uint32_t s_pick[3];   // chosen bin, items before it, items in it
    __shared__ uint32_t s_cursor;
    const uint32_t tid = threadIdx.x;

    for (size_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const U* __restrict__ row = keys + r * row_stride;
        __syncthreads();   // the row before has been written out: s, h and s_cursor are free
        uint32_t m = 0;    // items in LDS
        if (cols <= (uint32_t)kRowCap) {
            row_sweep<U, KIND, DESC>(row, cols, [&](U code, uint32_t col, bool in) {
                if (in) s.put(col, code, col);
            });
            m = cols;
        } else {
            // the chosen prefix: the items still in play are those with (code & mcode) == pcode && (col & mpos) == ppos
            U pcode = 0, mcode = 0;
            uint32_t ppos = 0, mpos = 0;
            uint32_t want = k, before = 0;   // rank still wanted inside the prefix (1-based); S
            if (tid == 0) s_cursor = 0u;
            for (uint32_t lv = 0; lv < plan.levels; ++lv) {
                const SelDigit g = plan.d[lv];
                for (uint32_t b = tid; b < (uint32_t)kSelBins; b += kSelNT) h[b] = 0u;
                if (tid < 3u) s_pick[tid] = 0u;
                __syncthreads();
                row_sweep<U, KIND, DESC>(row, cols, [&](U code, uint32_t col, bool in) {
                    sel_hist_add(h, in && (code & mcode) == pcode && (col & mpos) == ppos, sel_digit<U>(g, code, col));
                });
                __syncthreads();
                // the bin that holds the want-th item: thread t owns bins 8 t .. 8 t + 7
                const uint32_t* hp = h + tid * 8u;
                uint32_t c[8], sum = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) sum += c[j] = hp[j];
                uint32_t total;
                const uint32_t incl = sel_block_scan(sum, s_wave, &total);
                uint32_t run = incl - sum;
                if (run < want && want <= incl) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (run < want && want <= run + c[j]) {
                            s_pick[0] = tid * 8u + j;
                            s_pick[1] = run;
                            s_pick[2] = c[j];
                        }
                        run += c[j];
                    }
                }
                __syncthreads();
                const uint32_t bin = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_pick[0]);
                const uint32_t skip = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_pick[1]);
                const uint32_t held = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_pick[2]);
                __syncthreads();   // s_pick and h are cleared again at the next level
                before += skip;
                want -= skip;
                if (g.from_pos) {
                    ppos |= bin << g.shift;
                    mpos |= g.mask << g.shift;
                } else {
                    pcode |= (U)bin << g.shift;
                    mcode |= (U)g.mask << g.shift;
                }
                if (before + held <= (uint32_t)kRowCap) {
                    m = before + held;
                    break;
                }
            }
            // (the loop always leaves by the break: at the last level every bin holds one composite and before < k <= kRowMaxK)
            row_sweep<U, KIND, DESC>(row, cols, [&](U code, uint32_t col, bool in) {
                const U cm = code & mcode;
                const bool take = in && (cm < pcode || (cm == pcode && (col & mpos) <= ppos));
                const unsigned long long bm = __ballot(take);
                if (bm) {   // (uniform over the wave)
                    const uint32_t lane = tid & 63u;
                    uint32_t base = 0u;
                    if (lane == 0u) base = atomicAdd(&s_cursor, (uint32_t)__popcll(bm));
                    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                    const uint32_t at = base + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
                    if (take && at < (uint32_t)kRowCap) s.put(at, code, col);   // (never beyond: exactly m items are taken)
                }
            });
        }
        uint32_t P = 1;
        while (P < m) P <<= 1;
        for (uint32_t i = m + tid; i < P; i += kSelNT) s.pad(i);
        __syncthreads();
        for (uint32_t kk = 2; kk <= P; kk <<= 1) {
            for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < P / 2; i += kSelNT) {
                    const uint32_t l = ((i & ~(j - 1u)) << 1) | (i & (j - 1u));
                    s.cswap(l, l | j, (l & kk) == 0u);
                }
                __syncthreads();
            }
        }
        const size_t out0 = r * (size_t)k;
        for (uint32_t j = tid; j < k; j += kSelNT) {
            if (keys_out) keys_out[out0 + j] = key_dec<U, KIND, DESC>(s.code(j));
            if (index_out) index_out[out0 + j] = s.col(j);
        }
    }
}

}  // namespace adlhip
