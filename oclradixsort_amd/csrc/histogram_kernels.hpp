// histogram_kernels.hpp -- histograms of typed keys (adlhip_histogram_range_typed / adlhip_bincount_typed): how many keys fall in each
// bin, the bins given by sorted edges or by the key's own value.  No reference counterpart.
//
// LDS path (range mode; bincount up to kHistLdsBins bins):
//   hist_count_kernel   workgroup w walks its chunk tile by tile, computes every key's bin and adds 1 to a zeroed table in LDS with
//                       DS atomics; at the end it stores the whole table, all num_bins words, as row w of the work buffer
//   hist_reduce_kernel  counts[b] = the sum of column b over the rows, rows read 32 bins (128 bytes) at a time
// Sorted path (bincount above that limit; the host sorts a copy of the keys as unsigned numbers and clears the counters first):
//   hist_heads_kernel   the first position i of every run of equal keys stores -i in counts[key]
//   hist_tails_kernel   the last position i of every run adds i + 1 to counts[key]: one writer per word per launch
//
// Range mode: bin = (the number of edges <= key) - 1, both sides as the order-preserving code of typed_kernels.hpp (red_enc with the
// key's kind at run time, as compact_kernels.hpp compares), found by a branch-free binary search over the num_bins + 1 edge codes in
// LDS.  Every probe index is clamped to the edge array and the result to [0, num_bins) or "ignored", so unsorted edges give
// unspecified counts and no access outside the arrays.  A key at or above the last edge is ignored, unless include_upper is set and
// its code equals the last edge's: then it counts in the last bin whose lower edge is below the last edge (num_bins - 1 if there is
// none).  Bincount: bin = the key's bits as an unsigned number when that is below num_bins -- a negative key is a large unsigned
// number and falls out by the same comparison.
//
// Same-bin conflicts.  Lanes that add to one counter serialise, and so do lanes that add to different words of one bank.  The table is
// therefore kept in `copies` sub-tables (a power of two, as many as fit the counter budget, at most kHistMaxCopies), lane l adding to
// sub-table l % copies; the sub-tables lie an ODD number of words apart, so one bin's copies sit in different banks.  A lane first
// combines runs of equal bins among its own 8 consecutive items into one add.  The sub-tables are summed when the row is stored.
// One table and one add per key was built first and measured in the same session: within 4 % on uniform keys, 1.2 to 4.5 x as long
// on all-equal keys; it is gone, there is one path and no knob.
//
// The tile is the reduce stage's: kRedTile = 2048 elements, 8 consecutive elements per thread, 16-byte loads (red_load).  A chunk is a
// contiguous range of whole tiles, split on the host.  A launch reads only what EARLIER launches wrote: no workgroup waits on
// another, no atomics to global memory, nothing data-dependent reaches the host.  Counts are sums of integers: exact, and the same
// from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reduce_kernels.hpp"

namespace adlhip {

constexpr int kHistRange = 0, kHistBincount = 1;   // MODE of the count kernel
constexpr uint32_t kHistIgnored = 0xffffffffu;     // the bin of a key that is not counted
constexpr uint32_t kHistRangeWords = 4096;         // counter words of the range mode (ADLHIP_HISTOGRAM_MAX_RANGE_BINS): with 4097 8-byte
                                                   // edges 49 172 bytes, three workgroups per CU
constexpr uint32_t kHistLdsBins = 8192;            // counter words of bincount = the largest table of the LDS path: 32 KiB, four
                                                   // workgroups in the 160 KiB of a CU
constexpr uint32_t kHistMaxCopies = 32;            // sub-tables at most
constexpr uint32_t kHistRedBins = 32;              // bins per workgroup of the reduce kernel (kSelNT / kHistRedBins groups of rows)

struct HistArgs {
    uint32_t kind;            // kKey* of the keys (range mode)
    uint32_t num_bins;
    uint32_t include_upper;   // range mode
    uint32_t copies, stride;  // sub-tables and the words between them (odd, >= num_bins)
    uint32_t top_step;        // the largest power of two <= num_bins + 1 (range mode)
};

// dynamic LDS of hist_count_kernel
template <typename U, int MODE>
__host__ __device__ constexpr uint32_t hist_edge_bytes(uint32_t num_bins)
{
    return MODE == kHistRange ? (uint32_t)(((size_t)(num_bins + 1) * sizeof(U) + 15u) & ~(size_t)15u) : 0u;
}

// the number of codes e[0 .. len) that are <= code (STRICT: < code) when e is non-decreasing; always in [0, len]
template <typename U, bool STRICT>
__device__ __forceinline__ uint32_t hist_search(const U* e, uint32_t len, uint32_t top_step, U code)
{
    uint32_t pos = 0;
    for (uint32_t step = top_step; step; step >>= 1) {
        const uint32_t t = pos + step;
        const U ev = e[(t < len ? t : len) - 1u];
        const bool below = STRICT ? ev < code : ev <= code;
        pos = (t <= len && below) ? t : pos;
    }
    return pos;
}

// rows[blockIdx.x * num_bins + b] = the keys of this workgroup's tiles that fall in bin b, for every b < num_bins.  keys and edges are
// 16-byte aligned; edges (range mode) holds num_bins + 1 keys.  Dynamic LDS: hist_edge_bytes + copies * stride words.
template <typename U, int MODE>
__global__ __launch_bounds__(kSelNT) void hist_count_kernel(const U* __restrict__ keys, uint32_t n, uint32_t tiles, uint32_t tiles_per_wg,
                                                            const U* __restrict__ edges, HistArgs a, uint32_t* __restrict__ rows)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_hist[];
    U* s_edge = reinterpret_cast<U*>(s_hist);
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_hist + hist_edge_bytes<U, MODE>(a.num_bins));
    const uint32_t B = a.num_bins, len = B + 1u;
    const RedCodec codec = {a.kind, 0u};
    for (uint32_t i = threadIdx.x; i < a.copies * a.stride; i += (uint32_t)kSelNT) s_cnt[i] = 0u;
    if constexpr (MODE == kHistRange) {
        for (uint32_t i = threadIdx.x; i < len; i += (uint32_t)kSelNT) s_edge[i] = red_enc<U, kRedMax>(edges[i], codec);
    }
    __syncthreads();
    U top = (U)0;
    uint32_t upper_bin = kHistIgnored;   // where a key equal to the last edge goes
    if constexpr (MODE == kHistRange) {
        top = s_edge[B];
        if (a.include_upper) {
            const uint32_t lower = hist_search<U, true>(s_edge, len, a.top_step, top);   // edges below the last one
            upper_bin = lower == 0u ? B - 1u : (lower - 1u < B - 1u ? lower - 1u : B - 1u);
        }
    }
    uint32_t* mine = s_cnt + (threadIdx.x & (a.copies - 1u)) * a.stride;
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const size_t first = (size_t)tile * kRedTile + (size_t)threadIdx.x * kRedItems;
        const uint32_t cnt = first >= (size_t)n ? 0u : ((size_t)n - first < (size_t)kRedItems ? (uint32_t)((size_t)n - first) : (uint32_t)kRedItems);
        U x[kRedItems];
        red_load<U>(keys, first, cnt, x);
        uint32_t bin[kRedItems];
        if constexpr (MODE == kHistRange) {
            uint32_t pos[kRedItems];
#pragma unroll
            for (int e = 0; e < kRedItems; ++e) {
                x[e] = red_enc<U, kRedMax>(x[e], codec);
                pos[e] = 0u;
            }
            for (uint32_t step = a.top_step; step; step >>= 1) {   // the 8 searches side by side: 8 independent LDS reads per step
#pragma unroll
                for (int e = 0; e < kRedItems; ++e) {
                    const uint32_t t = pos[e] + step;
                    const U ev = s_edge[(t < len ? t : len) - 1u];
                    pos[e] = (t <= len && ev <= x[e]) ? t : pos[e];
                }
            }
#pragma unroll
            for (int e = 0; e < kRedItems; ++e) {
                uint32_t b = pos[e] - 1u;                              // pos 0 (below the first edge): kHistIgnored
                if (pos[e] > B) b = x[e] == top ? upper_bin : kHistIgnored;
                bin[e] = (uint32_t)e < cnt ? b : kHistIgnored;
            }
        } else {
#pragma unroll
            for (int e = 0; e < kRedItems; ++e) bin[e] = ((uint32_t)e < cnt && x[e] < (U)B) ? (uint32_t)x[e] : kHistIgnored;
        }
        // one add per run of equal bins among the thread's items: the run's first item adds the run's length
        uint32_t run[kRedItems];
        run[kRedItems - 1] = 1u;
#pragma unroll
        for (int e = kRedItems - 2; e >= 0; --e) run[e] = bin[e] == bin[e + 1] ? run[e + 1] + 1u : 1u;
#pragma unroll
        for (int e = 0; e < kRedItems; ++e)
            if (bin[e] < B && (e == 0 || bin[e] != bin[e - 1])) atomicAdd(&mine[bin[e]], run[e]);
    }
    __syncthreads();
    uint32_t* row = rows + (size_t)blockIdx.x * B;
    for (uint32_t b = threadIdx.x; b < B; b += (uint32_t)kSelNT) {
        uint32_t sum = 0u;
        for (uint32_t c = 0; c < a.copies; ++c) sum += s_cnt[c * a.stride + b];
        row[b] = sum;
    }
}

// counts[b] = rows[0][b] + ... + rows[num_rows - 1][b] for every b < num_bins.  A workgroup takes kHistRedBins bins; its threads form
// kSelNT / kHistRedBins groups that take every such-th row, 128 contiguous bytes per group and row.
ADLHIP_KERNEL __global__ __launch_bounds__(kSelNT) void hist_reduce_kernel(const uint32_t* __restrict__ rows, uint32_t num_rows, uint32_t num_bins,
                                                                            uint32_t* __restrict__ counts)
{
    constexpr uint32_t GROUPS = (uint32_t)kSelNT / kHistRedBins;
    __shared__ uint32_t s_part[kSelNT];
    const uint32_t col = threadIdx.x % kHistRedBins, g = threadIdx.x / kHistRedBins;
    const uint32_t b = blockIdx.x * kHistRedBins + col;
    uint32_t sum = 0u;
    if (b < num_bins) {
#pragma unroll 8
        for (uint32_t r = g; r < num_rows; r += GROUPS) sum += rows[(size_t)r * num_bins + b];
    }
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (g == 0u && b < num_bins) {
#pragma unroll
        for (uint32_t k = 1; k < GROUPS; ++k) sum += s_part[k * kHistRedBins + col];
        counts[b] = sum;
    }
}

// sorted holds n keys in ascending unsigned order; counts holds num_bins zeros.  Afterwards counts[v] = -(the first position of v).
template <typename U>
__global__ __launch_bounds__(kSelNT) void hist_heads_kernel(const U* __restrict__ sorted, uint32_t n, uint32_t num_bins, uint32_t* __restrict__ counts)
{
    const size_t stride = (size_t)gridDim.x * kSelNT;
    for (size_t i = (size_t)blockIdx.x * kSelNT + threadIdx.x; i < (size_t)n; i += stride) {
        const U k = sorted[i];
        if (k < (U)num_bins && (i == 0 || sorted[i - 1] != k)) counts[(uint32_t)k] = 0u - (uint32_t)i;
    }
}

// counts[v] += (the last position of v) + 1: with the heads' -first, the length of v's run (mod 2^32, and a run is shorter than that)
template <typename U>
__global__ __launch_bounds__(kSelNT) void hist_tails_kernel(const U* __restrict__ sorted, uint32_t n, uint32_t num_bins, uint32_t* __restrict__ counts)
{
    const size_t stride = (size_t)gridDim.x * kSelNT;
    for (size_t i = (size_t)blockIdx.x * kSelNT + threadIdx.x; i < (size_t)n; i += stride) {
        const U k = sorted[i];
        if (k < (U)num_bins && (i + 1 == (size_t)n || sorted[i + 1] != k)) counts[(uint32_t)k] += (uint32_t)i + 1u;
    }
}

}  // namespace adlhip
