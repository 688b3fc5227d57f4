// sortrows_kernels.hpp -- sort and argsort along the rows of a rows x cols matrix of typed keys (adlhip_sort_rows_typed).  No
// reference counterpart.  The contract, per row: the stable typed argsort of the row, that is its composites (key_enc(key), column)
// in unsigned ascending order.  All composites of a row are distinct, so arrival order in LDS never matters.
//
//   the row kernel  cols <= kRowCap.  A tile is the kRowCap LDS slots of toprows_kernels.hpp (RowItems<U>).  With P = 1 << shift the
//                   power of two >= cols (at least 2) it holds G = kRowCap / P rows side by side: row b of the tile in slots
//                   [b P, b P + cols), the slots up to (b + 1) P padded with the all-ones composite.  One bitonic network over the
//                   occupied blocks runs the merge phases up to length P only, and takes the compare direction from the index
//                   inside the block, (l & (P - 1)) & kk, not from the index in the tile: every block comes out ascending, all G
//                   rows in log2(P) (log2(P) + 1) / 2 stages.  Workgroups of 256 threads take tiles in turns (blockIdx.x,
//                   blockIdx.x + gridDim.x, ...); the last tile may hold fewer than G rows, whose blocks are neither loaded, sorted
//                   nor stored.
//                   row_stride == cols: the rows of a tile are one contiguous span, swept once by row_sweep (16-byte loads on its
//                   body, its two ends element by element); an element's row is its index in the span divided by cols, by a
//                   multiplication with the host's reciprocal.  A larger stride: one sweep per row.  Elements between cols and
//                   row_stride are never read.  The outputs are written once, densely, 4 or 8 bytes per thread in index order.
//                   Nothing but keys_out / index_out is written: no global scratch, no atomics to global memory, no fence, and no
//                   workgroup depends on another.
//   the flat path   three streaming kernels around the flat argsort and the stable (row, position) sort, see primitives.hip:
//                   rows_pack_kernel (dense copy of strided rows), rows_of_positions_kernel (p / cols), rows_emit_kernel (columns
//                   and gathered keys).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "toprows_kernels.hpp"

namespace adlhip {

// e / cols for e * cols < 2^32, with inv = 2^32 / cols + 1 from the host: inv cols = 2^32 + x with 0 < x <= cols, so
// e inv / 2^32 = e / cols + e x / (cols 2^32), and the second term is below 1 / cols, the least distance of e / cols to the next integer
__device__ __forceinline__ uint32_t div_by_cols(uint32_t e, uint64_t inv) { return (uint32_t)(((uint64_t)e * inv) >> 32); }

template <typename U, int KIND, int DESC>
__global__ __launch_bounds__(kSelNT) void sort_rows_kernel(const U* __restrict__ keys, size_t rows, uint32_t cols, size_t row_stride,
                                                           uint32_t shift, uint64_t inv_cols, U* __restrict__ keys_out,
                                                           uint32_t* __restrict__ index_out)
{
    __shared__ RowItems<U> s;
    const uint32_t tid = threadIdx.x;
    const uint32_t P = 1u << shift;
    const size_t G = (size_t)kRowCap >> shift;
    const size_t tiles = (rows + G - 1) / G;

    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t r0 = t * G;
        const uint32_t g = (uint32_t)(rows - r0 < G ? rows - r0 : G);   // rows of this tile
        const uint32_t slots = g << shift, items = g * cols;            // (<= kRowCap both)
        __syncthreads();   // the tile before has been written out: s is free
        if (cols < P)
            for (uint32_t i = tid; i < slots; i += kSelNT)
                if ((i & (P - 1u)) >= cols) s.pad(i);
        if (row_stride == (size_t)cols) {
            row_sweep<U, KIND, DESC>(keys + r0 * row_stride, items, [&](U code, uint32_t e, bool in) {
                const uint32_t b = div_by_cols(e, inv_cols), col = e - b * cols;
                if (in) s.put((b << shift) + col, code, col);
            });
        } else {
            for (uint32_t b = 0; b < g; ++b)
                row_sweep<U, KIND, DESC>(keys + (r0 + b) * row_stride, cols, [&](U code, uint32_t col, bool in) {
                    if (in) s.put((b << shift) + col, code, col);
                });
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
        const size_t out0 = r0 * (size_t)cols;
        for (uint32_t e = tid; e < items; e += kSelNT) {
            const uint32_t b = div_by_cols(e, inv_cols);
            const uint32_t at = (b << shift) + (e - b * cols);
            if (keys_out) keys_out[out0 + e] = key_dec<U, KIND, DESC>(s.code(at));
            if (index_out) index_out[out0 + e] = s.col(at);
        }
    }
}

// ---- the flat path's streaming kernels: n = rows * cols elements, one per thread and turn ---------------------------------------
// dense[r cols + c] = keys[r row_stride + c]
template <typename U>
__global__ __launch_bounds__(kSelNT) void rows_pack_kernel(const U* __restrict__ keys, size_t n, uint32_t cols, size_t row_stride,
                                                           U* __restrict__ dense)
{
    const size_t stride = (size_t)gridDim.x * kSelNT;
    for (size_t i = (size_t)blockIdx.x * kSelNT + threadIdx.x; i < n; i += stride) {
        const uint32_t r = (uint32_t)i / cols;   // (the exact 32-bit division: i < 2^32 and nothing here is known to fit 24 bits)
        dense[i] = keys[(size_t)r * row_stride + ((uint32_t)i - r * cols)];
    }
}

// rowkey[j] = the row of position p[j]
ADLHIP_KERNEL __global__ __launch_bounds__(kSelNT) void rows_of_positions_kernel(const uint32_t* __restrict__ p, size_t n, uint32_t cols,
                                                                                 uint32_t* __restrict__ rowkey)
{
    const size_t stride = (size_t)gridDim.x * kSelNT;
    for (size_t j = (size_t)blockIdx.x * kSelNT + threadIdx.x; j < n; j += stride) rowkey[j] = p[j] / cols;
}

// index_out[j] = the column of position p[j] in its row rowkey[j]; keys_out[j] = the key there, fetched from the caller's input
template <typename U>
__global__ __launch_bounds__(kSelNT) void rows_emit_kernel(const U* __restrict__ keys, const uint32_t* __restrict__ p,
                                                           const uint32_t* __restrict__ rowkey, size_t n, uint32_t cols, size_t row_stride,
                                                           U* __restrict__ keys_out, uint32_t* __restrict__ index_out)
{
    const size_t stride = (size_t)gridDim.x * kSelNT;
    for (size_t j = (size_t)blockIdx.x * kSelNT + threadIdx.x; j < n; j += stride) {
        const uint32_t r = rowkey[j];
        const uint32_t col = p[j] - r * cols;
        if (index_out) index_out[j] = col;
        if (keys_out) keys_out[j] = keys[(size_t)r * row_stride + col];
    }
}

}  // namespace adlhip
