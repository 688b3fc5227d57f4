// reduce_kernels.hpp -- the reduce stage of adlhip_reduce_runs / adlhip_reduce_by_key_typed: a segmented reduction (sum, min, max) of
// values over keys that are already grouped (sorted, for reduce_by_key).  No reference counterpart.
//
// A head is position 0 or a position j with key[j] != key[j - 1] (bits); run r starts at the r-th head.  A tail is position n - 1 or a
// position whose successor is a head; run r ends at the r-th tail.
//
//   reduce_partial_kernel  workgroup w walks its chunk once                             -> chunk_heads[w]: its head count,
//                          chunk_flag[w]: the chunk contains a head, chunk_agg[w]: the aggregate of the elements from its last head on
//                          (of the whole chunk if it has none; never empty)
//   reduce_carry_kernel    one workgroup: exclusive scan of the head counts in place (the total R -> the caller's word) and segmented
//                          exclusive scan of (flag, aggregate)                             -> chunk_carry[w]: the aggregate of the elements
//                          in front of chunk w that belong to the run open at its start (valid for every w > 0: no chunk is empty)
//   reduce_emit_kernel     workgroup w walks its chunk again, tile by tile, with a running (rank, carry): a segmented inclusive scan per
//                          tile; heads write unique[r] and offsets[r], tails write reduced[r]; the last workgroup writes offsets[R] = n
//   runs_counts_kernel     (unique_kernels.hpp) counts[r] = offsets[r + 1] - offsets[r]
//
// The tile is kRedTile = 2048 ELEMENTS whatever the widths: kSelNT threads x kRedItems = 8 consecutive elements per thread, so that a
// 4-byte key with an 8-byte value (and the reverse) has one geometry and a thread's scan over its own items needs no exchange.  A
// thread loads its items with 16-byte vector loads: 2 for a 4-byte array, 4 for an 8-byte one (the 32 or 64 bytes of a thread are
// contiguous; a wave's loads of one instruction are strided by that much, the lines are shared by the 2 or 4 instructions).
// A chunk is a contiguous range of whole tiles, split on the host as in unique_kernels.hpp.  A launch reads only what EARLIER launches
// wrote: no workgroup waits on another, no atomics to global memory, nothing data-dependent reaches the host.
//
// "Nothing yet" is a validity flag, never an identity element: an aggregate is combined with the operator only when both sides hold at
// least one element, so a run of one element returns that element's bits (-0, signalling NaNs, payloads).  Float sums are plain IEEE
// adds in an association that depends on n and the grid alone -- the same input, device and knobs give the same bits.
// MIN / MAX work on the order-preserving code of typed_kernels.hpp (the value's kind at run time): one unsigned max per width; MIN is
// the max of the complemented codes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "select_kernels.hpp"

namespace adlhip {

constexpr int kRedItems = 8;                    // consecutive elements per thread and tile
constexpr int kRedTile = kSelNT * kRedItems;    // elements per tile
constexpr int kRedSum = 0, kRedFloatSum = 1, kRedMax = 2;   // OP of the kernels

// how MIN / MAX see a value: enc = the order-preserving code of the kind, complemented for MIN
struct RedCodec {
    uint32_t kind, comp;
};

template <typename W, int OP>
__device__ __forceinline__ W red_enc(W b, const RedCodec c)
{
    if constexpr (OP != kRedMax) return b;
    using S = typename std::make_signed<W>::type;
    constexpr int BITS = 8 * (int)sizeof(W);
    constexpr W SIGN = (W)1 << (BITS - 1);
    if (c.kind == (uint32_t)kKeySigned) b ^= SIGN;
    if (c.kind == (uint32_t)kKeyFloat) b ^= (W)((S)b >> (BITS - 1)) | SIGN;
    return c.comp ? (W)~b : b;
}

template <typename W, int OP>
__device__ __forceinline__ W red_dec(W e, const RedCodec c)
{
    if constexpr (OP != kRedMax) return e;
    using S = typename std::make_signed<W>::type;
    constexpr int BITS = 8 * (int)sizeof(W);
    constexpr W SIGN = (W)1 << (BITS - 1);
    if (c.comp) e = (W)~e;
    if (c.kind == (uint32_t)kKeySigned) e ^= SIGN;
    if (c.kind == (uint32_t)kKeyFloat) e ^= (W)((S)(W)~e >> (BITS - 1)) | SIGN;
    return e;
}

template <typename W, int OP>
__device__ __forceinline__ W red_op(W a, W b)
{
    if constexpr (OP == kRedSum) return (W)(a + b);
    else if constexpr (OP == kRedMax) return a > b ? a : b;
    else if constexpr (sizeof(W) == 4) return (W)__float_as_uint(__uint_as_float((uint32_t)a) + __uint_as_float((uint32_t)b));
    else return (W)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
}

// The element of the segmented scan: f = a head lies in the range, v = the range holds an element, cnt = its heads, a = the aggregate
// of its elements from the last head on (of all of them without a head); a means nothing while v is 0.
template <typename W>
struct RedState {
    uint32_t f, v, cnt;
    W a;
};

template <typename W>
__device__ __forceinline__ RedState<W> red_identity()
{
    RedState<W> s;
    s.f = 0u; s.v = 0u; s.cnt = 0u; s.a = (W)0;
    return s;
}

// L in front of R.  Associative, with red_identity on both sides.
template <typename W, int OP>
__device__ __forceinline__ RedState<W> red_combine(const RedState<W> L, const RedState<W> R)
{
    RedState<W> o;
    o.f = L.f | R.f;
    o.cnt = L.cnt + R.cnt;
    if (R.f || !L.v) {
        o.v = R.v; o.a = R.a;
    } else if (!R.v) {
        o.v = L.v; o.a = L.a;
    } else {
        o.v = 1u; o.a = red_op<W, OP>(L.a, R.a);
    }
    return o;
}

// carry (+) the states of the threads in front of this one, in thread order; *total = carry (+) the states of all threads.  Every thread
// calls it; s_wave holds kSelNT / 64 states.
template <typename W, int OP>
__device__ __forceinline__ RedState<W> red_block_scan(const RedState<W> mine, const RedState<W> carry, RedState<W>* s_wave, RedState<W>* total)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    RedState<W> inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        RedState<W> t;
        const uint32_t fv = __shfl_up(inc.f | (inc.v << 1), o);
        t.f = fv & 1u; t.v = fv >> 1;
        t.cnt = __shfl_up(inc.cnt, o);
        t.a = __shfl_up(inc.a, o);
        if (lane >= (uint32_t)o) inc = red_combine<W, OP>(t, inc);
    }
    __syncthreads();   // s_wave may still be read from the call before
    if (lane == 63u) s_wave[w] = inc;
    __syncthreads();
    RedState<W> ex;
    {
        const uint32_t fv = __shfl_up(inc.f | (inc.v << 1), 1);
        ex.f = fv & 1u; ex.v = fv >> 1;
        ex.cnt = __shfl_up(inc.cnt, 1);
        ex.a = __shfl_up(inc.a, 1);
        if (lane == 0u) ex = red_identity<W>();
    }
    RedState<W> p = carry, tot = carry;
#pragma unroll
    for (uint32_t j = 0; j < kSelNT / 64; ++j) {
        const RedState<W> t = s_wave[j];
        if (j < w) p = red_combine<W, OP>(p, t);
        tot = red_combine<W, OP>(tot, t);
    }
    *total = tot;
    return red_combine<W, OP>(p, ex);
}

// the largest v over the workgroup's threads.  Every thread calls it.
__device__ __forceinline__ uint32_t red_block_max(uint32_t v, uint32_t* s_wave)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_xor(v, o);
        v = t > v ? t : v;
    }
    __syncthreads();   // s_wave may still be read from the call before
    if (lane == 0u) s_wave[w] = v;
    __syncthreads();
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < kSelNT / 64; ++j) m = s_wave[j] > m ? s_wave[j] : m;
    return m;
}

template <typename T>
struct alignas(16) RedVec {
    T v[16 / sizeof(T)];
};

// x[e] = src[first + e] for e < cnt (cnt <= kRedItems, first a multiple of kRedItems): 16-byte loads when the thread's items are all there
template <typename T>
__device__ __forceinline__ void red_load(const T* __restrict__ src, size_t first, uint32_t cnt, T (&x)[kRedItems])
{
    constexpr int PER = 16 / (int)sizeof(T);
    if (cnt == (uint32_t)kRedItems) {
#pragma unroll
        for (int u = 0; u < kRedItems / PER; ++u) {
            const RedVec<T> t = *reinterpret_cast<const RedVec<T>*>(src + first + u * PER);
#pragma unroll
            for (int e = 0; e < PER; ++e) x[u * PER + e] = t.v[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) x[e] = (uint32_t)e < cnt ? src[first + e] : (T)0;
    }
}

// This thread's items of one tile: elements first .. first + cnt - 1; returns cnt.  bit e of *heads: item e is a head.  The key in front
// of the first item belongs to another thread, tile or chunk: one scalar load (a line the neighbour's vector load fetches anyway).
template <typename K>
__device__ __forceinline__ uint32_t red_load_keys(const K* __restrict__ keys, uint32_t n, size_t first, K (&k)[kRedItems], uint32_t* heads)
{
    const uint32_t cnt = first >= (size_t)n ? 0u : ((size_t)n - first < (size_t)kRedItems ? (uint32_t)((size_t)n - first) : (uint32_t)kRedItems);
    red_load<K>(keys, first, cnt, k);
    K prev = (K)0;
    if (first > 0 && cnt) prev = keys[first - 1];
    uint32_t h = 0;
#pragma unroll
    for (int e = 0; e < kRedItems; ++e) {
        const bool head = (uint32_t)e < cnt && (first + e == 0 || k[e] != (e ? k[e - 1] : prev));
        h |= (head ? 1u : 0u) << e;
    }
    *heads = h;
    return cnt;
}

// See the head of this file.  keys and vals are 16-byte aligned.
template <typename K, typename W, int OP>
__global__ __launch_bounds__(kSelNT) void reduce_partial_kernel(const K* __restrict__ keys, const W* __restrict__ vals, uint32_t n, uint32_t tiles,
                                                                uint32_t tiles_per_wg, RedCodec codec, uint32_t* __restrict__ chunk_heads,
                                                                uint32_t* __restrict__ chunk_flag, W* __restrict__ chunk_agg)
{
    __shared__ uint32_t s_max[kSelNT / 64];
    __shared__ RedState<W> s_wave[kSelNT / 64];
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    // acc: this thread's elements behind the last head the WORKGROUP has seen; the operators commute, so thread order does not matter
    RedState<W> acc = red_identity<W>();
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const size_t first = (size_t)tile * kRedTile + (size_t)threadIdx.x * kRedItems;
        K k[kRedItems];
        W x[kRedItems];
        uint32_t heads;
        const uint32_t cnt = red_load_keys<K>(keys, n, first, k, &heads);
        red_load<W>(vals, first, cnt, x);
        // 1 + the tile-relative index of the tile's last head, 0 without one
        const uint32_t mine = heads ? threadIdx.x * (uint32_t)kRedItems + (32u - (uint32_t)__clz((int)heads)) : 0u;
        const uint32_t last = red_block_max(mine, s_max);
        if (last) {
            acc.f = 1u;
            acc.v = 0u;
        }
        acc.cnt += (uint32_t)__popc(heads);
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            if ((uint32_t)e < cnt && threadIdx.x * (uint32_t)kRedItems + e + 1u >= last) {
                const W c = red_enc<W, OP>(x[e], codec);
                acc.a = acc.v ? red_op<W, OP>(acc.a, c) : c;
                acc.v = 1u;
            }
        }
    }
    // (+) of the accumulators alone: their f stays out of it
    RedState<W> mine = acc, total;
    mine.f = 0u;
    (void)red_block_scan<W, OP>(mine, red_identity<W>(), s_wave, &total);
    if (threadIdx.x == 0) {
        chunk_heads[blockIdx.x] = total.cnt;
        chunk_flag[blockIdx.x] = acc.f;   // (uniform over the workgroup)
        chunk_agg[blockIdx.x] = total.a;  // codes for MIN / MAX
    }
}

// One workgroup.  chunk_heads[w] becomes the heads in front of chunk w, *num_runs their total, chunk_carry[w] the aggregate in front of
// chunk w of the run open at its start (w > 0).  Thread t owns the chunks [t * per, (t + 1) * per).
template <typename W, int OP>
__global__ __launch_bounds__(kSelNT) void reduce_carry_kernel(uint32_t* __restrict__ chunk_heads, const uint32_t* __restrict__ chunk_flag,
                                                              const W* __restrict__ chunk_agg, W* __restrict__ chunk_carry, uint32_t chunks,
                                                              uint32_t* __restrict__ num_runs)
{
    __shared__ RedState<W> s_wave[kSelNT / 64];
    const uint32_t per = (chunks + (uint32_t)kSelNT - 1u) / (uint32_t)kSelNT;
    const uint32_t c0 = threadIdx.x * per < chunks ? threadIdx.x * per : chunks;
    const uint32_t c1 = c0 + per < chunks ? c0 + per : chunks;
    RedState<W> mine = red_identity<W>();
    for (uint32_t c = c0; c < c1; ++c) {
        RedState<W> s;
        s.f = chunk_flag[c]; s.v = 1u; s.cnt = chunk_heads[c]; s.a = chunk_agg[c];
        mine = red_combine<W, OP>(mine, s);
    }
    RedState<W> total;
    RedState<W> p = red_block_scan<W, OP>(mine, red_identity<W>(), s_wave, &total);
    for (uint32_t c = c0; c < c1; ++c) {
        RedState<W> s;
        s.f = chunk_flag[c]; s.v = 1u; s.cnt = chunk_heads[c]; s.a = chunk_agg[c];
        chunk_heads[c] = p.cnt;
        chunk_carry[c] = p.a;   // (meaningless for chunk 0, which reads no carry)
        p = red_combine<W, OP>(p, s);
    }
    if (threadIdx.x == 0) *num_runs = total.cnt;
}

// chunk_base[w] = the heads in front of workgroup w's chunk, chunk_carry[w] as reduce_carry_kernel wrote it.  unique_out and reduced_out
// are required, offsets is written where given.  Elements at R and beyond (offsets: R + 1) are never written.
template <typename K, typename W, int OP>
__global__ __launch_bounds__(kSelNT) void reduce_emit_kernel(const K* __restrict__ keys, const W* __restrict__ vals, uint32_t n, uint32_t tiles,
                                                             uint32_t tiles_per_wg, RedCodec codec, const uint32_t* __restrict__ chunk_base,
                                                             const W* __restrict__ chunk_carry, K* __restrict__ unique_out,
                                                             W* __restrict__ reduced_out, uint32_t* __restrict__ offsets)
{
    __shared__ RedState<W> s_wave[kSelNT / 64];
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = t0 + tiles_per_wg < tiles ? t0 + tiles_per_wg : tiles;
    // the elements of this chunk in front of the current tile, behind everything in front of the chunk: cnt = the heads in front of the
    // tile, a = the aggregate of the open run so far
    RedState<W> carry;
    carry.f = 0u;
    carry.v = blockIdx.x > 0 ? 1u : 0u;
    carry.cnt = chunk_base[blockIdx.x];
    carry.a = blockIdx.x > 0 ? chunk_carry[blockIdx.x] : (W)0;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const size_t first = (size_t)tile * kRedTile + (size_t)threadIdx.x * kRedItems;
        K k[kRedItems];
        W x[kRedItems];
        uint32_t heads;
        const uint32_t cnt = red_load_keys<K>(keys, n, first, k, &heads);
        red_load<W>(vals, first, cnt, x);
        // the key behind the last item belongs to another thread, tile or chunk: the mirror of the load in red_load_keys
        const bool more = first + kRedItems < (size_t)n;
        K next = (K)0;
        if (more) next = keys[first + kRedItems];
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
            mine.cnt += head ? 1u : 0u;
        }
        RedState<W> total;
        const RedState<W> p = red_block_scan<W, OP>(mine, carry, s_wave, &total);
        uint32_t h = p.cnt;   // heads in front of the item
        bool open = p.v;      // the run of the item began in front of this thread, and p.a holds its elements so far
#pragma unroll
        for (int e = 0; e < kRedItems; ++e) {
            if ((uint32_t)e >= cnt) continue;
            const bool head = (heads >> e) & 1u;
            if (head) {
                open = false;
                if (h < n) {   // (never false: there are at most n heads)
                    unique_out[h] = k[e];
                    if (offsets) offsets[h] = (uint32_t)(first + e);
                }
                ++h;
            }
            const bool tail = e + 1 < kRedItems ? ((uint32_t)(e + 1) >= cnt || ((heads >> (e + 1)) & 1u)) : (!more || next != k[e]);
            if (tail && h - 1u < n) {   // (position 0 is a head, so h >= 1 here)
                const W r = open ? red_op<W, OP>(p.a, x[e]) : x[e];
                reduced_out[h - 1u] = red_dec<W, OP>(r, codec);
            }
        }
        carry = total;
        carry.f = 0u;
    }
    // the last workgroup holds position n - 1: carry.cnt is R now
    if (offsets && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && carry.cnt <= n) offsets[carry.cnt] = n;
}

}  // namespace adlhip
