// finish16_kernels.hpp -- gfx950 device code: the LDS finish of the large keys-only sort for whole u32 keys (round 4).
//
// After the two MSD passes a segment slab holds the low 16 bits of ~n / 65536 keys (uint16_t; the bits above are the segment's
// number).  ONE WAVE sorts one segment, as wave_segment_sort_kernel (hybrid_kernels.hpp) does -- stable 8-bit LSD passes in the
// wave's own slice of LDS, no workgroup barrier -- but the keys stay 16 bits wide all the way:
//   * they are loaded two to a dword (half the load instructions) and live two to a register;
//   * the LDS tile holds uint16_t (3 KiB instead of 6 for 1536 keys: the wave slots, not the LDS, bound the occupancy) in an
//     interleaved order -- position p sits at index (p / 128) * 128 + (p % 64) * 2 + (p / 64) % 2 -- so that ONE ds_read_b32 per lane
//     brings back rows 2j and 2j + 1 (positions 128 j + lane and 128 j + 64 + lane): half the read-backs, and the final stores are
//     still one dword per lane to consecutive addresses.
// The counters of round 3 (profiles/r3_pmc_msd2_u32_all_counters.txt) put the old finish at 72 % LDS-busy with 61 % of those cycles in
// bank conflicts; conflicts of 64 random bins over 32 banks cannot be laid out away, so what this kernel buys is fewer LDS
// instructions per key and more waves in flight to keep the LDS pipe full while others wait for memory.
//
// Per pass ONE returning atomic per key counts its bin and ranks the key (its arrival number inside its bin, in position order); a
// scan turns the counts into bin starts, and slot = bin start + rank.  The bin starts are gathered with plain LDS reads (a gather is
// cheaper than a second atomic, tools/r4_lds_bench; the compiler keeps eight ahead of their 16-bit stores, counted lgkmcnt waits):
// read through a volatile pointer, which the compiler cannot place in LDS, they were a FLAT load and a full wait per key -- 64 Mi keys
// 0.102 -> 0.096-0.097 ms per launch (CHANGELOG.md, "the 16-bit finish gathers its bin starts from LDS", records the variants that
// were compared).  The slab is loaded and the result stored non-temporally: neither is read again.  The LDS array is the limit --
// SQ_LDS_IDX_ACTIVE is 186 K cycles per CU, 62 % of them bank conflicts of the returning atomics, the gathers and the 16-bit scatter
// -- and what was tried on top changed nothing: 8 waves per SIMD instead of 5 (bounded batches of ranks and gathers, digits
// recomputed: 63 VGPRs), a prologue of one round trip, a tile index of four instructions instead of eight (profiles/finish16_ab.txt,
// finish16_pmc.txt).
//
// So the LDS cycles themselves had to go.  Where more than 8 bits are left to sort -- where the LSD code runs two passes -- ONE pass
// (finish16_bins) places the keys by the top kFinish16BinBits = 9 bits of what is left, 512 bins, not stably (equal keys of a
// key-only sort are indistinguishable), into a blocked layout: lane l owns 2 RR consecutive positions at an odd dword stride
// (finish16_block_byte), so that every lane reads its own block back without a bank conflict.  A bin of uniform keys holds 2-3 keys,
// the largest of a segment 7-8 (12 at most in simulation), and what shares a bin is ordered in registers: M rounds of odd-even
// transposition on whole 16-bit keys, M = the segment's largest bin, v_min_u32 / v_max_u32 between neighbouring registers and one
// DPP wave shift per direction for the pair that straddles two lanes.  The sorted block goes back to the tile and is read out in
// rows of 64 for the same stores as before.  A segment whose keys all share one bin, or whose largest bin exceeds
// kFinish16MaxRounds = 24, takes the LSD passes below on the keys it still holds; it has paid the ranking (one atomic per key) by
// then.  64 Mi keys: 0.096 -> 0.076-0.077 ms per launch, SQ_LDS_IDX_ACTIVE 186 K -> 124 K cycles per CU, SQ_INSTS_VALU 37.3 M ->
// 27.9 M (CHANGELOG.md, "the 16-bit finish places once and orders its bins in registers"; profiles/finish16_bins_ab.txt,
// finish16_bins_pmc.txt).  At 403 MB in 0.077 ms the kernel now moves 5.3 TB/s: neither the LDS array (about two thirds busy) nor the
// VALU is the limit any more.
// LDS per wave: 256 (R2 | 1) bytes of tile + 2 KiB of counters = <10,4> 4864, <12,4> 5376, <20,4> 7424 bytes; the VGPRs, not the LDS,
// bound the resident waves.  Registers: <10,4> 73, <12,4> 86, <20,4> 125 VGPRs (6, 5 and 4 waves per SIMD), no scratch, no FLAT load.
// What the wave's LDS accesses may assume of each other is written down once, at finish16_lds_order().
//
// Reference behaviour: Tahoe/ClKernels/RadixSort32Kernels.cl:401-489 (sort4Bits1: the stable local sort of a block).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hybrid_kernels.hpp"

namespace adlhip {

constexpr int kFinish16BinBits = 9;      // B: the one LDS pass of the fast path places the keys by their top B bits
constexpr int kFinish16MaxRounds = 24;   // a segment whose largest bin holds more keys takes the two LSD passes instead

template <int R2>
struct Finish16Cfg {
    static constexpr int CAP = 128 * R2;                     // keys a wave's tile holds
    static constexpr int BINS = 1 << kFinish16BinBits;
    static constexpr size_t TILE = 256 * (R2 | 1);           // bytes: 64 lanes x an odd number of dwords (finish16_block_byte)
    static constexpr size_t PER_WAVE = TILE + 4 * BINS;      // tile + counters
};

__device__ __forceinline__ uint32_t finish16_index(uint32_t p) { return (p & ~127u) | ((p & 63u) << 1) | ((p >> 6) & 1u); }

// The ordering contract of a wave's slice of LDS.  One wave owns the tile and the counters; the hardware executes a wave's DS
// operations in the order they were issued, so a lane that reads what another lane of the same wave wrote needs no wait and no
// barrier -- only that the compiler ISSUES the write first.  Nothing in the types says so: the tile is written as uint16_t and read
// back as uint32_t (strict aliasing lets the loads move above the stores), and the bin starts are written as one u32x4 per lane and
// gathered by other lanes.  This point is that promise: no LDS access moves across it.  It emits no instruction.
__device__ __forceinline__ void finish16_lds_order() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// The blocked layout of the fast path: lane l owns the J = 2 RR consecutive positions [l J, (l + 1) J), RR dwords at a lane stride of
// RR | 1 dwords.  An odd stride puts the 32 lanes of a ds_read_b32 / ds_write_b32 group on 32 different banks; 64 consecutive
// positions (the scatter's pads, the striped read-out) touch at most 32 + 64 / J consecutive dwords.  Returns the byte offset.
template <int RR>
__device__ __forceinline__ uint32_t finish16_block_byte(uint32_t p)
{
    constexpr uint32_t J = 2 * RR;
    if constexpr ((RR & 1) != 0) {
        return 2u * p;
    } else if constexpr ((J & (J - 1)) == 0) {
        return 2u * p + 4u * (p / J);
    } else {   // p / J for p < 64 J <= 2560 as a 24-bit multiply and a shift: exact while p (MAGIC J - 65536) < 65536
        constexpr uint32_t MAGIC = (65536u + J - 1u) / J;
        static_assert(64u * J * (MAGIC * J - 65536u) < 65536u, "the reciprocal is not exact over the tile");
        return 2u * p + 4u * (__umul24(p, MAGIC) >> 16);
    }
}

// the largest value of the wave, in every lane; all 64 lanes must be active (the DPP steps of wave_incl_scan_u32 with max for +)
__device__ __forceinline__ uint32_t finish16_wave_max(uint32_t v)
{
    v = max(v, dpp_mov0<0x111, 0xf, 0xf>(v));
    v = max(v, dpp_mov0<0x112, 0xf, 0xf>(v));
    v = max(v, dpp_mov0<0x114, 0xf, 0xf>(v));
    v = max(v, dpp_mov0<0x118, 0xf, 0xf>(v));
    v = max(v, dpp_mov0<0x142, 0xa, 0xf>(v));
    v = max(v, dpp_mov0<0x143, 0xc, 0xf>(v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// The fast path (low_bits > 8, where the LSD code below runs two passes): ONE LDS pass places the keys by their top
// min(B, low_bits) bits -- not stably: equal keys are indistinguishable -- into the blocked layout, every lane reads its J keys
// back and M rounds of odd-even transposition in registers order what shares a bin (M = the largest bin of the segment: keys of
// different bins are in order already, so every bin is a run of its own and a run of length L is sorted after L rounds, whichever
// parity it starts on).  Positions [m, 64 J) are padded with 0xffff, which no compare-exchange moves below a key.  Returns false
// with kp[] and the tile's meaning untouched when the LSD code has to run: every key in one bin, or M > kFinish16MaxRounds.
template <int RR>
__device__ __forceinline__ bool finish16_bins(const uint32_t (&kp)[RR], uint32_t* __restrict__ out, uint32_t m, int lane,
                                              uint16_t* __restrict__ buf16, uint32_t* __restrict__ cnt, uint32_t low_bits, uint32_t hi,
                                              bool a_lo, bool a_hi, bool b_lo, bool b_hi)
{
    constexpr int L = RR - 1, J = 2 * RR, S = RR | 1;
    constexpr int NB = 1 << kFinish16BinBits, PL = NB / 64;   // counters, counters per lane
    static_assert(PL % 4 == 0, "a lane scans its counters as u32x4");
    const uint32_t bb = low_bits < (uint32_t)kFinish16BinBits ? low_bits : (uint32_t)kFinish16BinBits;
    const uint32_t sh = low_bits - bb;   // <= 16 - B: the digit of either half lies inside its half
    auto dlo = [&](uint32_t x) -> uint32_t { return (x >> sh) & (uint32_t)(NB - 1); };
    auto dhi = [&](uint32_t x) -> uint32_t { return (x >> (16u + sh)) & (uint32_t)(NB - 1); };
    {   // every key in one bin: all 64 lanes of every atomic would queue on ONE counter, and the LSD code knows what to skip
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dlo(kp[0]));
        bool same = true;
#pragma unroll
        for (int j = 0; j < RR; ++j) {
            if (j < L || a_lo) same &= dlo(kp[j]) == d0;
            if (j < L || a_hi) same &= dhi(kp[j]) == d0;
        }
        if (__all(same)) return false;
    }
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < PL / 4; ++q) *reinterpret_cast<u32x4*>(cnt + PL * lane + 4 * q) = z;
    uint32_t rk[RR];   // the two ranks of a register's keys, in whatever order the atomics of a bin were served
#pragma unroll
    for (int j = 0; j < RR; ++j) {
        uint32_t r0 = 0u, r1 = 0u;
        if (j < L || a_lo) r0 = __hip_atomic_fetch_add(&cnt[dlo(kp[j])], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (j < L || a_hi) r1 = __hip_atomic_fetch_add(&cnt[dhi(kp[j])], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        rk[j] = r0 | (r1 << 16);
    }
    const bool tail = low_bits > bb;   // otherwise the bin is the whole key
    uint32_t rounds;
    {   // counts -> bin starts, and the largest count
        u32x4 c[PL / 4];
        uint32_t sum = 0u, big = 0u;
#pragma unroll
        for (int q = 0; q < PL / 4; ++q) {
            c[q] = *reinterpret_cast<const u32x4*>(cnt + PL * lane + 4 * q);
            sum += c[q].x + c[q].y + c[q].z + c[q].w;
            big = max(max(big, max(c[q].x, c[q].y)), max(c[q].z, c[q].w));
        }
        rounds = finish16_wave_max(big);
        if (tail && rounds > (uint32_t)kFinish16MaxRounds) return false;
        uint32_t run = wave_incl_scan_u32(sum) - sum;
#pragma unroll
        for (int q = 0; q < PL / 4; ++q) {
            u32x4 o;
            o.x = run;
            o.y = o.x + c[q].x;
            o.z = o.y + c[q].y;
            o.w = o.z + c[q].z;
            run = o.w + c[q].w;
            *reinterpret_cast<u32x4*>(cnt + PL * lane + 4 * q) = o;
        }
    }
    unsigned char* tile = reinterpret_cast<unsigned char*>(buf16);
    const bool sort = tail && rounds > 1u;   // wave-uniform
    if (sort) {   // the pads: positions [m, 64 J) are at most 128, since m > 128 (RR - 1)
        const uint32_t p0 = m + (uint32_t)lane, p1 = p0 + 64u;
        if (p0 < (uint32_t)(64 * J)) *reinterpret_cast<uint16_t*>(tile + finish16_block_byte<RR>(p0)) = (uint16_t)0xffffu;
        if (p1 < (uint32_t)(64 * J)) *reinterpret_cast<uint16_t*>(tile + finish16_block_byte<RR>(p1)) = (uint16_t)0xffffu;
    }
    finish16_lds_order();   // the bin starts are written before any lane gathers one
#pragma unroll
    for (int j = 0; j < RR; ++j) {   // slot = bin start (a plain LDS read) + rank
        uint32_t p0 = 0u, p1 = 0u;
        if (j < L || a_lo) p0 = cnt[dlo(kp[j])] + (rk[j] & 0xffffu);
        if (j < L || a_hi) p1 = cnt[dhi(kp[j])] + (rk[j] >> 16);
        if (j < L || a_lo) *reinterpret_cast<uint16_t*>(tile + finish16_block_byte<RR>(p0)) = (uint16_t)kp[j];
        if (j < L || a_hi) *reinterpret_cast<uint16_t*>(tile + finish16_block_byte<RR>(p1)) = (uint16_t)(kp[j] >> 16);
    }
    finish16_lds_order();   // the 16-bit stores of the tile are issued before any lane reads what others placed
    if (sort) {
        uint32_t* own = reinterpret_cast<uint32_t*>(tile) + S * lane;
        uint32_t k[J];
#pragma unroll
        for (int j = 0; j < RR; ++j) {
            const uint32_t w = own[j];
            k[2 * j] = w & 0xffffu;
            k[2 * j + 1] = w >> 16;
        }
        for (uint32_t r = 0u; r < rounds; r += 2u) {
#pragma unroll
            for (int j = 0; j < RR; ++j) {   // pairs (0,1), (2,3), ... inside the lane
                const uint32_t a = k[2 * j], b = k[2 * j + 1];
                k[2 * j] = min(a, b);
                k[2 * j + 1] = max(a, b);
            }
            // pairs (1,2), (3,4), ... and the lane's last key against the next lane's first (wave_shl:1 / wave_shr:1: lane l
            // receives from lane l + 1 / l - 1; the edge lanes keep `old`, which their key beats)
            const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp((int)0xffffffffu, (int)k[0], 0x130, 0xf, 0xf, false);
            const uint32_t dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)k[J - 1], 0x138, 0xf, 0xf, false);
#pragma unroll
            for (int j = 0; j < RR - 1; ++j) {
                const uint32_t a = k[2 * j + 1], b = k[2 * j + 2];
                k[2 * j + 1] = min(a, b);
                k[2 * j + 2] = max(a, b);
            }
            k[J - 1] = min(k[J - 1], up);
            k[0] = max(k[0], dn);
        }
#pragma unroll
        for (int j = 0; j < RR; ++j) own[j] = k[2 * j] | (k[2 * j + 1] << 16);
        finish16_lds_order();   // the sorted block is written before the striped read-out
    }
#pragma unroll
    for (int i = 0; i < J; ++i) {   // row i = positions 64 i + lane: one dword per lane to consecutive addresses
        if (i < 2 * L || (i == 2 * L ? b_lo : b_hi)) {
            const uint32_t p = (uint32_t)(64 * i + lane);
            const uint32_t v = *reinterpret_cast<const uint16_t*>(tile + finish16_block_byte<RR>(p));
            __builtin_nontemporal_store(hi | v, out + p);
        }
    }
    return true;
}

// RR row pairs; the first RR - 1 are full (m > 128 (RR - 1)), only the last is tested per lane
template <int RR>
__device__ __forceinline__ void finish16_rows(const uint32_t* __restrict__ src32, uint32_t* __restrict__ out, uint32_t m, int lane,
                                              uint16_t* __restrict__ buf16, uint32_t* __restrict__ cnt, uint32_t low_bits, uint32_t hi)
{
    constexpr int L = RR - 1;
    // as loaded: dword i = 64 j + lane holds keys 2 i and 2 i + 1; after a pass: positions 128 j + lane and 128 j + 64 + lane
    const bool a_lo = 2u * (uint32_t)(64 * L + lane) < m, a_hi = 2u * (uint32_t)(64 * L + lane) + 1u < m;
    const bool b_lo = (uint32_t)(128 * L + lane) < m, b_hi = (uint32_t)(128 * L + 64 + lane) < m;
    uint32_t kp[RR];
#pragma unroll
    for (int j = 0; j < RR; ++j)
        if (j < L || a_lo) kp[j] = __builtin_nontemporal_load(src32 + j * 64 + lane);
    if (low_bits > 8u && finish16_bins<RR>(kp, out, m, lane, buf16, cnt, low_bits, hi, a_lo, a_hi, b_lo, b_hi)) return;
    bool placed = false;   // wave-uniform: the keys sit in position order (a pass has run)
    const int npass = ((int)low_bits + 7) / 8;
    int sb = 0;
    const uint32_t* buf32 = reinterpret_cast<const uint32_t*>(buf16);
    for (int p = 0; p < npass; ++p) {
        const int nb = ((int)low_bits - sb + (npass - p - 1)) / (npass - p);
        const uint32_t mask = (1u << nb) - 1u;
        const bool v_lo = placed ? b_lo : a_lo, v_hi = placed ? b_hi : a_hi;
        auto dlo = [&](uint32_t x) -> uint32_t { return (x >> sb) & mask; };
        auto dhi = [&](uint32_t x) -> uint32_t { return (x >> (16 + sb)) & mask; };
        {   // a pass in which every key has the same digit changes nothing -- and would queue all 64 lanes of every atomic on ONE counter
            const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dlo(kp[0]));
            bool same = true;
#pragma unroll
            for (int j = 0; j < RR; ++j) {
                if (j < L || v_lo) same &= dlo(kp[j]) == d0;
                if (j < L || v_hi) same &= dhi(kp[j]) == d0;
            }
            if (__all(same)) {
                sb += nb;
                continue;
            }
        }
        const u32x4 z = {0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(cnt + 4 * lane) = z;
        uint32_t rk[RR];   // the two ranks of a register's keys
#pragma unroll
        for (int j = 0; j < RR; ++j) {   // position order: row 2j before row 2j + 1, colliding lanes in lane order (stable)
            uint32_t r0 = 0u, r1 = 0u;
            if (j < L || v_lo) r0 = __hip_atomic_fetch_add(&cnt[dlo(kp[j])], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            if (j < L || v_hi) r1 = __hip_atomic_fetch_add(&cnt[dhi(kp[j])], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            rk[j] = r0 | (r1 << 16);
        }
        {   // counts -> bin starts
            const u32x4 c = *reinterpret_cast<const u32x4*>(cnt + 4 * lane);
            const uint32_t s4 = c.x + c.y + c.z + c.w;
            const uint32_t ex = wave_incl_scan_u32(s4) - s4;
            u32x4 o;
            o.x = ex;
            o.y = ex + c.x;
            o.z = o.y + c.y;
            o.w = o.z + c.z;
            *reinterpret_cast<u32x4*>(cnt + 4 * lane) = o;
        }
        finish16_lds_order();   // the bin starts are written before any lane gathers one
#pragma unroll
        for (int j = 0; j < RR; ++j) {   // slot = bin start (a plain LDS read) + rank
            uint32_t p0 = 0u, p1 = 0u;
            if (j < L || v_lo) p0 = cnt[dlo(kp[j])] + (rk[j] & 0xffffu);
            if (j < L || v_hi) p1 = cnt[dhi(kp[j])] + (rk[j] >> 16);
            if (j < L || v_lo) buf16[finish16_index(p0)] = (uint16_t)kp[j];
            if (j < L || v_hi) buf16[finish16_index(p1)] = (uint16_t)(kp[j] >> 16);
        }
        finish16_lds_order();   // the 16-bit stores of the tile are issued before its 32-bit read-back
#pragma unroll
        for (int j = 0; j < RR; ++j)
            if (j < L || b_lo) kp[j] = buf32[j * 64 + lane];
        placed = true;
        sb += nb;
    }
    if (placed) {
#pragma unroll
        for (int j = 0; j < RR; ++j) {
            if (j < L || b_lo) __builtin_nontemporal_store(hi | (kp[j] & 0xffffu), out + 128 * j + lane);
            if (j < L || b_hi) __builtin_nontemporal_store(hi | (kp[j] >> 16), out + 128 * j + 64 + lane);
        }
    } else {   // no pass had anything to do: every key of the segment is the same, any order will do
#pragma unroll
        for (int j = 0; j < RR; ++j) {
            if (j < L || a_lo) out[2 * (64 * j + lane)] = hi | (kp[j] & 0xffffu);
            if (j < L || a_hi) out[2 * (64 * j + lane) + 1] = hi | (kp[j] >> 16);
        }
    }
}

template <int RR, int R2>
__device__ __forceinline__ void finish16_dispatch(int rows2, const uint32_t* __restrict__ src32, uint32_t* __restrict__ out, uint32_t m,
                                                  int lane, uint16_t* __restrict__ buf16, uint32_t* __restrict__ cnt, uint32_t low_bits,
                                                  uint32_t hi)
{
    if constexpr (RR >= R2) {
        finish16_rows<R2>(src32, out, m, lane, buf16, cnt, low_bits, hi);
    } else {
        if (rows2 <= RR) finish16_rows<RR>(src32, out, m, lane, buf16, cnt, low_bits, hi);
        else finish16_dispatch<RR + 1, R2>(rows2, src32, out, m, lane, buf16, cnt, low_bits, hi);
    }
}

// slab: 65536 segment slabs of `stride` uint16_t (stride even); segment s holds seg_cnt[s] keys and goes to out[seg_off[s] ...).
// dyn[0] = bits the finish sorts (<= 16), dyn[1] = the keys' common prefix above the two digits (msd2_offsets_kernel).
template <int R2, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void wave_finish16_kernel(const uint16_t* __restrict__ slab, uint32_t* __restrict__ out,
                                                                    const uint32_t* __restrict__ seg_off,
                                                                    const uint32_t* __restrict__ seg_cnt, uint32_t stride,
                                                                    const uint32_t* __restrict__ gate, const uint32_t* __restrict__ dyn,
                                                                    uint32_t num_segments, uint32_t* fault)
{
    if (gate && *gate != 0u) return;
    using C = Finish16Cfg<R2>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = (int)threadIdx.x & 63;
    const int w = (int)threadIdx.x >> 6;
    unsigned char* mine = smem + (size_t)w * C::PER_WAVE;
    uint16_t* __restrict__ buf16 = reinterpret_cast<uint16_t*>(mine);
    uint32_t* __restrict__ cnt = reinterpret_cast<uint32_t*>(mine + C::TILE);
    const uint32_t seg = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (uint32_t)WAVES + (uint32_t)w));
    if (seg >= num_segments) return;
    const uint32_t low_bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)dyn[0]);
    const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg_cnt[seg]);
    const uint32_t begin = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg_off[seg]);
    if (m == 0u) return;
    if (m > (uint32_t)C::CAP || low_bits > 16u) {   // never sort wrongly in silence
        if (lane == 0) atomicOr(fault + 1, 0x40000u);
        return;
    }
    const uint32_t hi = ((dyn[1] << 16) | seg) << low_bits;
    const uint32_t* src32 = reinterpret_cast<const uint32_t*>(slab + (size_t)seg * stride);
    finish16_dispatch<1, R2>((int)((m + 127u) >> 7), src32, out + begin, m, lane, buf16, cnt, low_bits, hi);
}

}   // namespace adlhip
