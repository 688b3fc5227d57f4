// large_plan.hpp -- the large sort's host arithmetic: its size limits, the slab and tile sizes, the two work-buffer layouts, which form
// a sort takes (large_sort_form) and, from all of that, the ONE plan of a sort call (large_plan) and the large sort's term of the
// scratch query (large_work_bytes_at).  Host only and nothing that launches: no kernel header, no HIP call; adlhip.hip is its one
// user in the library, and tests/large_plan_dump.cpp compiles it with a plain host compiler.
#pragma once
#include "adlhip_internal.hpp"

namespace adlhip_internal {

// ---- small inputs: the whole sort in one workgroup (adlhip.hip small_sort) ---------------------------------------------------------
constexpr size_t kSmallMax = 16384;

// ---- large keys-only sort: two unstable MSD passes with bucket cursors + LDS finish (hybrid_kernels.hpp "sort.msd2") ------
// u32 keys and u64 keys (equal keys are indistinguishable, so the passes need not be stable); pairs keep the stable paths.
constexpr size_t kMsd2Min = kSmallMax;                             // elements; the path works from here ("sort.msd2" >= 2) ...
constexpr size_t kMsd2AutoMin = size_t(2) << 20;                   // ... and is chosen above the mid-size sort's range
                                                                   // (profiles/r2_msd2_size_curve.txt: 2.5 Mi keys 58 vs 70 us)
// up to 280 Mi keys a segment (mean n / 65536 = 4480, + 7.5 sd <= 5120) fits the 80 rows one wave holds; beyond, the finish takes one
// workgroup per segment (wg_segment_sort_kernel: tiles of 8192 ... 20480 keys) up to a mean of 17408 + 7.5 sd
constexpr size_t kMsd2MaxU32 = size_t(1088) << 20;
constexpr size_t kMsd2MaxU64 = (size_t(1) << 28) + (size_t(1) << 22);   // mean segment 4160
// the wave-per-segment finish's tiles: 64 * 20, 64 * 40, 64 * 80 elements

// from here the 16-bit second slab of whole u32 keys always fits the caller's n-element scratch array (1.5 x the mean + 72 per
// segment <= 2 x the mean); one fixed threshold keeps the work requirement piecewise monotone in n (sort_work_bytes' edges)
constexpr size_t kSlabInTmpMin = size_t(16) << 20;

// ---- the same for {key, value} pairs, STABLE: look-back instead of cursors (hybrid_kernels.hpp msd_lookback_scatter_kernel) --
constexpr size_t kMsd2sAutoMin = size_t(1) << 20;   // pairs; measured with the narrow second digit: 1.5 Mi pairs 55 vs 89 us (three-kernel
                                                    // passes), 4 Mi 89 vs 105, 8 Mi 135 vs 183 (profiles/r3_narrow_second_digit.txt)
constexpr size_t kMsd2sMax = (size_t(1) << 28) + (size_t(1) << 22);
// tile of the look-back passes: TileCfg<uint64_t, 8, 512, 16> = 8192 pairs, TileCfg<uint32_t, 8, 512, 32> = 16384 keys
constexpr uint32_t msd2s_tile(size_t elem_bytes) { return elem_bytes == 8 ? 8192u : 16384u; }
// u32 words between two chains' ticket counters.  adlhip.hip asserts that it is the kernels' (adlhip::kTicketStride, onesweep_kernels.hpp)
constexpr int kLargeTicketStride = 32;

// ---- the three conditions every decision below shares, each written once -----------------------------------------------------------
// whole u32 keys get the 16-bit second slab (the stable form then keeps 65536 segments; the cursor form has it where its second
// digit is 8 bits wide)
constexpr bool large_slab16(size_t elem_bytes, bool whole) { return elem_bytes == 4 && whole; }
// the cursor form sorts whole keys (the element is the key), up to the size its finish's tiles reach
constexpr size_t cursor_max(size_t elem_bytes) { return elem_bytes == 4 ? kMsd2MaxU32 : kMsd2MaxU64; }
constexpr bool cursor_eligible(size_t elem_bytes, bool keys, bool whole, size_t n) { return keys && whole && n <= cursor_max(elem_bytes); }
// the stable form (and the hybrid form, whose first pass is the stable one)
constexpr bool stable_eligible(size_t n) { return n <= kMsd2sMax; }

// slab of a segment = the smallest of the finish's tiles that holds its mean + 7.5 standard deviations of a uniform key
// distribution (64 Mi keys: 1024 + 240 = 1264, slab 1536; a segment beyond its slab sends the sort to the safety net, it is never
// wrong; at 7.5 sd that is one sort in 10^8)
// slab and finish tile of the first tier: 64 * 24 elements.  With 64 * 20 = 1280 (mean 1024 at 64 Mi keys + 7.5 sd) keys whose
// density varied by 20 % over the key range already went to the safety net; 1536 takes ~45 % and costs nothing measurable
// (finish 118.0 vs 118.3 us at 64 Mi keys: five workgroups of four waves per CU instead of three of eight)
constexpr uint32_t kMsd2Stride0 = 1536;
// tile of the finish for n elements: 1280 / 1536 / 2560 / 5120 (what a wave -- or a workgroup of the binning finish -- holds),
// 8192 ... 20480 for the workgroup-per-segment finish
// fine: whole u32 keys with a 16-bit second slab -- from 2560 keys up their finish is the workgroup kernel, which has tiles of 3072
// and 4096 keys too (a half-empty 5120-key tile costs its 20 predicated rows all the same: 144 Mi keys 0.35 ms for the finish)
inline uint32_t msd2_tier_b(size_t n, uint32_t slots = 65536, bool fine = false)
{
    const size_t mean = (n + slots - 1) / slots;
    size_t sd = 1;
    while (sd * sd < mean) ++sd;
    const size_t need = mean + (15 * sd + 1) / 2;
    if (fine && need > 2560 && need <= 4096) return need <= 3072 ? 3072u : 4096u;
    // (the tiers' bounds on the mean stay as they were; up to a mean of ~640 the 1280-element tile already leaves 1.5 x)
    if (need <= 5120) return need <= 832 ? 1280u : need <= 1280 ? kMsd2Stride0 : need <= 2560 ? 2560u : 5120u;
    // (u32 keys beyond 280 Mi only: the workgroup-per-segment finish, 512 threads x 16 / 24 rows, 1024 x 16 / 20)
    return need <= 8192 ? 8192u : need <= 12288 ? 12288u : need <= 16384 ? 16384u : 20480u;
}
// elements between two segment slabs: the mean + 50 % (or + 7.5 sd where that is more), at most the finish's tile.  (Round 2 spaced
// the slabs by the tile whatever n was: 168 MB of second slab for 2 Mi keys.)
inline uint32_t msd2_stride_b(size_t n, uint32_t slots = 65536, bool fine = false, bool lean = false)
{
    const size_t mean = (n + slots - 1) / slots;
    size_t sd = 1;
    while (sd * sd < mean) ++sd;
    // lean (level 2 of adlhip_radix_sort_scratch_bytes_for, stable form): the mean + 7.5 sd only -- what evenly spread keys need
    const size_t want = align_up(std::max(lean ? mean : mean + mean / 2, mean + (15 * sd + 1) / 2) + 8, 64);
    return (uint32_t)std::min<size_t>(want, msd2_tier_b(n, slots, fine));
}

// Width w of the second digit of the cursor form (hybrid_kernels.hpp slot_to_segment): 8 from 12 Mi elements up; below, as many
// bits as leave segments of about a thousand elements -- 256 << w slots instead of 65536.  The finish then sorts 8 - w bits more
// (u32 keys: more than 16, so the second slab holds whole keys), which costs less than launching 65536 waves for a few dozen
// keys each (profiles/r3_narrow_second_digit.txt).
// Measured (cursor form, 65536 segments | narrow): u32 keys 2.5 Mi 71 | 51 us, 4 Mi 81 | 58, 8 Mi 104 | 91, 16 Mi 140 | 138, 24 Mi
// 177 | 199; u64 keys (binning finish on the ~1000-key segments) 1.5 Mi 117 | 47 us, 4 Mi 154 | 79, 16 Mi 289 | 221, 24 Mi 397 | 346.
// bin_finish: the segments go to the binning finish (whole u64 keys, cursor form), which likes them a thousand keys long at any n;
// the LSD finish pays for every extra bit with LDS passes, so there the narrow digit stops at 16 Mi elements.
inline uint32_t msd2_seg_shift(size_t n, bool bin_finish)
{
    const size_t max_n = bin_finish ? size_t(1) << 40 : size_t(16) << 20;
    if (n >= max_n) return 8u;
    uint32_t w = 2u;
    while (w < 8u && (n >> (8u + w)) > 1024u) ++w;
    return w;
}


// head-room of a first-pass bucket slab over the mean bucket, in per cent: 50 at full speed; the lean work size
// (adlhip_radix_sort_scratch_bytes_for, level 2) takes 12 -- 64 Mi u32 keys then need 306 MB of work instead of 451, and keys whose
// density varies by more than ~10 % over the key range are sorted by the safety net inside the sort
constexpr int kFullHeadroomPct = 50, kLeanHeadroomPct = 12;

// Workgroups of the kernels that host the safety net (512 threads, one tile of the one-sweep pass's size in LDS: two per CU).
// All of them must be resident at once -- the net's phases are separated by grid-wide barriers -- and the first 256 serve the
// 256 buckets in the kernel's ordinary role.
constexpr uint32_t kNetWgsMax = 512;
constexpr size_t kNetTableBytes = (size_t)256 * kNetWgsMax * 4 + 1024;   // [256][workgroups] digit table + 256 totals

// ---- the work buffer of a large sort -------------------------------------------------------------------------------------------------
// One struct for both layouts.  Fields a form does not have stay zero.
struct LargeLayout {
    // both forms
    size_t off_mode, off_cnt, off_off, off_hard, off_coop, off_slab_a, off_slab_b, total;
    uint32_t stride_a, stride_b, tier_b, seg_shift, slots;
    bool slab_b_in_tmp;   // the second slab fits the caller's n-element scratch array (u32 keys from ~40 Mi keys: 16-bit elements,
                          // 1.5 x the mean per segment = 0.75 n * 4 bytes); the safety net, which needs that array as its partner,
                          // only ever runs when the slabs' contents are void
    // cursor form
    uint32_t tiles_per_bucket;
    // stable and hybrid forms
    size_t off_place, off_tickets, off_status_a, off_status_b;
    uint32_t pieces, slice, rows_a, rows_b, ticket_words;
    size_t status_bytes_a, status_bytes_b;
};

// what both layouts start with: the mode words, the segment counts and offsets, the list of segments the binning finish hands to the
// LSD finish, and the safety net's table.  Returns where that table ends.
inline size_t large_layout_head(LargeLayout& L)
{
    L.off_mode = 0;
    L.off_cnt = L.off_mode + 256;
    L.off_off = L.off_cnt + 65536 * 4;
    L.off_hard = align_up(L.off_off + 65537 * 4, 256);                       // segments the binning finish hands to the LSD finish
    L.off_coop = L.off_hard + 65536 * 4;                                     // safety net: table [256][256] + 256 totals
    return L.off_coop + kNetTableBytes;
}

// the cursor form (whole keys: 8-byte elements are u64 keys)
inline LargeLayout msd2_layout(size_t n, size_t elem_bytes, int headroom_pct)
{
    LargeLayout L{};
    const uint32_t tile = elem_bytes == 4 ? 16384u : 8192u;   // TileCfg<E, 8, 512, 32 | 16>
    // mean bucket + 50 % + 4096: the head-room of the segment slabs below (1536 for a mean of 1024), so that keys whose density
    // varies by up to ~45 % over the key range stay on this path (with + 3 % any mild skew went to the safety net)
    L.stride_a = (uint32_t)align_up(n / 256 + (n / 256) * (size_t)headroom_pct / 100 + 4096, 64);
    L.seg_shift = msd2_seg_shift(n, elem_bytes == 8);   // the cursor form sorts whole keys: 8-byte elements = u64 keys
    L.slots = 256u << L.seg_shift;
    const bool fine = elem_bytes == 4 && L.seg_shift == 8;   // whole u32 keys, 16-bit second slab
    L.stride_b = msd2_stride_b(n, L.slots, fine);
    L.tier_b = msd2_tier_b(n, L.slots, fine);
    L.tiles_per_bucket = (L.stride_a + tile - 1) / tile;
    L.off_slab_a = align_up(large_layout_head(L), 256);
    L.off_slab_b = align_up(L.off_slab_a + (size_t)256 * L.stride_a * elem_bytes, 256);
    // u32 keys: 16-bit second slab (when the finish has 16 bits to sort: w = 8)
    const size_t slab_b_bytes = (size_t)L.slots * L.stride_b * (elem_bytes == 4 && L.seg_shift == 8 ? 2 : elem_bytes);
    L.slab_b_in_tmp = elem_bytes == 4 && L.seg_shift == 8 && n >= kSlabInTmpMin && slab_b_bytes <= n * elem_bytes;
    L.total = L.off_slab_b + (L.slab_b_in_tmp ? 0 : slab_b_bytes);
    return L;
}

// the stable and hybrid forms
// slab16: whole u32 keys -- the second slab holds their low 16 bits and, from 16 Mi keys, sits in the caller's n-element scratch
// array (see LargeLayout::slab_b_in_tmp)
// lean: the sub-slabs of the first pass and the segment slabs keep statistical head-room only (mean + 8 sd / + 7.5 sd instead of
// + 50 %): 64 Mi pairs 1.25 GB of work instead of 1.7.  Evenly spread keys run at the same speed; keys whose density varies by more
// than a few per cent between neighbouring parts of their range take the safety net.
inline LargeLayout msd2s_layout(size_t n, size_t elem_bytes, bool slab16, bool lean)
{
    LargeLayout L{};
    const uint32_t kMsd2sTile = msd2s_tile(elem_bytes);
    // pieces = chains of pass A = sub-slabs per bucket.  16 = twice the number of XCDs: workgroup i runs on XCD i % 8 and takes
    // chain i % 16, so a chain's tiles stay on ONE XCD -- its status rows and the abutting runs of consecutive tiles meet in
    // that XCD's L2.  Chain counts that break this measured slower although they make pass B's tiles fuller (64 Mi pairs,
    // pass A / pass B: 16 chains 0.252 / 0.309 ms, 12 chains 0.282 / 0.325, 18 chains 0.303 / 0.324).  The code below keeps
    // the choice open (any count up to 24 works).
    L.pieces = 16;
    const size_t slice = align_up((n + L.pieces - 1) / L.pieces, kMsd2sTile);
    const size_t mean = slice / 256;
    size_t sd = 1;
    while (sd * sd < mean) ++sd;
    const size_t stride = align_up(mean + (lean ? 0 : mean / 2) + 8 * sd + 64, 64);   // + 50 %: as much skew as the segment slabs take
    L.slice = (uint32_t)slice;
    L.stride_a = (uint32_t)stride;
    L.rows_a = L.slice / kMsd2sTile;
    // the most tiles a bucket can have: pass B's tiles run across the sub-slabs, and a sub-slab holds at most its stride
    L.rows_b = (uint32_t)(((size_t)L.pieces * L.stride_a + kMsd2sTile - 1) / kMsd2sTile);
    // (whole u32 keys keep 65536 segments: their second slab holds 16-bit keys only while the finish has 16 bits to sort)
    L.seg_shift = slab16 ? 8u : msd2_seg_shift(n, false);
    L.slots = 256u << L.seg_shift;
    L.stride_b = msd2_stride_b(n, L.slots, slab16, lean);
    L.tier_b = msd2_tier_b(n, L.slots, slab16);
    L.ticket_words = (32 + 256) * kLargeTicketStride;
    L.status_bytes_a = (size_t)L.pieces * L.rows_a * 1024;
    L.status_bytes_b = (size_t)256 * L.rows_b * 1024;
    L.off_place = 128;
    L.off_tickets = align_up(large_layout_head(L), 256);
    // the regions are sized by bounds that do not depend on `pieces` and grow with n, so that the scratch for n suffices
    // for every smaller n (adlhip_radix_sort_scratch_bytes): sub-slabs of a bucket together <= n/256 + 16 * (head-room),
    // rows of pass A <= n/tile + 16, rows of a bucket in pass B <= its sub-slabs / tile + 16
    size_t sdb = 1;
    while (sdb * sdb * 4096 < n) ++sdb;   // >= sd of every choice (a sub-slab's mean is at most n / 4096 + 32)
    const size_t bucket_bound = n / 256 + (lean ? 0 : n / 512) + 24 * (32 + 16 + 8 * (sdb + 1) + 128);
    const size_t rows_a_bound = n / kMsd2sTile + 24;
    const size_t rows_b_bound = bucket_bound / kMsd2sTile + 25;
    L.off_status_a = align_up(L.off_tickets + (size_t)L.ticket_words * 4, 256);
    L.off_status_b = L.off_status_a + rows_a_bound * 1024;
    L.off_slab_a = align_up(L.off_status_b + 256 * rows_b_bound * 1024, 256);
    L.off_slab_b = align_up(L.off_slab_a + 256 * bucket_bound * elem_bytes, 256);
    const size_t slab_b_bytes = (size_t)L.slots * L.stride_b * (slab16 ? 2 : elem_bytes);
    L.slab_b_in_tmp = slab16 && n >= kSlabInTmpMin && slab_b_bytes <= n * elem_bytes;
    L.total = L.off_slab_b + (L.slab_b_in_tmp ? 0 : slab_b_bytes);
    if ((size_t)L.pieces * L.rows_a > rows_a_bound || L.rows_b > rows_b_bound || (size_t)L.pieces * L.stride_a > bucket_bound)
        L.total = 0;   // cannot happen; msd2s_sort refuses
    return L;
}

// Which sorts take the large sort, and in which form.  keys: the element is the key (u32 / u64 keys), else {key, value} pairs.
//   whole u32 keys from 96 Mi keys               -> hybrid: stable first pass + cursor-placed second pass (msd2s_sort, hybrid)
//   whole u64 keys from 48 Mi keys               -> stable passes (msd2s_sort) + binning finish
//   whole keys below                            -> cursor passes (msd2_sort: smaller fixed cost)
//   pairs; partial sortBits (>= 16)             -> stable passes (msd2s_sort)
// "sort.msd2" = 3 / 4 / 5 force the stable / cursor / hybrid form where it applies (tests, A/B measurements).
enum LargeForm { kLargeNone = 0, kLargeCursor, kLargeStable, kLargeHybrid };
inline LargeForm large_sort_form(const adlhip_device* d, size_t elem_bytes, bool keys, size_t n, int sort_bits, int max_bits)
{
    if (!(d->sort_algo < 0 && d->msd2_path && d->digit_bits == 8 && d->tile_variant < 0)) return kLargeNone;
    if (d->resident_wgs < 256) return kLargeNone;   // the safety net's grid barrier spans 256 workgroups
    if (sort_bits < 16) return kLargeNone;          // two 8-bit digits must fit inside the sorted bits
    const bool forced = d->msd2_path >= 2;
    const bool whole = sort_bits == max_bits;
    // "sort.rank" = 0 (no reliance on the lane order of colliding DS atomics): pairs keep the stable form -- its passes and its
    // wave-per-segment finish have ballot-ranked variants (tiles up to 2560 pairs: n <= 96 Mi) --, keys take the per-digit passes
    if (d->rank_mode != 1 && (keys || n > (size_t(96) << 20) || msd2_tier_b(n, 256u << msd2_seg_shift(n, false)) > 2560u)) return kLargeNone;
    if (!keys) return n > (forced ? kMsd2Min : kMsd2sAutoMin) && stable_eligible(n) ? kLargeStable : kLargeNone;
    // u64 keys have no mid-size sort (it serves 32-bit keys), and with the narrow second digit and the binning finish the large sort
    // beats their per-digit passes from the one-workgroup sort's limit up: 100 K keys 78 -> 32 us, 1 Mi 117 -> 47, 2 Mi 172 -> 52
    // (profiles/r3_small_sizes_large_sort_vs_auto.txt)
    if (n <= (forced || elem_bytes == 8 ? kMsd2Min : kMsd2AutoMin)) return kLargeNone;
    if (!whole || d->msd2_path == 3) return stable_eligible(n) ? kLargeStable : kLargeNone;
    if (d->msd2_path == 4) return n <= cursor_max(elem_bytes) ? kLargeCursor : kLargeNone;
    if (d->msd2_path == 5) return stable_eligible(n) ? kLargeHybrid : kLargeNone;
    // profiles/r3_forms_by_size.txt -- u32 keys: cursor | hybrid 64 Mi 0.424 | 0.423 ms, 128 Mi 0.782 | 0.751, 256 Mi 1.700 | 1.620
    // (16 Mi: 0.140 | 0.159); u64 keys: cursor | stable 16 Mi 0.294 | 0.312, 64 Mi 0.846 | 0.803, 256 Mi 3.18 | 2.99 (hybrid 2.96)
    // round 4 (profiles/r4_forms_by_size.txt, persistent cursor passes): u32 keys cursor | hybrid 64 Mi 0.355 | 0.420 ms, 96 Mi 0.559 | 0.585,
    // 128 Mi 0.688 | 0.743, 256 Mi 1.496 | 1.436 -- the cursor-placed first pass loses ground with n (4.3 TB/s at 64 Mi, 3.4 at 256 Mi)
    const size_t hybrid_min = d->persist ? (size_t(192) << 20) : (size_t(96) << 20);
    if (elem_bytes == 4 && n >= hybrid_min && stable_eligible(n)) return kLargeHybrid;
    if (elem_bytes == 8 && n >= (size_t(48) << 20) && stable_eligible(n)) return kLargeStable;
    return n <= cursor_max(elem_bytes) ? kLargeCursor : kLargeNone;
}

// whole u64 keys: the binning finish pays from a mean segment of ~384 keys (16 Mi keys: 0.144 vs 0.148 ms, 4 Mi: 0.116 vs 0.098,
// 64 Mi: 0.263 vs 0.406, profiles/r3_bin_finish.txt)
inline bool use_bin_finish(const adlhip_device* d, size_t elem_bytes, bool key64, size_t n, bool whole_keys)
{
    if (!whole_keys || !d->bin_finish) return false;
    if (d->bin_finish == 2) return elem_bytes == 4 || key64;   // forced (tests, A/B): any size, u32 keys too
    return elem_bytes == 8 && key64 && n >= (size_t(24) << 20);
}

// ---- one plan ------------------------------------------------------------------------------------------------------------------------
// A form at one of the two head-rooms.  lean = level 2 of adlhip_radix_sort_scratch_bytes_for: kLeanHeadroomPct in the cursor form's
// first slabs, statistical head-room only in the stable form's slabs.
struct LargeCandidate {
    LargeForm form;
    bool lean;
};
inline LargeLayout large_layout(const LargeCandidate& c, size_t n, size_t elem_bytes, bool whole)
{
    if (c.form == kLargeCursor) return msd2_layout(n, elem_bytes, c.lean ? kLeanHeadroomPct : kFullHeadroomPct);
    return msd2s_layout(n, elem_bytes, large_slab16(elem_bytes, whole), c.lean);
}
// What a sort falls back to when its preferred form does not fit the work buffer, in the order tried: whole keys may still fit the
// cursor form (its second slab is smaller), at full head-room or at the lean one; pairs and partial sorts the stable form with
// statistical head-room only.  {key, value} pairs in two arrays are pairs like any other.  Returns how many it wrote to `out`.
inline int large_fallbacks(size_t elem_bytes, bool keys, bool whole, size_t n, LargeCandidate out[3])
{
    int k = 0;
    if (cursor_eligible(elem_bytes, keys, whole, n)) {
        out[k++] = {kLargeCursor, false};
        out[k++] = {kLargeCursor, true};
    }
    if (stable_eligible(n)) out[k++] = {kLargeStable, true};
    return k;
}

// What one sort call runs: the form, its head-room, and the layout of its work buffer.  form == kLargeNone: not the large sort.
struct LargePlan {
    LargeForm form = kLargeNone;
    bool lean = false;                        // the candidate's: level-2 head-room
    int headroom_pct = kFullHeadroomPct;      // of the cursor form's first slabs
    bool slab16 = false;                      // the second slab holds the keys' low 16 bits (whole u32 keys, 65536 segments)
    bool bin = false;                         // the binning finish (use_bin_finish)
    LargeLayout L{};
    size_t work_bytes = 0;                    // = L.total, what the plan needs of the offered bytes
};

// The plan of a sort of n elements of elem_bytes bytes (keys: the element is the key; pairs in one array or in two are not) on
// sort_bits of max_bits key bits, with `offered` bytes of work buffer: the form large_sort_form prefers at full head-room, else the
// first of large_fallbacks that fits, else none.  The large sort takes every input it is eligible for by size, bits and scratch --
// whatever the keys are like (adlhip.hip sort_entry).
inline LargePlan large_plan(const adlhip_device* d, size_t elem_bytes, bool keys, size_t n, int sort_bits, int max_bits, size_t offered)
{
    LargePlan P;
    const LargeForm preferred = large_sort_form(d, elem_bytes, keys, n, sort_bits, max_bits);
    if (preferred == kLargeNone) return P;
    const bool whole = sort_bits == max_bits;
    LargeCandidate c[4] = {{preferred, false}};
    const int count = 1 + large_fallbacks(elem_bytes, keys, whole, n, c + 1);
    for (int i = 0; i < count; ++i) {
        if (i > 0 && c[i].form == preferred && !c[i].lean) continue;   // (the preferred form itself: already tried)
        const LargeLayout L = large_layout(c[i], n, elem_bytes, whole);
        if (L.total > offered) continue;
        P.form = c[i].form;
        P.lean = c[i].lean;
        P.headroom_pct = c[i].form == kLargeCursor && c[i].lean ? kLeanHeadroomPct : kFullHeadroomPct;
        P.slab16 = large_slab16(elem_bytes, whole) && L.seg_shift == 8;
        // (whole u64 keys: the binning finish wants segments of ~384 keys and more -- 24 Mi keys in 65536 segments, or any n with a
        // narrow second digit, which leaves segments of about a thousand keys)
        P.bin = use_bin_finish(d, elem_bytes, keys && elem_bytes == 8, L.seg_shift < 8 ? (size_t(24) << 20) : n, whole);
        P.L = L;
        P.work_bytes = L.total;
        return P;
    }
    return P;
}

// The large sort's term of the scratch query (adlhip.hip sort_work_bytes_at) for one n: every form this (kind, n, sort_bits) can
// take, whatever "sort.msd2" says now (the knob may change between the query and the sort).  Level 1: the larger of the full stable
// and the full cursor layout; level 2, lean: the first lean fallback -- whole keys keep the cursor form with little head-room, pairs
// and partial sorts the stable form.  0: no large sort for this (kind, n, sort_bits).
inline size_t large_work_bytes_at(int elem_kind, size_t n, int sort_bits, int level)
{
    const size_t eb = elem_kind == ADLHIP_ELEM_U32 ? 4 : 8;
    const int max_bits = elem_kind == ADLHIP_ELEM_U64 ? 64 : 32;
    const bool whole = sort_bits == max_bits;
    const bool keys = elem_kind == ADLHIP_ELEM_U32 || elem_kind == ADLHIP_ELEM_U64;
    if (!(n > kMsd2Min && sort_bits >= 16)) return 0;
    LargeCandidate c[3];
    const int count = large_fallbacks(eb, keys, whole, n, c);
    if (level == 2) {
        for (int i = 0; i < count; ++i)
            if (c[i].lean) return large_layout(c[i], n, eb, whole).total;
        return 0;
    }
    size_t e = 0;
    if (stable_eligible(n)) e = large_layout({kLargeStable, false}, n, eb, whole).total;
    for (int i = 0; i < count; ++i)
        if (!c[i].lean) e = std::max(e, large_layout(c[i], n, eb, whole).total);
    return e;
}

}  // namespace adlhip_internal
