// primitives.hip -- the host side of what is built on top of the sorts: typed keys and argsort, top-k, row-wise top-k, sort along rows and within segments, unique /
// run-length encode, reduce by key, typed scans, stream compaction, histograms, merges, set operations, sorted search, joins.  No reference counterpart.  It reaches the sorts through adlhip_internal.hpp alone (sort_elements,
// sort_work_bytes, soa_wide_layout) and never sees their kernels.
#include "adlhip_internal.hpp"

#include <algorithm>
#include <initializer_list>

// non-template kernels of the headers: runs_counts_kernel (unique_kernels.hpp) belongs to this unit, soa_repack_high_kernel
// (soa_wide_kernels.hpp, which typed_kernels.hpp builds on) to adlhip.hip.  A kernel is emitted whether it is launched or not, a static
// one too, so here that one becomes a template that nothing instantiates
#undef ADLHIP_KERNEL
#define ADLHIP_KERNEL template <int = 0>
#include "typed_kernels.hpp"
#undef ADLHIP_KERNEL
#define ADLHIP_KERNEL
#include "select_kernels.hpp"
#include "toprows_kernels.hpp"
#include "sortrows_kernels.hpp"
#include "segments_kernels.hpp"
#include "unique_kernels.hpp"
#include "reduce_kernels.hpp"
#include "scan_kernels.hpp"
#include "compact_kernels.hpp"
#include "histogram_kernels.hpp"
#include "merge_kernels.hpp"
#include "setop_kernels.hpp"
#include "search_kernels.hpp"
#include "join_kernels.hpp"

// instantiated in kernels_select.hip / kernels_toprows.hip / kernels_sortrows.hip / kernels_segments.hip / kernels_unique.hip / kernels_reduce.hip / kernels_scan.hip /
// kernels_compact.hip / kernels_histogram.hip / kernels_merge.hip / kernels_setop.hip / kernels_search.hip / kernels_join.hip; here they are only declared
#ifndef ADLHIP_SINGLE_TU
#define X(...) extern template __global__ __VA_ARGS__;
#include "select_kernels.inc"
#include "toprows_kernels.inc"
#include "sortrows_kernels.inc"
#include "segments_kernels.inc"
#include "unique_kernels.inc"
#include "reduce_kernels.inc"
#include "scan_kernels.inc"
#include "compact_kernels.inc"
#include "histogram_kernels.inc"
#include "merge_kernels.inc"
#include "setop_kernels.inc"
#include "search_kernels.inc"
#include "join_kernels.inc"
#undef X
#endif

using namespace adlhip_internal;

namespace {
// ---- what the entry points share ------------------------------------------------------------------------------------------------
struct TypeInfo {
    int bytes, kind;   // kind: adlhip::kKeyUnsigned / kKeySigned / kKeyFloat
};
// ADLHIP_KEY_* as (bytes, kind); `name` is the parameter that carries it
int type_info(const char* name, int type, TypeInfo* out)
{
    if (type < ADLHIP_KEY_U32 || type > ADLHIP_KEY_F64) return fail("%s must be one of ADLHIP_KEY_U32 .. ADLHIP_KEY_F64 (0..5), got %d", name, type);
    out->bytes = type < ADLHIP_KEY_U64 ? 4 : 8;
    out->kind = type % 3;
    return ADLHIP_SUCCESS;
}
int key_type_info(int key_type, int order, TypeInfo* out)
{
    if (type_info("key_type", key_type, out)) return ADLHIP_FAILURE;
    if (order != ADLHIP_ORDER_ASCENDING && order != ADLHIP_ORDER_DESCENDING)
        return fail("order must be ADLHIP_ORDER_ASCENDING (0) or ADLHIP_ORDER_DESCENDING (1), got %d", order);
    return ADLHIP_SUCCESS;
}
int reduce_value_info(int value_type, int op, TypeInfo* out)
{
    if (type_info("value_type", value_type, out)) return ADLHIP_FAILURE;
    if (op != ADLHIP_REDUCE_SUM && op != ADLHIP_REDUCE_MIN && op != ADLHIP_REDUCE_MAX)
        return fail("op must be ADLHIP_REDUCE_SUM (0), ADLHIP_REDUCE_MIN (1) or ADLHIP_REDUCE_MAX (2), got %d", op);
    return ADLHIP_SUCCESS;
}
int typed_check_n(size_t n)
{
    if (n > kMaxElems) return fail("n = %zu exceeds the supported maximum %zu", n, (size_t)kMaxElems);   // (< 2^32: indices fit a dword)
    return ADLHIP_SUCCESS;
}

int check_aligned16(const char* what, std::initializer_list<const void*> ptrs)
{
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 15u) ? fail("%s buffers must be 16-byte aligned", what) : ADLHIP_SUCCESS;
}

// do [p, p + bytes) and [q, q + qbytes) share a byte?  A null p shares none.
bool overlaps(const void* p, size_t bytes, const void* q, size_t qbytes)
{
    const char* a = static_cast<const char*>(p);
    const char* b = static_cast<const char*>(q);
    return a && a < b + qbytes && b < a + bytes;
}

// the word that takes the number of runs: required, 4-byte aligned, cleared by an empty input (the caller returns on failure or n == 0)
int count_word(adlhip_device* d, const char* what, const char* name, uint32_t* word, size_t n)
{
    if (!word) return fail("%s: %s is required", what, name);
    if (reinterpret_cast<uintptr_t>(word) & 3u) return fail("%s: %s must be 4-byte aligned", what, name);
    if (n == 0) HIPCHK(hipMemsetAsync(word, 0, 4, d->stream));
    return ADLHIP_SUCCESS;
}

// what the run-length, unique and reduce entry points refuse about their buffers, before anything is enqueued
struct Buf {
    const void* p;
    size_t bytes;
    const char* name;
    bool required = true;   // (an input always is)
};
int check_buffers(const char* what, std::initializer_list<Buf> ins, std::initializer_list<Buf> outs, const void* count, const void* work)
{
    bool null = !work;
    for (const auto& list : {ins, outs})
        for (const Buf& b : list) null |= b.required && !b.p;
    if (null) return fail("null buffer passed to %s", what);
    for (const auto& list : {ins, outs})
        for (const Buf& b : list)
            if (check_aligned16(what, {b.p, work})) return ADLHIP_FAILURE;
    for (const Buf& in : ins) {
        for (const Buf& b : outs)
            if (overlaps(b.p, b.bytes, in.p, in.bytes)) return fail("%s: %s must not overlap %s", what, b.name, in.name);
        if (overlaps(count, 4, in.p, in.bytes)) return fail("%s: the count word must not overlap %s", what, in.name);
    }
    return ADLHIP_SUCCESS;
}

// the expression ... with U_ naming uint32_t (bytes_ == 4) or uint64_t (anything else); nests for a key and a value width
#define ADLHIP_BY_WIDTH(bytes_, U_, ...) \
    ((bytes_) == 4 ? [&] { using U_ = uint32_t; return __VA_ARGS__; }() : [&] { using U_ = uint64_t; return __VA_ARGS__; }())

// The chunk split of the run and reduce stages: every workgroup owns tiles_per_wg whole tiles (the last one what is left, at least
// one); at most wgs_per_cu workgroups per CU, fewer when the grid knob says so.
struct ChunkSplit {
    uint32_t wgs, tiles, tiles_per_wg;
};
ChunkSplit chunk_split(const adlhip_device* d, size_t n, size_t tile, int wgs_per_cu, int grid_knob)
{
    const size_t tiles = (n + tile - 1) / tile;
    size_t cap = (size_t)d->prop.multiProcessorCount * wgs_per_cu;
    if (grid_knob > 0) cap = std::min(cap, (size_t)grid_knob);
    const size_t tiles_per_wg = (tiles + cap - 1) / cap;
    return ChunkSplit{(uint32_t)((tiles + tiles_per_wg - 1) / tiles_per_wg), (uint32_t)tiles, (uint32_t)tiles_per_wg};
}

// counts[r] = offsets[r + 1] - offsets[r] for the *num_out runs of n elements
int launch_runs_counts(adlhip_device* d, const uint32_t* offsets, const uint32_t* num_out, size_t n, uint32_t* counts)
{
    const uint32_t cwgs = (uint32_t)((n + adlhip::kRunsCountsPerWg - 1) / adlhip::kRunsCountsPerWg);   // (at most 2^21)
    return launch(d, "runs_counts", [&] {
        hipLaunchKernelGGL(adlhip::runs_counts_kernel, dim3(cwgs), dim3(adlhip::kSelNT), 0, d->stream, offsets, num_out, (uint32_t)n, counts);
    });
}

// ---- typed keys, order, argsort (typed_kernels.hpp) -------------------------------------------------------------------------------
// calls F_<KIND, DESC>(...) for the run-time kind and order
#define ADLHIP_TYPED_DISPATCH(kind_, desc_, CALL)                                    \
    do {                                                                             \
        switch ((kind_) * 2 + ((desc_) ? 1 : 0)) {                                   \
        case 0: CALL(adlhip::kKeyUnsigned, 0); break;                                \
        case 1: CALL(adlhip::kKeyUnsigned, 1); break;                                \
        case 2: CALL(adlhip::kKeySigned, 0); break;                                  \
        case 3: CALL(adlhip::kKeySigned, 1); break;                                  \
        case 4: CALL(adlhip::kKeyFloat, 0); break;                                   \
        default: CALL(adlhip::kKeyFloat, 1); break;                                  \
        }                                                                            \
    } while (0)

// one streaming sweep: dst[i] = enc(src[i]) or dec(src[i]).  The identity (unsigned, ascending) launches nothing when dst is src.
template <typename U>
int key_codec(adlhip_device* d, int kind, int desc, bool decode, U* dst, const U* src, size_t n)
{
    if (kind == adlhip::kKeyUnsigned && !desc) {
        if (dst != src) HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(U), hipMemcpyDeviceToDevice, d->stream));
        return ADLHIP_SUCCESS;
    }
    const size_t nvec = n / (16 / sizeof(U));
    const uint32_t wgs = (uint32_t)std::min<size_t>(std::max<size_t>((nvec + adlhip::kSoaNT - 1) / adlhip::kSoaNT, 1),
                                                    (size_t)d->prop.multiProcessorCount * 16);
    return launch(d, decode ? "key_decode" : "key_encode", [&] {
#define ADLHIP_CODEC(KIND_, DESC_)                                                                                              \
    if (decode) hipLaunchKernelGGL((adlhip::key_codec_kernel<U, KIND_, DESC_, 1>), dim3(wgs), dim3(adlhip::kSoaNT), 0, d->stream, dst, src, n); \
    else hipLaunchKernelGGL((adlhip::key_codec_kernel<U, KIND_, DESC_, 0>), dim3(wgs), dim3(adlhip::kSoaNT), 0, d->stream, dst, src, n)
        ADLHIP_TYPED_DISPATCH(kind, desc, ADLHIP_CODEC);
#undef ADLHIP_CODEC
    });
}

// The typed sibling of soa_wide_sort: {32 encoded key bits, source index} pairs through the stable pair sort, once per key dword, one
// gather at the end.  keys_out / vals_out / index_out: whichever the caller wants (null = not written); none of them may be keys_in
// or vals_in when it is gathered (8-byte keys, values) -- the callers pass partner arrays and copy back.
template <typename U, typename V>
int typed_index_sort(adlhip_device* d, int kind, int desc, const U* keys_in, U* keys_out, const V* vals_in, V* vals_out,
                     uint32_t* index_out, void* work, size_t n)
{
    const SoaWideLayout L = soa_wide_layout(d, n);
    char* w = static_cast<char*>(work);
    uint64_t* pa = reinterpret_cast<uint64_t*>(w + L.off_pairs_a);
    uint64_t* pb = reinterpret_cast<uint64_t*>(w + L.off_pairs_b);
    void* kv = w + L.off_kv;
    const uint32_t nn = (uint32_t)n;
    const uint32_t wgs = (uint32_t)stride32_wgs(d->prop, n);
    int rc = launch(d, sizeof(U) == 4 ? "typed_pack_index_k32" : "typed_pack_index_k64", [&] {
#define ADLHIP_PACK(KIND_, DESC_) \
    hipLaunchKernelGGL((adlhip::typed_pack_index_kernel<U, KIND_, DESC_>), dim3(wgs), dim3(adlhip::kSoaNT), 0, d->stream, keys_in, pa, nn)
        ADLHIP_TYPED_DISPATCH(kind, desc, ADLHIP_PACK);
#undef ADLHIP_PACK
    });
    if (rc) return rc;
    rc = sort_elements(d, ADLHIP_ELEM_KV32, pa, pb, kv, L.kv_bytes, n, 32);
    if (rc) return rc;
    const uint64_t* sorted = pa;
    if constexpr (sizeof(U) == 8) {   // second 32-bit digit; the sort is stable, so equal high dwords keep the order of their low dwords
        rc = launch(d, "typed_repack_high", [&] {
#define ADLHIP_REPACK(KIND_, DESC_) \
    hipLaunchKernelGGL((adlhip::typed_repack_high_kernel<KIND_, DESC_>), dim3(wgs), dim3(adlhip::kSoaNT), 0, d->stream, keys_in, (const uint64_t*)pa, pb, nn)
            ADLHIP_TYPED_DISPATCH(kind, desc, ADLHIP_REPACK);
#undef ADLHIP_REPACK
        });
        if (rc) return rc;
        rc = sort_elements(d, ADLHIP_ELEM_KV32, pb, pa, kv, L.kv_bytes, n, 32);
        if (rc) return rc;
        sorted = pb;
    }
    return launch(d, "typed_gather", [&] {
#define ADLHIP_GATHER(KIND_, DESC_) \
    hipLaunchKernelGGL((adlhip::typed_gather_kernel<U, V, KIND_, DESC_>), dim3(wgs), dim3(adlhip::kSoaNT), 0, d->stream, sorted, keys_in, keys_out, vals_in, vals_out, index_out, nn)
        if constexpr (sizeof(U) == 8) ADLHIP_GATHER(adlhip::kKeyUnsigned, 0);   // 8-byte keys are fetched, not decoded
        else ADLHIP_TYPED_DISPATCH(kind, desc, ADLHIP_GATHER);
#undef ADLHIP_GATHER
    });
}

// in-place pairs: gathered arrays land in the partner arrays and are copied back, as soa_wide_sort does
template <typename U, typename V>
int typed_pairs_sort(adlhip_device* d, int kind, int desc, U* keys, V* vals, U* tmp_keys, V* tmp_vals, void* work, size_t n)
{
    U* kout = sizeof(U) == 4 ? keys : tmp_keys;   // 4-byte keys are the pairs' own low dwords, decoded: keys[] is not read by the gather
    int rc = typed_index_sort<U, V>(d, kind, desc, keys, kout, vals, tmp_vals, nullptr, work, n);
    if (rc) return rc;
    if (sizeof(U) == 8) HIPCHK(hipMemcpyAsync(keys, tmp_keys, n * sizeof(U), hipMemcpyDeviceToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(vals, tmp_vals, n * sizeof(V), hipMemcpyDeviceToDevice, d->stream));
    return ADLHIP_SUCCESS;
}

// encode in place -> unsigned sort on whole keys -> decode in place.  A sort that refuses after the encode was enqueued (a work buffer
// that does not fit the one-sweep path the knobs ask for, ...) still gets its decode: the caller's keys come back as they were.
template <typename U>
int typed_keys_sort(adlhip_device* d, int elem_kind, int kind, int desc, U* keys, U* tmp, void* work, size_t work_bytes, size_t n)
{
    int rc = key_codec<U>(d, kind, desc, false, keys, keys, n);
    if (rc) return rc;
    rc = sort_elements(d, elem_kind, keys, tmp, work, work_bytes, n, 8 * (int)sizeof(U));
    if (rc) {
        const std::string kept = adlhip_last_error();
        (void)key_codec<U>(d, kind, desc, true, keys, keys, n);
        adlhip_set_last_error(kept.c_str());   // the sort's message, not the decode's
        return rc;
    }
    return key_codec<U>(d, kind, desc, true, keys, keys, n);
}

// ---- top-k (select_kernels.hpp) ----------------------------------------------------------------------
// Work buffer of adlhip_topk_typed: the larger of
//   selection   [SelState][result: k positions][X], X = the larger of
//                 two survivor lists of n {code, position} each (codes and positions in arrays of their own), and
//                 the finish, which runs when the lists are dead: [partner array of the position sort: k u32][gathered keys: k]
//                 [work of the position sort / of the k-element typed pair sort, whichever is larger]
//   fallback    [work of the n-element argsort][its sorted keys: n][its index: n u32]
// every part 256-byte aligned.
constexpr size_t kTopkSelectMaxFraction = 8;   // "topk.algo" = -1: selection while k <= n / 8 (unmeasured; tools/topk_bench.py)
struct TopkLayout {
    size_t off_result, off_x;                               // selection
    size_t off_codes[2], off_pos[2];                        //   X as survivor lists
    size_t off_ptmp, off_keys, off_fwork, fwork_bytes;      //   X as the finish's scratch
    size_t off_akeys, off_aidx, awork_bytes;                // fallback (its sort's work at offset 0)
    size_t total;
};
TopkLayout topk_layout(const adlhip_device* d, size_t key_bytes, size_t n, size_t k)
{
    TopkLayout L;
    L.off_result = sizeof(adlhip::SelState);
    L.off_x = L.off_result + align_up(k * 4, 256);
    size_t o = L.off_x;
    for (int i = 0; i < 2; ++i) {
        L.off_codes[i] = o;
        L.off_pos[i] = o + align_up(n * key_bytes, 256);
        o = L.off_pos[i] + align_up(n * 4, 256);
    }
    const size_t lists_end = o;
    L.off_ptmp = L.off_x;
    L.off_keys = L.off_ptmp + align_up(k * 4, 256);
    L.off_fwork = L.off_keys + align_up(k * key_bytes, 256);
    L.fwork_bytes = std::max(sort_work_bytes(d, ADLHIP_ELEM_U32, k, 32, 1), soa_wide_layout(d, k).total);
    const size_t select_total = std::max(lists_end, L.off_fwork + L.fwork_bytes);
    L.awork_bytes = soa_wide_layout(d, n).total;
    L.off_akeys = align_up(L.awork_bytes, 256);
    L.off_aidx = L.off_akeys + align_up(n * key_bytes, 256);
    L.total = std::max(select_total, L.off_aidx + align_up(n * 4, 256));
    return L;
}

// digit `level` of the composite (code of `key_bits` bits, position of `pos_bits` bits), most significant first, 11 bits each but
// for the last digit of either part
adlhip::SelDigit topk_digit(int level, int key_bits, int pos_bits)
{
    const int key_levels = (key_bits + adlhip::kSelDigitBits - 1) / adlhip::kSelDigitBits;
    const bool from_pos = level >= key_levels;
    const int left = from_pos ? pos_bits - adlhip::kSelDigitBits * (level - key_levels) : key_bits - adlhip::kSelDigitBits * level;
    if (left <= 0) return adlhip::SelDigit{0u, 0u, 0u};   // behind the last digit: everything counts as digit 0
    const int bits = std::min(left, adlhip::kSelDigitBits);
    return adlhip::SelDigit{from_pos ? 1u : 0u, (uint32_t)(left - bits), (1u << bits) - 1u};
}

// the composite of n positions: bits of the position part, digits in all (<= kSelMaxLevels)
struct SelectPlan {
    int pos_bits, levels;
};
SelectPlan select_plan(int key_bits, size_t n)
{
    int pos_bits = 1;
    while (pos_bits < 32 && ((size_t)1 << pos_bits) < n) ++pos_bits;
    const int digit = adlhip::kSelDigitBits;
    return SelectPlan{pos_bits, (key_bits + digit - 1) / digit + (pos_bits + digit - 1) / digit};
}

// the full argsort into the work buffer, its first k entries to the caller
template <typename U>
int topk_by_sort(adlhip_device* d, int kind, int desc, const U* keys_in, U* keys_out, uint32_t* index_out, void* work, size_t n, size_t k)
{
    const TopkLayout L = topk_layout(d, sizeof(U), n, k);
    char* w = static_cast<char*>(work);
    U* akeys = reinterpret_cast<U*>(w + L.off_akeys);
    uint32_t* aidx = reinterpret_cast<uint32_t*>(w + L.off_aidx);
    const int rc = typed_index_sort<U, uint32_t>(d, kind, desc, keys_in, keys_out ? akeys : nullptr, nullptr, nullptr, aidx, work, n);
    if (rc) return rc;
    if (keys_out) HIPCHK(hipMemcpyAsync(keys_out, akeys, k * sizeof(U), hipMemcpyDeviceToDevice, d->stream));
    if (index_out) HIPCHK(hipMemcpyAsync(index_out, aidx, k * 4, hipMemcpyDeviceToDevice, d->stream));
    return ADLHIP_SUCCESS;
}

// keys_in need not be 16-byte aligned when stage_keys is set: the two kernels that load the keys in 16-byte vectors then read a copy
// of them in the first survivor list (dead until level 2 writes it, by which time both have run); the gather reads keys_in itself
template <typename U>
int topk_by_select(adlhip_device* d, int kind, int desc, const U* keys_in, U* keys_out, uint32_t* index_out, void* work, size_t n, size_t k,
                   bool stage_keys = false)
{
    const TopkLayout L = topk_layout(d, sizeof(U), n, k);
    char* w = static_cast<char*>(work);
    adlhip::SelState* st = reinterpret_cast<adlhip::SelState*>(w);
    uint32_t* result = reinterpret_cast<uint32_t*>(w + L.off_result);
    U* codes[2] = {reinterpret_cast<U*>(w + L.off_codes[0]), reinterpret_cast<U*>(w + L.off_codes[1])};
    uint32_t* pos[2] = {reinterpret_cast<uint32_t*>(w + L.off_pos[0]), reinterpret_cast<uint32_t*>(w + L.off_pos[1])};
    const uint32_t nn = (uint32_t)n, kk = (uint32_t)k;
    const int key_bits = 8 * (int)sizeof(U);
    const SelectPlan sp = select_plan(key_bits, n);
    const int pos_bits = sp.pos_bits, levels = sp.levels;
    constexpr size_t tile = (size_t)adlhip::kSelNT * adlhip::kSelVecs * (16 / sizeof(U));
    const uint32_t wgs = (uint32_t)std::min<size_t>((n + tile - 1) / tile, (size_t)d->prop.multiProcessorCount * 8);

    HIPCHK(hipMemsetAsync(st, 0, sizeof(adlhip::SelState), d->stream));   // the starting state, whatever the buffer held
    const U* keys_vec = keys_in;
    if (stage_keys) {
        HIPCHK(hipMemcpyAsync(codes[0], keys_in, n * sizeof(U), hipMemcpyDeviceToDevice, d->stream));
        keys_vec = codes[0];
    }
    int rc = launch(d, "select_hist", [&] {
#define ADLHIP_SELH(KIND_, DESC_) \
    hipLaunchKernelGGL((adlhip::select_hist_kernel<U, KIND_, DESC_>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys_vec, nn, st, topk_digit(0, key_bits, pos_bits))
        ADLHIP_TYPED_DISPATCH(kind, desc, ADLHIP_SELH);
#undef ADLHIP_SELH
    });
    if (rc) return rc;
    rc = launch(d, "select_filter_first", [&] {
#define ADLHIP_SELF(KIND_, DESC_)                                                                                                   \
    hipLaunchKernelGGL((adlhip::select_filter_kernel<U, KIND_, DESC_, 1>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys_vec, \
                       (const uint32_t*)nullptr, codes[1], pos[1], result, st, 1u, nn, kk, topk_digit(0, key_bits, pos_bits),       \
                       topk_digit(1, key_bits, pos_bits))
        ADLHIP_TYPED_DISPATCH(kind, desc, ADLHIP_SELF);
#undef ADLHIP_SELF
    });
    if (rc) return rc;
    for (int lv = 2; lv <= levels; ++lv) {   // the worst case; a level behind the one that completed the selection leaves at once
        rc = launch(d, "select_filter", [&] {
            hipLaunchKernelGGL((adlhip::select_filter_kernel<U, 0, 0, 0>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream,
                               (const U*)codes[(lv - 1) & 1], (const uint32_t*)pos[(lv - 1) & 1], codes[lv & 1], pos[lv & 1], result, st,
                               (uint32_t)lv, nn, kk, topk_digit(lv - 1, key_bits, pos_bits), topk_digit(lv, key_bits, pos_bits));
        });
        if (rc) return rc;
    }

    // finish: the k positions ascending, their keys, then the stable typed pair sort of (key, position) -- stability and ascending
    // positions give the tie order of the argsort
    uint32_t* ptmp = reinterpret_cast<uint32_t*>(w + L.off_ptmp);
    U* gkeys = reinterpret_cast<U*>(w + L.off_keys);
    void* fwork = w + L.off_fwork;
    rc = sort_elements(d, ADLHIP_ELEM_U32, result, ptmp, fwork, L.fwork_bytes, k, 32);
    if (rc) return rc;
    const uint32_t gwgs = (uint32_t)stride32_wgs(d->prop, k);
    rc = launch(d, "select_gather", [&] {
        hipLaunchKernelGGL((adlhip::select_gather_kernel<U>), dim3(gwgs), dim3(adlhip::kSelNT), 0, d->stream, keys_in, (const uint32_t*)result,
                           gkeys, kk);
    });
    if (rc) return rc;
    return typed_index_sort<U, uint32_t>(d, kind, desc, gkeys, keys_out, index_out ? result : nullptr, index_out, nullptr, fwork, k);
}

// ---- row-wise top-k (toprows_kernels.hpp) ---------------------------------------------------------------
// "topk.rows_algo" = -1: the row kernel while k <= kRowMaxK and cols <= kTopkRowsMaxCols.  One workgroup streaming a very long row
// loses to the per-row loop, which puts the whole device on each row; where has NOT been measured (tools/topk_rows_bench.py measures
// it): 256 Ki is a placeholder, as kTopkSelectMaxFraction is.
constexpr size_t kTopkRowsMaxCols = size_t(256) << 10;
constexpr int kTopkRowsWgsPerCu = 4;   // default grid of the row kernel per CU (its LDS admits 3 workgroups of 4-byte keys, 2 of 8-byte keys)

// the per-row loop: `rows` 1-D top-k calls on the shared work buffer, in stream order
template <typename U>
int topk_rows_loop(adlhip_device* d, int kind, int desc, const U* keys_in, size_t rows, size_t cols, size_t row_stride, size_t k,
                   U* keys_out, uint32_t* index_out, void* work)
{
    const bool select = d->topk_algo < 0 ? k <= cols / kTopkSelectMaxFraction : d->topk_algo == 1;
    for (size_t r = 0; r < rows; ++r) {
        const U* row = keys_in + r * row_stride;
        U* ko = keys_out ? keys_out + r * k : nullptr;
        uint32_t* io = index_out ? index_out + r * k : nullptr;
        // (the selection loads its keys in 16-byte vectors; a row that starts elsewhere is staged.  The argsort reads key by key.)
        const int rc = select ? topk_by_select<U>(d, kind, desc, row, ko, io, work, cols, k, (reinterpret_cast<uintptr_t>(row) & 15u) != 0)
                              : topk_by_sort<U>(d, kind, desc, row, ko, io, work, cols, k);
        if (rc) return rc;
    }
    return ADLHIP_SUCCESS;
}

template <typename U>
int topk_rows_kernel_path(adlhip_device* d, int kind, int desc, const U* keys_in, size_t rows, size_t cols, size_t row_stride, size_t k,
                          U* keys_out, uint32_t* index_out)
{
    adlhip::RowPlan plan;
    const int key_bits = 8 * (int)sizeof(U);
    const SelectPlan sp = select_plan(key_bits, cols);
    plan.levels = (uint32_t)sp.levels;
    for (int lv = 0; lv < adlhip::kSelMaxLevels; ++lv) plan.d[lv] = topk_digit(lv, key_bits, sp.pos_bits);
    const size_t cap = d->topk_rows_grid > 0 ? (size_t)d->topk_rows_grid : (size_t)d->prop.multiProcessorCount * kTopkRowsWgsPerCu;
    const uint32_t wgs = (uint32_t)std::min(rows, cap);
    return launch(d, sizeof(U) == 4 ? "topk_rows_k32" : "topk_rows_k64", [&] {
#define ADLHIP_ROWS(KIND_, DESC_)                                                                                                   \
    hipLaunchKernelGGL((adlhip::topk_rows_kernel<U, KIND_, DESC_>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys_in, rows,  \
                       (uint32_t)cols, row_stride, (uint32_t)k, keys_out, index_out, plan)
        ADLHIP_TYPED_DISPATCH(kind, desc, ADLHIP_ROWS);
#undef ADLHIP_ROWS
    });
}

// ---- sort along rows (sortrows_kernels.hpp) ---------------------------------------------------------------------
// "sort.rows_algo" = -1: the row kernel while cols <= kRowCap, the flat path above.  Where the row kernel starts to lose to the flat
// path has NOT been measured (tools/sort_rows_bench.py measures it); kRowCap is what the kernel can hold.
constexpr int kSortRowsWgsPerCu = 4;   // default grid of the row kernel per CU (its LDS admits 5 workgroups of 4-byte keys, 3 of 8-byte keys)

// does the row kernel serve (rows, cols) under the knobs?  Refuses "sort.rows_algo" = 1 with rows it cannot hold
int sort_rows_by_kernel(const adlhip_device* d, size_t cols, bool* kernel)
{
    if (d->sort_rows_algo == 1 && cols > (size_t)adlhip::kRowCap)
        return fail("sort of rows: the row kernel (\"sort.rows_algo\" = 1) serves cols <= %d, got %zu", adlhip::kRowCap, cols);
    *kernel = d->sort_rows_algo < 0 ? cols <= (size_t)adlhip::kRowCap : d->sort_rows_algo == 1;
    return ADLHIP_SUCCESS;
}

// rows * cols as n, refused from 2^32 on (and above what the flat sorts index, as they refuse it themselves)
int sort_rows_elems(size_t rows, size_t cols, size_t* n)
{
    if (__builtin_mul_overflow(rows, cols, n) || *n > kMaxElems)
        return fail("sort of rows: rows * cols = %zu * %zu exceeds the supported maximum %zu", rows, cols, (size_t)kMaxElems);
    return ADLHIP_SUCCESS;
}

// Work of the flat path, n = rows * cols: [the rows packed densely: n keys (used when row_stride != cols)][p: n positions]
// [rowkey: n row ids][the partner arrays of the (rowkey, p) sort: n u32 each][work of the argsort / of that sort, whichever is
// larger], every part 256-byte aligned.  One row is the argsort alone: its work at offset 0.
struct SortRowsLayout {
    size_t off_dense, off_pos, off_rowkey, off_tkeys, off_tvals, off_swork, swork_bytes, total;
    int row_bits;   // sort_bits of the (rowkey, p) sort: the bit length of rows - 1, a multiple of 4
};
SortRowsLayout sort_rows_layout(const adlhip_device* d, size_t key_bytes, size_t rows, size_t cols)
{
    SortRowsLayout L = {};
    const size_t n = rows * cols;
    L.swork_bytes = soa_wide_layout(d, n).total;
    if (rows > 1) {
        L.row_bits = 4;
        while (L.row_bits < 32 && ((rows - 1) >> L.row_bits) != 0) L.row_bits += 4;
        L.off_pos = align_up(n * key_bytes, 256);
        L.off_rowkey = L.off_pos + align_up(n * 4, 256);
        L.off_tkeys = L.off_rowkey + align_up(n * 4, 256);
        L.off_tvals = L.off_tkeys + align_up(n * 4, 256);
        L.off_swork = L.off_tvals + align_up(n * 4, 256);
        L.swork_bytes = std::max(L.swork_bytes, sort_work_bytes(d, ADLHIP_ELEM_SOA32, n, L.row_bits, 1));
    }
    L.total = L.off_swork + L.swork_bytes;
    return L;
}

template <typename U>
int sort_rows_kernel_path(adlhip_device* d, int kind, int desc, const U* keys_in, size_t rows, size_t cols, size_t row_stride, U* keys_out,
                          uint32_t* index_out)
{
    uint32_t shift = 1;   // P = 1 << shift: the power of two >= cols, at least 2
    while (((size_t)1 << shift) < cols) ++shift;
    const size_t per_tile = (size_t)adlhip::kRowCap >> shift, tiles = (rows + per_tile - 1) / per_tile;
    size_t cap = (size_t)d->prop.multiProcessorCount * kSortRowsWgsPerCu;
    if (d->sort_rows_grid > 0) cap = std::min(cap, (size_t)d->sort_rows_grid);
    const uint32_t wgs = (uint32_t)std::min(tiles, cap);
    const uint64_t inv_cols = (uint64_t(1) << 32) / cols + 1;   // div_by_cols
    return launch(d, sizeof(U) == 4 ? "sort_rows_k32" : "sort_rows_k64", [&] {
#define ADLHIP_SROWS(KIND_, DESC_)                                                                                                  \
    hipLaunchKernelGGL((adlhip::sort_rows_kernel<U, KIND_, DESC_>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys_in, rows,  \
                       (uint32_t)cols, row_stride, shift, inv_cols, keys_out, index_out)
        ADLHIP_TYPED_DISPATCH(kind, desc, ADLHIP_SROWS);
#undef ADLHIP_SROWS
    });
}

template <typename U>
int sort_rows_flat_path(adlhip_device* d, int kind, int desc, const U* keys_in, size_t rows, size_t cols, size_t row_stride, U* keys_out,
                        uint32_t* index_out, void* work)
{
    const SortRowsLayout L = sort_rows_layout(d, sizeof(U), rows, cols);
    const size_t n = rows * cols;
    char* w = static_cast<char*>(work);
    if (rows == 1) return typed_index_sort<U, uint32_t>(d, kind, desc, keys_in, keys_out, nullptr, nullptr, index_out, w + L.off_swork, n);
    uint32_t* pos = reinterpret_cast<uint32_t*>(w + L.off_pos);
    uint32_t* rowkey = reinterpret_cast<uint32_t*>(w + L.off_rowkey);
    const uint32_t wgs = (uint32_t)std::min<size_t>((n + adlhip::kSelNT - 1) / adlhip::kSelNT, (size_t)d->prop.multiProcessorCount * 16);
    const U* dense = keys_in;
    int rc;
    if (row_stride != cols) {
        U* packed = reinterpret_cast<U*>(w + L.off_dense);
        rc = launch(d, "rows_pack", [&] {
            hipLaunchKernelGGL((adlhip::rows_pack_kernel<U>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys_in, n, (uint32_t)cols,
                               row_stride, packed);
        });
        if (rc) return rc;
        dense = packed;
    }
    rc = typed_index_sort<U, uint32_t>(d, kind, desc, dense, nullptr, nullptr, nullptr, pos, w + L.off_swork, n);
    if (rc) return rc;
    rc = launch(d, "rows_of_positions", [&] {
        hipLaunchKernelGGL(adlhip::rows_of_positions_kernel, dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, (const uint32_t*)pos, n,
                           (uint32_t)cols, rowkey);
    });
    if (rc) return rc;
    // stable on the row id: every row's elements stay in key order, ties by ascending position
    rc = adlhip_radix_sort_soa32(d, rowkey, pos, reinterpret_cast<uint32_t*>(w + L.off_tkeys), reinterpret_cast<uint32_t*>(w + L.off_tvals),
                                 w + L.off_swork, L.swork_bytes, n, L.row_bits);
    if (rc) return rc;
    return launch(d, "rows_emit", [&] {
        hipLaunchKernelGGL((adlhip::rows_emit_kernel<U>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys_in, (const uint32_t*)pos,
                           (const uint32_t*)rowkey, n, (uint32_t)cols, row_stride, keys_out, index_out);
    });
}

// ---- unique / run-length encode (unique_kernels.hpp) ------------------------------------------------------
// Work of the run stage: [chunk head counts: one u32 per workgroup of the largest grid][offsets: n + 1 u32, used when the caller wants
// counts but passes no offsets], each rounded up to 256 bytes.
constexpr int kUniqueWgsPerCu = 4;   // grid of the run stage per CU at most ("debug.unique_grid" lowers it)
struct RunsLayout {
    size_t off_offsets, total;
};
RunsLayout runs_layout(const adlhip_device* d, size_t n)
{
    RunsLayout L;
    L.off_offsets = align_up((size_t)d->prop.multiProcessorCount * kUniqueWgsPerCu * 4, 256);
    L.total = L.off_offsets + align_up((n + 1) * 4, 256);
    return L;
}

// Work of adlhip_unique_typed: [run stage][S: the sorted keys, n][the sort's own buffers]
//   keys path   [tmp: the sort's partner array, n keys][work of the typed keys sort]
//   index path  [P: the argsort's index, n u32][work of the argsort]
struct UniqueLayout {
    size_t off_sorted, off_tmp, off_swork, swork_bytes, keys_total;   // keys path
    size_t off_perm, off_awork, awork_bytes, index_total;             // index path
};
UniqueLayout unique_layout(const adlhip_device* d, size_t key_bytes, size_t n)
{
    UniqueLayout L;
    L.off_sorted = runs_layout(d, n).total;
    const size_t behind = L.off_sorted + align_up(n * key_bytes, 256);
    L.off_tmp = behind;
    L.off_swork = L.off_tmp + align_up(n * key_bytes, 256);
    L.swork_bytes = sort_work_bytes(d, key_bytes == 4 ? ADLHIP_ELEM_U32 : ADLHIP_ELEM_U64, n, 8 * (int)key_bytes, 1);
    L.keys_total = L.off_swork + align_up(L.swork_bytes, 256);
    L.off_perm = behind;
    L.off_awork = L.off_perm + align_up(n * 4, 256);
    L.awork_bytes = soa_wide_layout(d, n).total;
    L.index_total = L.off_awork + align_up(L.awork_bytes, 256);
    return L;
}

// the run stage on n > 0 grouped keys; perm (null or the argsort's index) feeds first_index and inverse
template <typename U>
int runs_stage(adlhip_device* d, const U* keys, const uint32_t* perm, size_t n, U* unique_out, uint32_t* counts, uint32_t* offsets,
               uint32_t* first_index, uint32_t* inverse, uint32_t* num_out, void* work)
{
    const RunsLayout L = runs_layout(d, n);
    char* w = static_cast<char*>(work);
    uint32_t* chunk = reinterpret_cast<uint32_t*>(w);
    if (counts && !offsets) offsets = reinterpret_cast<uint32_t*>(w + L.off_offsets);
    const ChunkSplit cs = chunk_split(d, n, (size_t)adlhip::kSelNT * adlhip::kSelVecs * (16 / sizeof(U)), kUniqueWgsPerCu, d->unique_grid);
    const uint32_t wgs = cs.wgs, nn = (uint32_t)n, nt = cs.tiles, tpw = cs.tiles_per_wg;
    int rc = launch(d, sizeof(U) == 4 ? "runs_count_k32" : "runs_count_k64", [&] {
        hipLaunchKernelGGL((adlhip::runs_count_kernel<U>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys, nn, nt, tpw, chunk);
    });
    if (rc) return rc;
    rc = launch_scan_single(d, "runs_scan", chunk, chunk, wgs, num_out);   // in place; the total is the number of runs
    if (rc) return rc;
    rc = launch(d, sizeof(U) == 4 ? "runs_emit_k32" : "runs_emit_k64", [&] {
        if (perm)
            hipLaunchKernelGGL((adlhip::runs_emit_kernel<U, 1>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys, perm, nn, nt, tpw,
                               (const uint32_t*)chunk, unique_out, offsets, first_index, inverse);
        else
            hipLaunchKernelGGL((adlhip::runs_emit_kernel<U, 0>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys, (const uint32_t*)nullptr, nn,
                               nt, tpw, (const uint32_t*)chunk, unique_out, offsets, (uint32_t*)nullptr, (uint32_t*)nullptr);
    });
    if (rc || !counts) return rc;
    return launch_runs_counts(d, offsets, num_out, n, counts);
}

// sort (keys path: a copy of the keys, in place; index path: the argsort, which also gives P), then the run stage
template <typename U>
int unique_run(adlhip_device* d, const TypeInfo& t, int order, bool index_path, const U* keys_in, size_t n, U* unique_out,
                      uint32_t* counts, uint32_t* offsets, uint32_t* first_index, uint32_t* inverse, uint32_t* num_out, void* work)
{
    const UniqueLayout L = unique_layout(d, sizeof(U), n);
    char* w = static_cast<char*>(work);
    U* sorted = reinterpret_cast<U*>(w + L.off_sorted);
    if (index_path) {
        uint32_t* perm = reinterpret_cast<uint32_t*>(w + L.off_perm);
        const int rc = typed_index_sort<U, uint32_t>(d, t.kind, order, keys_in, sorted, nullptr, nullptr, perm, w + L.off_awork, n);
        if (rc) return rc;
        return runs_stage<U>(d, sorted, perm, n, unique_out, counts, offsets, first_index, inverse, num_out, work);
    }
    HIPCHK(hipMemcpyAsync(sorted, keys_in, n * sizeof(U), hipMemcpyDeviceToDevice, d->stream));
    const int rc = typed_keys_sort<U>(d, sizeof(U) == 4 ? ADLHIP_ELEM_U32 : ADLHIP_ELEM_U64, t.kind, order, sorted, reinterpret_cast<U*>(w + L.off_tmp),
                                      w + L.off_swork, L.swork_bytes, n);
    if (rc) return rc;
    return runs_stage<U>(d, sorted, nullptr, n, unique_out, counts, offsets, nullptr, nullptr, num_out, work);
}

// ---- reduce by key (reduce_kernels.hpp) --------------------------------------------------------------------
// Work of the reduce stage, per workgroup of the largest grid: [head counts: u32][head flags: u32][tail aggregates: 8 bytes][carries: 8
// bytes], then [offsets: n + 1 u32, used when the caller wants counts but passes no offsets], each rounded up to 256 bytes.
constexpr int kReduceWgsPerCu = 4;   // grid of the reduce stage per CU at most ("debug.reduce_grid" lowers it)
struct ReduceLayout {
    size_t off_flag, off_agg, off_carry, off_offsets, total;
};
ReduceLayout reduce_layout(const adlhip_device* d, size_t n)
{
    const size_t cap = (size_t)d->prop.multiProcessorCount * kReduceWgsPerCu;
    ReduceLayout L;
    L.off_flag = align_up(cap * 4, 256);
    L.off_agg = L.off_flag + align_up(cap * 4, 256);
    L.off_carry = L.off_agg + align_up(cap * 8, 256);
    L.off_offsets = L.off_carry + align_up(cap * 8, 256);
    L.total = L.off_offsets + align_up((n + 1) * 4, 256);
    return L;
}

// Work of adlhip_reduce_by_key_typed: [reduce stage][the sorted keys, n][the permuted values, n][work of the typed pairs sort]
struct ReduceByKeyLayout {
    size_t off_keys, off_vals, off_swork, total;
};
ReduceByKeyLayout reduce_by_key_layout(const adlhip_device* d, size_t key_bytes, size_t value_bytes, size_t n)
{
    ReduceByKeyLayout L;
    L.off_keys = reduce_layout(d, n).total;
    L.off_vals = L.off_keys + align_up(n * key_bytes, 256);
    L.off_swork = L.off_vals + align_up(n * value_bytes, 256);
    L.total = L.off_swork + align_up(soa_wide_layout(d, n).total, 256);
    return L;
}

// the reduce stage on n > 0 grouped keys and their values
template <typename K, typename W, int OP>
int reduce_stage_op(adlhip_device* d, const K* keys, const W* vals, size_t n, adlhip::RedCodec codec, K* unique_out, W* reduced_out,
                    uint32_t* counts, uint32_t* offsets, uint32_t* num_out, void* work)
{
    const ReduceLayout L = reduce_layout(d, n);
    char* w = static_cast<char*>(work);
    uint32_t* heads = reinterpret_cast<uint32_t*>(w);
    uint32_t* flag = reinterpret_cast<uint32_t*>(w + L.off_flag);
    W* agg = reinterpret_cast<W*>(w + L.off_agg);
    W* carry = reinterpret_cast<W*>(w + L.off_carry);
    if (counts && !offsets) offsets = reinterpret_cast<uint32_t*>(w + L.off_offsets);
    const ChunkSplit cs = chunk_split(d, n, (size_t)adlhip::kRedTile, kReduceWgsPerCu, d->reduce_grid);
    const uint32_t wgs = cs.wgs, nn = (uint32_t)n, nt = cs.tiles, tpw = cs.tiles_per_wg;
    static const char* const kOpName[3] = {"sum", "fsum", "max"};
    const std::string kv = "_k" + std::to_string(8 * sizeof(K)) + "v" + std::to_string(8 * sizeof(W));
    int rc = launch(d, intern(std::string("reduce_partial_") + kOpName[OP] + kv), [&] {
        hipLaunchKernelGGL((adlhip::reduce_partial_kernel<K, W, OP>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys, vals, nn, nt, tpw, codec,
                           heads, flag, agg);
    });
    if (rc) return rc;
    rc = launch(d, intern(std::string("reduce_carry_") + kOpName[OP] + "_v" + std::to_string(8 * sizeof(W))), [&] {   // the head counts in place; their total is the number of runs
        hipLaunchKernelGGL((adlhip::reduce_carry_kernel<W, OP>), dim3(1), dim3(adlhip::kSelNT), 0, d->stream, heads, (const uint32_t*)flag,
                           (const W*)agg, carry, wgs, num_out);
    });
    if (rc) return rc;
    rc = launch(d, intern(std::string("reduce_emit_") + kOpName[OP] + kv), [&] {
        hipLaunchKernelGGL((adlhip::reduce_emit_kernel<K, W, OP>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys, vals, nn, nt, tpw, codec,
                           (const uint32_t*)heads, (const W*)carry, unique_out, reduced_out, offsets);
    });
    if (rc || !counts) return rc;
    return launch_runs_counts(d, offsets, num_out, n, counts);
}

// the kernel's operator from (op, the value's kind): wrapping sum, float sum, or max on codes (min: complemented codes)
template <typename K, typename W>
int reduce_stage(adlhip_device* d, const K* keys, const W* vals, size_t n, int value_kind, int op, K* unique_out, W* reduced_out,
                 uint32_t* counts, uint32_t* offsets, uint32_t* num_out, void* work)
{
    adlhip::RedCodec codec = {(uint32_t)value_kind, op == ADLHIP_REDUCE_MIN ? 1u : 0u};
    if (op != ADLHIP_REDUCE_SUM)
        return reduce_stage_op<K, W, adlhip::kRedMax>(d, keys, vals, n, codec, unique_out, reduced_out, counts, offsets, num_out, work);
    if (value_kind == adlhip::kKeyFloat)
        return reduce_stage_op<K, W, adlhip::kRedFloatSum>(d, keys, vals, n, codec, unique_out, reduced_out, counts, offsets, num_out, work);
    return reduce_stage_op<K, W, adlhip::kRedSum>(d, keys, vals, n, codec, unique_out, reduced_out, counts, offsets, num_out, work);
}

// the stable typed pairs sort from the caller's arrays into d_work (no copy: the sort's gather writes there), then the reduce stage
template <typename K, typename W>
int reduce_by_key_run(adlhip_device* d, const TypeInfo& t, int order, const K* keys_in, const W* vals_in, size_t n, int value_kind, int op,
                      K* unique_out, W* reduced_out, uint32_t* counts, uint32_t* offsets, uint32_t* num_out, void* work)
{
    const ReduceByKeyLayout L = reduce_by_key_layout(d, sizeof(K), sizeof(W), n);
    char* w = static_cast<char*>(work);
    K* skeys = reinterpret_cast<K*>(w + L.off_keys);
    W* svals = reinterpret_cast<W*>(w + L.off_vals);
    const int rc = typed_index_sort<K, W>(d, t.kind, order, keys_in, skeys, vals_in, svals, nullptr, w + L.off_swork, n);
    if (rc) return rc;
    return reduce_stage<K, W>(d, skeys, svals, n, value_kind, op, unique_out, reduced_out, counts, offsets, num_out, work);
}

// ---- typed scans (scan_kernels.hpp) ---------------------------------------------------------------------------
// Work of the scan stage, per workgroup of the largest grid: [head counts: u32, written and not used][head flags: u32][chunk
// aggregates: 8 bytes][carries: 8 bytes], each rounded up to 256 bytes, then 256 bytes for the word reduce_carry_kernel puts its
// number of runs in.  Nothing proportional to n.
constexpr int kScanWgsPerCu = 4;   // grid of the scan stage per CU at most ("debug.scan_grid" lowers it)
struct ScanLayout {
    size_t off_flag, off_agg, off_carry, off_count, total;
};
ScanLayout scan_layout(const adlhip_device* d)
{
    const size_t cap = (size_t)d->prop.multiProcessorCount * kScanWgsPerCu;
    ScanLayout L;
    L.off_flag = align_up(cap * 4, 256);
    L.off_agg = L.off_flag + align_up(cap * 4, 256);
    L.off_carry = L.off_agg + align_up(cap * 8, 256);
    L.off_count = L.off_carry + align_up(cap * 8, 256);
    L.total = L.off_count + 256;
    return L;
}

// the scan stage on n > 0 values; K = adlhip::ScanNoKey (keys null): one segment
template <typename K, typename W, int OP>
int scan_stage_op(adlhip_device* d, const K* keys, const W* vals, W* out, size_t n, adlhip::RedCodec codec, uint32_t mode, W init, void* work)
{
    constexpr bool keyed = !std::is_same<K, adlhip::ScanNoKey>::value;
    const ScanLayout L = scan_layout(d);
    char* w = static_cast<char*>(work);
    uint32_t* heads = reinterpret_cast<uint32_t*>(w);
    uint32_t* flag = reinterpret_cast<uint32_t*>(w + L.off_flag);
    W* agg = reinterpret_cast<W*>(w + L.off_agg);
    W* carry = reinterpret_cast<W*>(w + L.off_carry);
    uint32_t* count = reinterpret_cast<uint32_t*>(w + L.off_count);
    const ChunkSplit cs = chunk_split(d, n, (size_t)adlhip::kRedTile, kScanWgsPerCu, d->scan_grid);
    const uint32_t wgs = cs.wgs, nn = (uint32_t)n, nt = cs.tiles, tpw = cs.tiles_per_wg;
    static const char* const kOpName[3] = {"sum", "fsum", "max"};
    const std::string kv = (keyed ? "_k" + std::to_string(8 * sizeof(K)) : std::string("_k0")) + "v" + std::to_string(8 * sizeof(W));
    int rc = launch(d, intern(std::string("scan_partial_") + kOpName[OP] + kv), [&] {
        if constexpr (keyed)
            hipLaunchKernelGGL((adlhip::reduce_partial_kernel<K, W, OP>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys, vals, nn, nt, tpw,
                               codec, heads, flag, agg);
        else
            hipLaunchKernelGGL((adlhip::scan_partial_kernel<W, OP>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, vals, nn, nt, tpw, codec,
                               heads, flag, agg);
    });
    if (rc) return rc;
    rc = launch(d, intern(std::string("scan_carry_") + kOpName[OP] + "_v" + std::to_string(8 * sizeof(W))), [&] {
        hipLaunchKernelGGL((adlhip::reduce_carry_kernel<W, OP>), dim3(1), dim3(adlhip::kSelNT), 0, d->stream, heads, (const uint32_t*)flag,
                           (const W*)agg, carry, wgs, count);
    });
    if (rc) return rc;
    return launch(d, intern(std::string("scan_emit_") + kOpName[OP] + kv), [&] {
        hipLaunchKernelGGL((adlhip::scan_emit_kernel<K, W, OP>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys, vals, nn, nt, tpw, codec,
                           (const uint32_t*)flag, (const W*)agg, (const W*)carry, mode, init, out);
    });
}

// the kernel's operator from (op, the value's kind), as reduce_stage; the init's bits from host memory
template <typename K, typename W>
int scan_stage(adlhip_device* d, const K* keys, const W* vals, W* out, size_t n, int value_kind, int op, int exclusive, const void* h_init,
               void* work)
{
    const adlhip::RedCodec codec = {(uint32_t)value_kind, op == ADLHIP_REDUCE_MIN ? 1u : 0u};
    const uint32_t mode = !exclusive ? adlhip::kScanInclusive : h_init ? adlhip::kScanExclusiveInit : adlhip::kScanExclusive;
    W init = (W)0;
    if (h_init) __builtin_memcpy(&init, h_init, sizeof(W));
    if (op != ADLHIP_REDUCE_SUM) return scan_stage_op<K, W, adlhip::kRedMax>(d, keys, vals, out, n, codec, mode, init, work);
    if (value_kind == adlhip::kKeyFloat) return scan_stage_op<K, W, adlhip::kRedFloatSum>(d, keys, vals, out, n, codec, mode, init, work);
    return scan_stage_op<K, W, adlhip::kRedSum>(d, keys, vals, out, n, codec, mode, init, work);
}

// what both scan entry points refuse, before anything is enqueued; keys_in is null for the plain scan.  *done: nothing is left to do
int scan_check(adlhip_device* d, const char* what, const char* sizer, int key_bytes, const void* keys_in, const TypeInfo& v, int exclusive,
               const void* h_init, const void* vals_in, const void* out, size_t n, const void* work, size_t work_bytes, bool* done)
{
    *done = false;
    if (exclusive != 0 && exclusive != 1) return fail("%s: exclusive must be 0 or 1, got %d", what, exclusive);
    if (!exclusive && h_init) return fail("%s: an inclusive scan takes no init (h_init_or_null must be NULL)", what);
    if (typed_check_n(n)) return ADLHIP_FAILURE;
    if (n == 0) {
        *done = true;
        return ADLHIP_SUCCESS;
    }
    if ((key_bytes && !keys_in) || !vals_in || !out || !work) return fail("null buffer passed to %s", what);
    if (check_aligned16(what, {keys_in, vals_in, out, work})) return ADLHIP_FAILURE;
    const size_t vbytes = n * (size_t)v.bytes;
    if (key_bytes && overlaps(out, vbytes, keys_in, n * (size_t)key_bytes)) return fail("%s: d_out must not overlap d_keys_in", what);
    if (out != vals_in && overlaps(out, vbytes, vals_in, vbytes))
        return fail("%s: d_out must be d_vals_in itself or not overlap it", what);
    const size_t need = scan_layout(d).total;
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (%s)", work_bytes, need, sizer);
    return ADLHIP_SUCCESS;
}


// ---- stream compaction (compact_kernels.hpp) ------------------------------------------------------------------
// Work of the compaction: [selected counts: one u32 per workgroup of the largest grid], rounded up to 256 bytes.  Nothing proportional
// to n.
constexpr int kCompactWgsPerCu = 4;   // grid of the compaction per CU at most ("debug.compact_grid" lowers it)
size_t compact_work_bytes(const adlhip_device* d)
{
    return align_up((size_t)d->prop.multiProcessorCount * kCompactWgsPerCu * 4, 256);
}

// the compaction of n > 0 elements.  P: uint8_t (pred = the flags) or the keys' unsigned type (pred = the keys, pred_out = where they
// go); V: the unsigned type of the array that travels along (the flagged form's items, the if form's values), vals_out null = none
template <typename P, typename V>
int compact_stage(adlhip_device* d, const P* pred, adlhip::CompactPred pr, const V* vals, size_t n, int partition, P* pred_out, V* vals_out,
                  uint32_t* index_out, uint32_t* num_out, void* work)
{
    uint32_t* chunk = static_cast<uint32_t*>(work);
    const ChunkSplit cs = chunk_split(d, n, (size_t)adlhip::kRedTile, kCompactWgsPerCu, d->compact_grid);
    const uint32_t wgs = cs.wgs, nn = (uint32_t)n, nt = cs.tiles, tpw = cs.tiles_per_wg;
    static const char* const kSource[3] = {"flags", "k32", "k64"};
    const char* source = kSource[sizeof(P) == 1 ? 0 : sizeof(P) == 4 ? 1 : 2];
    int rc = launch(d, intern(std::string("compact_count_") + source), [&] {
        hipLaunchKernelGGL((adlhip::compact_count_kernel<P>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, pred, nn, nt, tpw, pr, chunk);
    });
    if (rc) return rc;
    rc = launch_scan_single(d, "compact_scan", chunk, chunk, wgs, num_out);   // in place; the total is the number selected
    if (rc) return rc;
    const int vbits = vals_out ? 8 * (int)sizeof(V) : 0;
    return launch(d, intern(std::string("compact_emit_") + source + "_v" + std::to_string(vbits)), [&] {
        if (vals_out)
            hipLaunchKernelGGL((adlhip::compact_emit_kernel<P, V>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, pred, vals, nn, nt, tpw, pr,
                               (const uint32_t*)chunk, (const uint32_t*)num_out, (uint32_t)partition, pred_out, vals_out, index_out);
        else
            hipLaunchKernelGGL((adlhip::compact_emit_kernel<P, adlhip::CompactNone>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, pred,
                               (const adlhip::CompactNone*)nullptr, nn, nt, tpw, pr, (const uint32_t*)chunk, (const uint32_t*)num_out,
                               (uint32_t)partition, pred_out, (adlhip::CompactNone*)nullptr, index_out);
    });
}

// the width of the array that travels along: 0 (then neither pointer may be given), 4 or 8
int compact_check_width(const char* what, const char* name, int bytes, bool allow_zero, const void* in, const void* out)
{
    if (bytes != 4 && bytes != 8 && !(allow_zero && bytes == 0))
        return fail("%s: %s must be %s4 or 8, got %d", what, name, allow_zero ? "0, " : "", bytes);
    if (bytes == 0 && (in || out)) return fail("%s: %s is 0, so its input and output arrays must be NULL", what, name);
    return ADLHIP_SUCCESS;
}
int compact_check_partition(const char* what, int partition)
{
    if (partition != 0 && partition != 1) return fail("%s: partition must be 0 (select) or 1 (stable partition), got %d", what, partition);
    return ADLHIP_SUCCESS;
}

// ---- histograms (histogram_kernels.hpp) ---------------------------------------------------------------------
static_assert(ADLHIP_HISTOGRAM_TILE == adlhip::kRedTile, "the header states the tile of the count kernel");
static_assert(ADLHIP_HISTOGRAM_MAX_RANGE_BINS == adlhip::kHistRangeWords, "the range mode's counters are sized for the public limit");
static_assert(kHistogramLdsBinsMax == (int)adlhip::kHistLdsBins, "\"debug.histogram_lds_bins\" may ask for no more bins than the LDS of the launch holds");
constexpr int kHistWgsPerCu = 4;   // grid of the count kernel per CU at most, while num_bins <= 2048

// Workgroups of the count kernel at most: 4 per CU up to 2048 bins, then fewer in proportion -- every workgroup stores a row of
// num_bins words and the reduce kernel reads them all -- and never less than two per CU: with one, a SIMD holds a single wave and
// every LDS latency of the search and of the adds is exposed (measured: 4096 range bins took 5 x as long as 256).
size_t hist_grid_cap(const adlhip_device* d, size_t num_bins)
{
    const size_t cus = (size_t)d->prop.multiProcessorCount, full = cus * kHistWgsPerCu;
    return std::max(2 * cus, std::min(full, full * 2048 / num_bins));
}
// Work of the LDS path: [rows: one of num_bins u32 per workgroup of the largest grid], rounded up to 256 bytes
size_t hist_rows_bytes(const adlhip_device* d, size_t num_bins)
{
    return align_up(hist_grid_cap(d, num_bins) * num_bins * 4, 256);
}
// Work of the sorted path: [S: the sorted keys, n][tmp: the sort's partner array, n keys][work of the unsigned keys sort]
struct HistSortLayout {
    size_t off_tmp, off_swork, swork_bytes, total;
};
HistSortLayout hist_sort_layout(const adlhip_device* d, size_t key_bytes, size_t n)
{
    HistSortLayout L;
    L.off_tmp = align_up(n * key_bytes, 256);
    L.off_swork = 2 * L.off_tmp;
    L.swork_bytes = sort_work_bytes(d, key_bytes == 4 ? ADLHIP_ELEM_U32 : ADLHIP_ELEM_U64, n, 8 * (int)key_bytes, 1);
    L.total = L.off_swork + align_up(L.swork_bytes, 256);
    return L;
}
bool hist_lds_path(const adlhip_device* d, bool by_edges, size_t num_bins)
{
    return by_edges || num_bins <= (size_t)d->histogram_lds_bins;
}
size_t hist_work_bytes(const adlhip_device* d, size_t key_bytes, size_t n, size_t num_bins, bool by_edges)
{
    return hist_lds_path(d, by_edges, num_bins) ? hist_rows_bytes(d, num_bins) : hist_sort_layout(d, key_bytes, n).total;
}

// the LDS path on n > 0 keys: count into rows of the work buffer, sum the rows
template <typename U, int MODE>
int hist_lds_stage(adlhip_device* d, const U* keys, size_t n, const U* edges, int kind, size_t num_bins, int include_upper, uint32_t* counts,
                   void* work)
{
    uint32_t* rows = static_cast<uint32_t*>(work);
    size_t cap = hist_grid_cap(d, num_bins);
    if (d->histogram_grid > 0) cap = std::min(cap, (size_t)d->histogram_grid);
    const size_t tiles = (n + adlhip::kRedTile - 1) / adlhip::kRedTile, tpw = (tiles + cap - 1) / cap;
    const uint32_t wgs = (uint32_t)((tiles + tpw - 1) / tpw);   // (<= cap: the rows fit hist_rows_bytes)
    adlhip::HistArgs a;
    a.kind = (uint32_t)kind;
    a.num_bins = (uint32_t)num_bins;
    a.include_upper = (uint32_t)include_upper;
    const uint32_t words = MODE == adlhip::kHistRange ? adlhip::kHistRangeWords : adlhip::kHistLdsBins;
    a.copies = 1;
    while (a.copies < adlhip::kHistMaxCopies && (size_t)a.copies * 2 * num_bins <= words) a.copies *= 2;
    a.stride = (uint32_t)num_bins | 1u;
    a.top_step = 1;
    while ((size_t)a.top_step * 2 <= num_bins + 1) a.top_step *= 2;
    const size_t lds = adlhip::hist_edge_bytes<U, MODE>(a.num_bins) + (size_t)a.copies * a.stride * 4;   // (at most 49 172 bytes: 4097 8-byte edges + 4097 counters)
    static const char* const kName[2][2] = {{"hist_count_range_k32", "hist_count_range_k64"}, {"hist_count_bins_k32", "hist_count_bins_k64"}};
    int rc = launch(d, kName[MODE][sizeof(U) == 8], [&] {
        hipLaunchKernelGGL((adlhip::hist_count_kernel<U, MODE>), dim3(wgs), dim3(adlhip::kSelNT), lds, d->stream, keys, (uint32_t)n, (uint32_t)tiles,
                           (uint32_t)tpw, edges, a, rows);
    });
    if (rc) return rc;
    const uint32_t rwgs = (uint32_t)((num_bins + adlhip::kHistRedBins - 1) / adlhip::kHistRedBins);
    return launch(d, "hist_reduce", [&] {
        hipLaunchKernelGGL(adlhip::hist_reduce_kernel, dim3(rwgs), dim3(adlhip::kSelNT), 0, d->stream, (const uint32_t*)rows, wgs, (uint32_t)num_bins,
                           counts);
    });
}

// the sorted path on n > 0 integer keys: negative keys are large unsigned numbers, so the unsigned order groups every value below
// num_bins in front of everything that is ignored
template <typename U>
int hist_sorted_stage(adlhip_device* d, const U* keys, size_t n, size_t num_bins, uint32_t* counts, void* work)
{
    const HistSortLayout L = hist_sort_layout(d, sizeof(U), n);
    char* w = static_cast<char*>(work);
    U* sorted = reinterpret_cast<U*>(w);
    HIPCHK(hipMemcpyAsync(sorted, keys, n * sizeof(U), hipMemcpyDeviceToDevice, d->stream));
    int rc = sort_elements(d, sizeof(U) == 4 ? ADLHIP_ELEM_U32 : ADLHIP_ELEM_U64, sorted, w + L.off_tmp, w + L.off_swork, L.swork_bytes, n,
                           8 * (int)sizeof(U));
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(counts, 0, num_bins * 4, d->stream));
    const uint32_t wgs = (uint32_t)std::min<size_t>((n + adlhip::kSelNT - 1) / adlhip::kSelNT, (size_t)d->prop.multiProcessorCount * 16);
    rc = launch(d, sizeof(U) == 4 ? "hist_heads_k32" : "hist_heads_k64", [&] {
        hipLaunchKernelGGL((adlhip::hist_heads_kernel<U>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, (const U*)sorted, (uint32_t)n,
                           (uint32_t)num_bins, counts);
    });
    if (rc) return rc;
    return launch(d, sizeof(U) == 4 ? "hist_tails_k32" : "hist_tails_k64", [&] {
        hipLaunchKernelGGL((adlhip::hist_tails_kernel<U>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, (const U*)sorted, (uint32_t)n,
                           (uint32_t)num_bins, counts);
    });
}

// what both histogram entry points refuse before anything is enqueued; *done: nothing is left to do (n == 0: the counters are cleared)
int hist_check(adlhip_device* d, const char* what, const TypeInfo& t, const void* keys_in, size_t n, const void* edges_in, size_t num_bins,
               bool by_edges, uint32_t* counts, const void* work, size_t work_bytes, bool* done)
{
    *done = false;
    if (typed_check_n(n)) return ADLHIP_FAILURE;
    if (!counts) return fail("null buffer passed to %s", what);
    if (check_aligned16(what, {counts})) return ADLHIP_FAILURE;
    if (n == 0) {
        *done = true;
        HIPCHK(hipMemsetAsync(counts, 0, num_bins * 4, d->stream));
        return ADLHIP_SUCCESS;
    }
    const size_t kb = n * (size_t)t.bytes, eb = by_edges ? (num_bins + 1) * (size_t)t.bytes : 0;
    if (check_buffers(what, {{keys_in, kb, "d_keys_in"}, {edges_in, eb, "d_edges_in", by_edges}}, {{counts, num_bins * 4, "d_counts_out"}}, nullptr,
                      work))
        return ADLHIP_FAILURE;
    const size_t need = hist_work_bytes(d, (size_t)t.bytes, n, num_bins, by_edges);
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_histogram_scratch_bytes)", work_bytes, need);
    return ADLHIP_SUCCESS;
}
// key_type and num_bins of either mode
int hist_check_mode(const char* what, int key_type, size_t num_bins, bool by_edges, TypeInfo* t)
{
    if (type_info("key_type", key_type, t)) return ADLHIP_FAILURE;
    if (!by_edges && t->kind == adlhip::kKeyFloat) return fail("%s: integer key types only (U32, I32, U64, I64), got %d", what, key_type);
    const size_t most = by_edges ? (size_t)ADLHIP_HISTOGRAM_MAX_RANGE_BINS : ((size_t)1 << 31) - 1;
    if (num_bins < 1 || num_bins > most) return fail("%s: num_bins must be in [1, %zu], got %zu", what, most, num_bins);
    return ADLHIP_SUCCESS;
}

// ---- merge of sorted sequences (merge_kernels.hpp) -------------------------------------------------------------
static_assert(ADLHIP_MERGE_TILE == adlhip::kRedTile, "the header states the tile of the merge");
// grid of the tile kernel per CU at most ("debug.merge_grid" lowers it): its LDS (12 or 20 KiB) admits that many workgroups, and the
// searches and the serial merge are chains of dependent LDS reads that only other waves hide
constexpr int kMergeWgsPerCu = 8;
constexpr size_t kMergeMaxElems = kMaxElems;   // na + nb: the limit of the sorts (positions in A || B fit a dword)

// na + nb, refused when it does not fit
int merge_total(const char* what, size_t na, size_t nb, size_t* n)
{
    if (na > kMergeMaxElems || nb > kMergeMaxElems - na)
        return fail("%s: na + nb = %zu + %zu exceeds the supported maximum %zu", what, na, nb, (size_t)kMergeMaxElems);
    *n = na + nb;
    return ADLHIP_SUCCESS;
}
// Work of the merge: [split: one u32 per tile boundary], rounded up to 256 bytes
size_t merge_work_bytes(size_t n)
{
    const size_t tiles = (n + adlhip::kRedTile - 1) / adlhip::kRedTile;
    return align_up(4 * (tiles + 1), 256);
}
int merge_check_value_bytes(const char* what, int value_bytes)
{
    if (value_bytes != 0 && value_bytes != 4 && value_bytes != 8) return fail("%s: value_bytes must be 0, 4 or 8, got %d", what, value_bytes);
    return ADLHIP_SUCCESS;
}

// check_buffers for the merge: every message names the argument; an input needs `align` bytes of alignment only (its element's: a
// tile's share of it starts at an arbitrary element anyway), the inputs may overlap one another, and no output may overlap an input,
// another output or the work buffer
struct MergeBuf {
    const void* p;
    size_t bytes;
    const char* name;
    bool required;
    size_t align;
};
int merge_check_buffers(const char* what, std::initializer_list<MergeBuf> ins, std::initializer_list<MergeBuf> outs)
{
    for (const auto& list : {ins, outs})
        for (const MergeBuf& b : list) {
            if (b.required && !b.p) return fail("%s: %s is required", what, b.name);
            if (reinterpret_cast<uintptr_t>(b.p) & (b.align - 1)) return fail("%s: %s must be %zu-byte aligned", what, b.name, b.align);
        }
    for (auto o = outs.begin(); o != outs.end(); ++o) {
        for (const MergeBuf& in : ins)
            if (in.p && overlaps(o->p, o->bytes, in.p, in.bytes)) return fail("%s: %s must not overlap %s", what, o->name, in.name);
        for (auto q = o + 1; q != outs.end(); ++q)
            if (q->p && overlaps(o->p, o->bytes, q->p, q->bytes)) return fail("%s: %s must not overlap %s", what, o->name, q->name);
    }
    return ADLHIP_SUCCESS;
}

// the merge of n = na + nb > 0 elements; V: the values' unsigned type, vals_out null = none
template <typename K, typename V>
int merge_stage(adlhip_device* d, adlhip::RedCodec codec, const K* a, const V* va, size_t na, const K* b, const V* vb, size_t nb, K* keys_out,
                V* vals_out, uint32_t* index_out, void* work)
{
    uint32_t* split = static_cast<uint32_t*>(work);
    const size_t n = na + nb;
    const uint32_t tiles = (uint32_t)((n + adlhip::kRedTile - 1) / adlhip::kRedTile);   // (at most 2^21)
    const uint32_t pwgs = (tiles + 1 + (uint32_t)adlhip::kSelNT - 1) / (uint32_t)adlhip::kSelNT;
    size_t cap = (size_t)d->prop.multiProcessorCount * kMergeWgsPerCu;
    if (d->merge_grid > 0) cap = std::min(cap, (size_t)d->merge_grid);
    const uint32_t wgs = (uint32_t)std::min((size_t)tiles, cap);
    const uint32_t ua = (uint32_t)na, ub = (uint32_t)nb;
    int rc = launch(d, "merge_partition", [&] {
        hipLaunchKernelGGL((adlhip::merge_partition_kernel<K>), dim3(pwgs), dim3(adlhip::kSelNT), 0, d->stream, a, ua, b, ub, codec, tiles, split);
    });
    if (rc) return rc;
    return launch(d, "merge_tiles", [&] {
        if (vals_out)
            hipLaunchKernelGGL((adlhip::merge_tiles_kernel<K, V>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, a, va, ua, b, vb, ub, codec,
                               (const uint32_t*)split, tiles, keys_out, vals_out, index_out);
        else
            hipLaunchKernelGGL((adlhip::merge_tiles_kernel<K, adlhip::MergeNone>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, a,
                               (const adlhip::MergeNone*)nullptr, ua, b, (const adlhip::MergeNone*)nullptr, ub, codec, (const uint32_t*)split,
                               tiles, keys_out, (adlhip::MergeNone*)nullptr, index_out);
    });
}

// ---- set operations on sorted sequences (setop_kernels.hpp) ----------------------------------------------------
static_assert(ADLHIP_SETOP_TILE == adlhip::kRedTile, "the header states the tile of the set operations");
static_assert(ADLHIP_SETOP_INTERSECTION == adlhip::kSetIntersection && ADLHIP_SETOP_UNION == adlhip::kSetUnion &&
              ADLHIP_SETOP_DIFFERENCE == adlhip::kSetDifference && ADLHIP_SETOP_SYMMETRIC_DIFFERENCE == adlhip::kSetSymmetricDifference,
              "the kernels' operations are the public ones");
// grid of the count and emit kernels per CU at most ("debug.setop_grid" lowers it): the merge's, for the merge's reason
constexpr int kSetopWgsPerCu = 8;
// Work of a set operation: [kept counts: one u32 per workgroup of the largest grid], rounded up to 256 bytes, then [split: one u32 per
// tile boundary], rounded up to 256 bytes
size_t setop_chunk_bytes(const adlhip_device* d)
{
    return align_up((size_t)d->prop.multiProcessorCount * kSetopWgsPerCu * 4, 256);
}
size_t setop_work_bytes(const adlhip_device* d, size_t n)
{
    return setop_chunk_bytes(d) + merge_work_bytes(n);
}

// the set operation on n = na + nb > 0 elements; V: the values' unsigned type, vals_out null = none; cap: what every output holds
template <typename K, typename V>
int setop_stage(adlhip_device* d, adlhip::RedCodec codec, uint32_t op, const K* a, const V* va, size_t na, const K* b, const V* vb, size_t nb,
                size_t cap, K* keys_out, V* vals_out, uint32_t* index_out, uint32_t* num_out, void* work)
{
    uint32_t* chunk = static_cast<uint32_t*>(work);
    uint32_t* split = reinterpret_cast<uint32_t*>(static_cast<char*>(work) + setop_chunk_bytes(d));
    const ChunkSplit cs = chunk_split(d, na + nb, (size_t)adlhip::kRedTile, kSetopWgsPerCu, d->setop_grid);
    const uint32_t wgs = cs.wgs, tiles = cs.tiles, tpw = cs.tiles_per_wg;
    const uint32_t pwgs = (tiles + 1 + (uint32_t)adlhip::kSelNT - 1) / (uint32_t)adlhip::kSelNT;
    const uint32_t ua = (uint32_t)na, ub = (uint32_t)nb;
    int rc = launch(d, "setop_partition", [&] {
        hipLaunchKernelGGL((adlhip::merge_partition_kernel<K>), dim3(pwgs), dim3(adlhip::kSelNT), 0, d->stream, a, ua, b, ub, codec, tiles, split);
    });
    if (rc) return rc;
    rc = launch(d, sizeof(K) == 4 ? "setop_count_k32" : "setop_count_k64", [&] {
        hipLaunchKernelGGL((adlhip::setop_count_kernel<K>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, a, ua, b, ub, codec, op,
                           (const uint32_t*)split, tiles, tpw, chunk);
    });
    if (rc) return rc;
    rc = launch_scan_single(d, "setop_scan", chunk, chunk, wgs, num_out);   // in place; the total is the number kept
    if (rc) return rc;
    const int vbits = vals_out ? 8 * (int)sizeof(V) : 0;
    return launch(d, intern(std::string("setop_emit_k") + std::to_string(8 * sizeof(K)) + "_v" + std::to_string(vbits)), [&] {
        if (vals_out)
            hipLaunchKernelGGL((adlhip::setop_emit_kernel<K, V>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, a, va, ua, b, vb, ub, codec, op,
                               (const uint32_t*)split, tiles, tpw, (const uint32_t*)chunk, (uint32_t)cap, num_out, keys_out, vals_out, index_out);
        else
            hipLaunchKernelGGL((adlhip::setop_emit_kernel<K, adlhip::MergeNone>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, a,
                               (const adlhip::MergeNone*)nullptr, ua, b, (const adlhip::MergeNone*)nullptr, ub, codec, op, (const uint32_t*)split,
                               tiles, tpw, (const uint32_t*)chunk, (uint32_t)cap, num_out, keys_out, (adlhip::MergeNone*)nullptr, index_out);
    });
}

// ---- sorted search (search_kernels.hpp) ----------------------------------------------------------------------
static_assert(ADLHIP_SEARCH_TILE == adlhip::kRedTile, "the header states the tile of the search");
static_assert(ADLHIP_SEARCH_LEFT == adlhip::kSearchLeft && ADLHIP_SEARCH_RIGHT == adlhip::kSearchRight, "the header states the sides");
static_assert(kSearchLdsKeysMax == (int)adlhip::kSearchLdsKeys, "\"debug.search_lds_keys\" may ask for no more codes than the kernel's table holds");
// grid per CU at most ("debug.search_grid" lowers it): what the LDS of a full table of 4-byte codes and the registers admit; the
// search is chains of dependent reads that only other waves hide.  Never more workgroups than tiles of needles: a workgroup does not
// gather a table for less than one tile
constexpr int kSearchWgsPerCu = 8;
constexpr size_t kSearchMaxElems = 0xFFFFFFFFull;   // m and n: positions fit a dword

uint32_t search_top_step(uint32_t len)   // the largest power of two <= len; 0 for 0
{
    if (len == 0) return 0u;
    uint32_t top = 1u;
    while ((uint64_t)top * 2 <= len) top *= 2;
    return top;
}

// the bounds of n > 0 needles in m >= 0 sorted elements
template <typename U>
int search_stage(adlhip_device* d, adlhip::RedCodec codec, int side, const U* sorted, size_t m, const U* needles, size_t n, uint32_t* pos_out)
{
    const size_t cap_keys = (size_t)d->search_lds_keys;   // C, or what the knob lowered it to (>= 2)
    adlhip::SearchArgs a;
    a.m = (uint32_t)m;
    a.stride = (uint32_t)std::max<size_t>(1, (m + cap_keys - 1) / cap_keys);
    a.samples = (uint32_t)((m + a.stride - 1) / a.stride);   // <= cap_keys
    a.top_s = search_top_step(a.samples);
    a.top_g = search_top_step(a.stride);
    const ChunkSplit cs = chunk_split(d, n, (size_t)adlhip::kRedTile, kSearchWgsPerCu, d->search_grid);
    const size_t lds = align_up((size_t)a.samples * sizeof(U), 16);   // (at most 32 KiB)
    static const char* const kName[2][2] = {{"search_left_k32", "search_left_k64"}, {"search_right_k32", "search_right_k64"}};
    return launch(d, kName[side][sizeof(U) == 8], [&] {
        if (side == ADLHIP_SEARCH_LEFT)
            hipLaunchKernelGGL((adlhip::search_sorted_kernel<U, adlhip::kSearchLeft>), dim3(cs.wgs), dim3(adlhip::kSelNT), lds, d->stream, sorted, a,
                               needles, (uint32_t)n, cs.tiles, cs.tiles_per_wg, codec, pos_out);
        else
            hipLaunchKernelGGL((adlhip::search_sorted_kernel<U, adlhip::kSearchRight>), dim3(cs.wgs), dim3(adlhip::kSelNT), lds, d->stream, sorted,
                               a, needles, (uint32_t)n, cs.tiles, cs.tiles_per_wg, codec, pos_out);
    });
}

// ---- expansion of runs and join of sorted sequences (join_kernels.hpp) ---------------------------------------
static_assert(ADLHIP_JOIN_TILE == adlhip::kRedTile, "the header states the tile of the join and the expansion");
static_assert(ADLHIP_JOIN_INNER == adlhip::kJoinInner && ADLHIP_JOIN_LEFT == adlhip::kJoinLeft && ADLHIP_JOIN_SEMI == adlhip::kJoinSemi &&
              ADLHIP_JOIN_ANTI == adlhip::kJoinAnti && ADLHIP_JOIN_NONE == adlhip::kJoinNone, "the kernels' kinds are the public ones");
// grid of the bounds, sum, starts and row kernels per CU at most ("debug.join_grid" lowers it): what their LDS (16.1, 0, 8.1 and
// 12 KiB) admits of the 8 waves a SIMD holds, as the merge's
constexpr int kJoinWgsPerCu = 8;
// Work of the expansion: [row totals: one u64 per workgroup of the largest grid], rounded up to 256 bytes; [start: one u32 per
// element], rounded up to 256 bytes; [split: one u32 per boundary of the tiles of num_runs + cap items], rounded up to 256 bytes.  The
// join puts [base: one u32 per element of A], rounded up to 256 bytes, between the first two
size_t join_chunk_bytes(const adlhip_device* d)
{
    return align_up((size_t)d->prop.multiProcessorCount * kJoinWgsPerCu * 8, 256);
}
size_t expand_work_bytes(const adlhip_device* d, size_t n, size_t cap)
{
    return join_chunk_bytes(d) + align_up(4 * n, 256) + merge_work_bytes(n + cap);
}
size_t join_work_bytes(const adlhip_device* d, size_t na, size_t cap)
{
    return align_up(4 * na, 256) + expand_work_bytes(d, na, cap);
}
int expand_check_sizes(const char* what, const char* n_name, size_t n, size_t cap)
{
    if (n > kMaxElems || cap > kMaxElems - n)
        return fail("%s: %s + cap = %zu + %zu exceeds the supported maximum %zu", what, n_name, n, cap, (size_t)kMaxElems);
    return ADLHIP_SUCCESS;
}

// What follows the chunk totals of n > 0 elements: their scan, whose total goes to num_out, and -- with cap > 0 -- the starts (counts
// may be start), the partition and the rows.  cs: the chunks the totals were taken over
template <typename V>
int expand_rows_stage(adlhip_device* d, const uint32_t* counts, size_t n, size_t cap, const ChunkSplit& cs, uint64_t* chunk, uint32_t* start,
                      uint32_t* split, const uint32_t* base_in, const V* vals_in, uint32_t* run_out, uint32_t* rank_out, V* vals_out,
                      uint64_t* num_out)
{
    int rc = launch(d, "expand_scan", [&] {
        hipLaunchKernelGGL(adlhip::expand_scan_kernel, dim3(1), dim3(adlhip::kSelNT), 0, d->stream, chunk, cs.wgs, num_out);
    });
    if (rc || cap == 0) return rc;
    const uint32_t un = (uint32_t)n, ucap = (uint32_t)cap;
    rc = launch(d, "expand_starts", [&] {
        hipLaunchKernelGGL(adlhip::expand_starts_kernel, dim3(cs.wgs), dim3(adlhip::kSelNT), 0, d->stream, counts, un, ucap, cs.tiles,
                           cs.tiles_per_wg, (const uint64_t*)chunk, start);
    });
    if (rc) return rc;
    const ChunkSplit rs = chunk_split(d, n + cap, (size_t)adlhip::kRedTile, kJoinWgsPerCu, d->join_grid);
    const uint32_t pwgs = (rs.tiles + 1 + (uint32_t)adlhip::kSelNT - 1) / (uint32_t)adlhip::kSelNT;
    rc = launch(d, "expand_partition", [&] {
        hipLaunchKernelGGL(adlhip::expand_partition_kernel, dim3(pwgs), dim3(adlhip::kSelNT), 0, d->stream, (const uint32_t*)start, un,
                           (const uint64_t*)num_out, ucap, rs.tiles, split);
    });
    if (rc) return rc;
    constexpr bool has_vals = !std::is_same<V, adlhip::MergeNone>::value;
    return launch(d, has_vals ? (sizeof(V) == 4 ? "expand_rows_v32" : "expand_rows_v64") : "expand_rows_v0", [&] {
        hipLaunchKernelGGL((adlhip::expand_rows_kernel<V>), dim3(rs.wgs), dim3(adlhip::kSelNT), 0, d->stream, (const uint32_t*)start, un,
                           (const uint64_t*)num_out, ucap, (const uint32_t*)split, rs.tiles, rs.tiles_per_wg, base_in, vals_in, run_out,
                           rank_out, vals_out);
    });
}

// the expansion of n > 0 counts
template <typename V>
int expand_stage(adlhip_device* d, const uint32_t* counts, size_t n, size_t cap, const V* vals_in, uint32_t* run_out, uint32_t* rank_out,
                 V* vals_out, uint64_t* num_out, void* work)
{
    char* w = static_cast<char*>(work);
    uint64_t* chunk = reinterpret_cast<uint64_t*>(w);
    uint32_t* start = reinterpret_cast<uint32_t*>(w + join_chunk_bytes(d));
    uint32_t* split = reinterpret_cast<uint32_t*>(w + join_chunk_bytes(d) + align_up(4 * n, 256));
    const ChunkSplit cs = chunk_split(d, n, (size_t)adlhip::kRedTile, kJoinWgsPerCu, d->join_grid);
    const int rc = launch(d, "expand_sum", [&] {
        hipLaunchKernelGGL(adlhip::expand_sum_kernel, dim3(cs.wgs), dim3(adlhip::kSelNT), 0, d->stream, counts, (uint32_t)n, cs.tiles,
                           cs.tiles_per_wg, chunk);
    });
    if (rc) return rc;
    return expand_rows_stage<V>(d, counts, n, cap, cs, chunk, start, split, nullptr, vals_in, run_out, rank_out, vals_out, num_out);
}

// the join of na > 0 elements of A with nb >= 0 of B
template <typename K>
int join_stage(adlhip_device* d, adlhip::RedCodec codec, uint32_t kind, const K* a, size_t na, const K* b, size_t nb, size_t cap,
               uint32_t* index_a, uint32_t* index_b, uint64_t* num_out, void* work)
{
    char* w = static_cast<char*>(work);
    uint64_t* chunk = reinterpret_cast<uint64_t*>(w);
    uint32_t* base = reinterpret_cast<uint32_t*>(w + join_chunk_bytes(d));
    uint32_t* start = reinterpret_cast<uint32_t*>(w + join_chunk_bytes(d) + align_up(4 * na, 256));   // the counts, then their scan
    uint32_t* split = reinterpret_cast<uint32_t*>(w + join_chunk_bytes(d) + 2 * align_up(4 * na, 256));
    // the table of B: the search's, but never more than kJoinTableBytes of it
    const size_t cap_keys = std::min((size_t)d->search_lds_keys, (size_t)adlhip::kJoinTableBytes / sizeof(K));
    adlhip::SearchArgs sa;
    sa.m = (uint32_t)nb;
    sa.stride = (uint32_t)std::max<size_t>(1, (nb + cap_keys - 1) / cap_keys);
    sa.samples = (uint32_t)((nb + sa.stride - 1) / sa.stride);   // <= cap_keys
    sa.top_s = search_top_step(sa.samples);
    sa.top_g = search_top_step(sa.stride);
    const size_t lds = align_up((size_t)sa.samples * sizeof(K), 16);
    const ChunkSplit cs = chunk_split(d, na, (size_t)adlhip::kRedTile, kJoinWgsPerCu, d->join_grid);
    const int rc = launch(d, sizeof(K) == 4 ? "join_bounds_k32" : "join_bounds_k64", [&] {
        hipLaunchKernelGGL((adlhip::join_bounds_kernel<K>), dim3(cs.wgs), dim3(adlhip::kSelNT), lds, d->stream, a, (uint32_t)na, b, sa, codec,
                           kind, cs.tiles, cs.tiles_per_wg, base, start, chunk);
    });
    if (rc) return rc;
    return expand_rows_stage<adlhip::MergeNone>(d, start, na, cap, cs, chunk, start, split, base, (const adlhip::MergeNone*)nullptr, index_a,
                                                index_b, (adlhip::MergeNone*)nullptr, num_out);
}

// ---- sort within segments (segments_kernels.hpp) ---------------------------------------------------------------
static_assert(ADLHIP_SEGMENT_INDEX_LOCAL == adlhip::kSegIndexLocal && ADLHIP_SEGMENT_INDEX_GLOBAL == adlhip::kSegIndexGlobal,
              "the header states the index bases");
// default grid of the segment kernel per CU: what its LDS admits.  The tile (32 KiB for 4-byte keys, 48 KiB for 8-byte keys) and the
// starts and lengths of up to 2048 listed segments (12 KiB) make 44.1 and 60.1 KiB of the CU's 160: 3 and 2 workgroups.  Reasoned from
// the LDS alone, not measured against fewer
constexpr int kSortSegmentsWgsPerCu32 = 3, kSortSegmentsWgsPerCu64 = 2;

// does the segment kernel serve max_segment under the knobs?  Refuses "sort.segments_algo" = 1 with a bound it cannot hold
int sort_segments_by_kernel(const adlhip_device* d, size_t max_segment, bool* kernel)
{
    const bool fits = max_segment > 0 && max_segment <= (size_t)adlhip::kRowCap;
    if (d->sort_segments_algo == 1 && !fits)
        return fail("sort of segments: the segment kernel (\"sort.segments_algo\" = 1) serves 0 < max_segment <= %d, got %zu", adlhip::kRowCap,
                    max_segment);
    *kernel = d->sort_segments_algo < 0 ? fits : d->sort_segments_algo == 1;
    return ADLHIP_SUCCESS;
}

int sort_segments_sizes(size_t n, size_t num_segments)
{
    if (n > kMaxElems) return fail("sort of segments: n = %zu exceeds the supported maximum %zu", n, (size_t)kMaxElems);
    if (num_segments > kMaxElems)
        return fail("sort of segments: num_segments = %zu exceeds the supported maximum %zu", num_segments, (size_t)kMaxElems);
    return ADLHIP_SUCCESS;
}

// Work of either path, S = num_segments, every part 256-byte aligned.
//   the segment kernel  [cls: S class numbers][ids: S segment ids][the partner arrays of the (cls, ids) sort: S u32 each][counts: the 14
//                       class counts][work of that sort on 4 bits]
//   the flat path       [pos: n positions][seg: n segment ids][the partner arrays of the (seg, pos) sort: n u32 each][work of the
//                       argsort / of that sort, whichever is larger].  One segment is the argsort alone: its work at offset 0.
struct SortSegmentsLayout {
    size_t off_a, off_b, off_ta, off_tb, off_counts, off_swork, swork_bytes, total;
    int seg_bits;   // flat path: sort_bits of the (seg, pos) sort, the bit length of S - 1 rounded up to a multiple of 4
};
SortSegmentsLayout sort_segments_layout(const adlhip_device* d, bool kernel, size_t n, size_t num_segments)
{
    SortSegmentsLayout L = {};
    if (kernel) {
        const size_t part = align_up(num_segments * 4, 256);
        L.off_b = part;
        L.off_ta = 2 * part;
        L.off_tb = 3 * part;
        L.off_counts = 4 * part;
        L.off_swork = L.off_counts + 256;
        L.swork_bytes = sort_work_bytes(d, ADLHIP_ELEM_SOA32, num_segments, 4, 1);
    } else {
        L.swork_bytes = soa_wide_layout(d, n).total;
        if (num_segments > 1) {
            L.seg_bits = 4;
            while (L.seg_bits < 32 && ((num_segments - 1) >> L.seg_bits) != 0) L.seg_bits += 4;
            const size_t part = align_up(n * 4, 256);
            L.off_b = part;
            L.off_ta = 2 * part;
            L.off_tb = 3 * part;
            L.off_swork = 4 * part;
            L.swork_bytes = std::max(L.swork_bytes, sort_work_bytes(d, ADLHIP_ELEM_SOA32, n, L.seg_bits, 1));
        }
    }
    L.total = L.off_swork + L.swork_bytes;
    return L;
}

template <typename U>
int sort_segments_kernel_path(adlhip_device* d, int kind, int desc, const U* keys_in, size_t n, const uint32_t* offsets, size_t S,
                              int index_base, U* keys_out, uint32_t* index_out, uint32_t* oversized, void* work)
{
    const SortSegmentsLayout L = sort_segments_layout(d, true, n, S);
    char* w = static_cast<char*>(work);
    uint32_t* cls = reinterpret_cast<uint32_t*>(w + L.off_a);
    uint32_t* ids = reinterpret_cast<uint32_t*>(w + L.off_b);
    uint32_t* counts = reinterpret_cast<uint32_t*>(w + L.off_counts);
    const uint32_t pwgs = (uint32_t)std::min<size_t>((S + adlhip::kSelNT - 1) / adlhip::kSelNT, (size_t)d->prop.multiProcessorCount * 16);
    int rc = launch(d, "segments_classify", [&] {
        hipLaunchKernelGGL(adlhip::segments_classify_kernel, dim3(pwgs), dim3(adlhip::kSelNT), 0, d->stream, offsets, (uint32_t)S, (uint32_t)n,
                           cls, ids);
    });
    if (rc) return rc;
    // stable on the class: the ids of every class stay ascending
    rc = adlhip_radix_sort_soa32(d, cls, ids, reinterpret_cast<uint32_t*>(w + L.off_ta), reinterpret_cast<uint32_t*>(w + L.off_tb),
                                 w + L.off_swork, L.swork_bytes, S, 4);
    if (rc) return rc;
    rc = launch(d, "segments_counts", [&] {
        hipLaunchKernelGGL(adlhip::segments_counts_kernel, dim3(1), dim3(64), 0, d->stream, (const uint32_t*)cls, (uint32_t)S, counts, oversized);
    });
    if (rc) return rc;
    size_t cap = (size_t)d->prop.multiProcessorCount * (sizeof(U) == 4 ? kSortSegmentsWgsPerCu32 : kSortSegmentsWgsPerCu64);
    if (d->sort_segments_grid > 0) cap = std::min(cap, (size_t)d->sort_segments_grid);
    const uint32_t wgs = (uint32_t)std::min(S, cap);
    return launch(d, sizeof(U) == 4 ? "segments_sort_k32" : "segments_sort_k64", [&] {
#define ADLHIP_SSEG(KIND_, DESC_)                                                                                                       \
    hipLaunchKernelGGL((adlhip::segments_sort_kernel<U, KIND_, DESC_>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys_in, (uint32_t)n, \
                       offsets, (uint32_t)S, (const uint32_t*)ids, (const uint32_t*)counts, (uint32_t)index_base, keys_out, index_out)
        ADLHIP_TYPED_DISPATCH(kind, desc, ADLHIP_SSEG);
#undef ADLHIP_SSEG
    });
}

template <typename U>
int sort_segments_flat_path(adlhip_device* d, int kind, int desc, const U* keys_in, size_t n, const uint32_t* offsets, size_t S,
                            int index_base, U* keys_out, uint32_t* index_out, uint32_t* oversized, void* work)
{
    const SortSegmentsLayout L = sort_segments_layout(d, false, n, S);
    char* w = static_cast<char*>(work);
    if (oversized) HIPCHK(hipMemsetAsync(oversized, 0, 4, d->stream));   // nothing is oversized here
    if (S == 1) return typed_index_sort<U, uint32_t>(d, kind, desc, keys_in, keys_out, nullptr, nullptr, index_out, w + L.off_swork, n);
    uint32_t* pos = reinterpret_cast<uint32_t*>(w + L.off_a);
    uint32_t* seg = reinterpret_cast<uint32_t*>(w + L.off_b);
    int rc = typed_index_sort<U, uint32_t>(d, kind, desc, keys_in, nullptr, nullptr, nullptr, pos, w + L.off_swork, n);
    if (rc) return rc;
    // the segment of p: the number of offsets off[1 .. S] that are <= p, which skips runs of empty segments (p < n = off[S], so S - 1 at
    // most for offsets that keep the contract; the emit kernel clamps what others give)
    rc = search_stage<uint32_t>(d, adlhip::RedCodec{(uint32_t)adlhip::kKeyUnsigned, 0u}, ADLHIP_SEARCH_RIGHT, offsets + 1, S, pos, n, seg);
    if (rc) return rc;
    // stable on the segment: every segment's elements stay in key order, ties by ascending position
    rc = adlhip_radix_sort_soa32(d, seg, pos, reinterpret_cast<uint32_t*>(w + L.off_ta), reinterpret_cast<uint32_t*>(w + L.off_tb),
                                 w + L.off_swork, L.swork_bytes, n, L.seg_bits);
    if (rc) return rc;
    const uint32_t wgs = (uint32_t)std::min<size_t>((n + adlhip::kSelNT - 1) / adlhip::kSelNT, (size_t)d->prop.multiProcessorCount * 16);
    return launch(d, "segments_emit", [&] {
        hipLaunchKernelGGL((adlhip::segments_emit_kernel<U>), dim3(wgs), dim3(adlhip::kSelNT), 0, d->stream, keys_in, (const uint32_t*)pos,
                           (const uint32_t*)seg, (uint32_t)n, offsets, (uint32_t)S, (uint32_t)index_base, keys_out, index_out);
    });
}

}  // namespace

extern "C" {

// ---- typed keys, order, argsort ---------------------------------------------------------------------
static int key_codec_entry(adlhip_device* d, int key_type, int order, bool decode, void* dst, const void* src, size_t n)
{
    TypeInfo t;
    if (bind(d) || key_type_info(key_type, order, &t) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (n == 0) return ADLHIP_SUCCESS;
    if (!dst || !src) return fail("null buffer passed to the key codec");
    if (check_aligned16("key", {dst, src})) return ADLHIP_FAILURE;
    return ADLHIP_BY_WIDTH(t.bytes, U, key_codec<U>(d, t.kind, order, decode, (U*)dst, (const U*)src, n));
}

int adlhip_key_encode(adlhip_device* d, int key_type, int order, void* dst, const void* src, size_t n)
{
    return key_codec_entry(d, key_type, order, false, dst, src, n);
}

int adlhip_key_decode(adlhip_device* d, int key_type, int order, void* dst, const void* src, size_t n)
{
    return key_codec_entry(d, key_type, order, true, dst, src, n);
}

int adlhip_sort_typed_scratch_bytes(adlhip_device* d, int key_type, int mode, int value_bytes, size_t n, size_t* tmp_keys_bytes,
                                    size_t* tmp_vals_bytes, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    TypeInfo t;
    if (key_type_info(key_type, ADLHIP_ORDER_ASCENDING, &t) || typed_check_n(n)) return ADLHIP_FAILURE;   // (n: as the sorts refuse it)
    if (mode < 0 || mode > 2) return fail("mode must be 0 (keys only), 1 (pairs) or 2 (argsort), got %d", mode);
    if (mode == 1 && soa_check_widths(t.bytes, value_bytes)) return ADLHIP_FAILURE;
    const bool partner_keys = mode == 0 || (mode == 1 && t.bytes == 8);   // (4-byte keys of pairs come out of the sorted pairs themselves)
    if (tmp_keys_bytes) *tmp_keys_bytes = partner_keys ? align_up(n * (size_t)t.bytes, 256) : 0;
    if (tmp_vals_bytes) *tmp_vals_bytes = mode == 1 ? align_up(n * (size_t)value_bytes, 256) : 0;
    if (work_bytes) *work_bytes = mode ? soa_wide_layout(d, n).total : sort_work_bytes(d, t.bytes == 4 ? ADLHIP_ELEM_U32 : ADLHIP_ELEM_U64, n, 8 * t.bytes, 1);
    return ADLHIP_SUCCESS;
}

int adlhip_sort_keys_typed(adlhip_device* d, int key_type, int order, void* keys, void* tmp, void* work, size_t work_bytes, size_t n)
{
    TypeInfo t;
    if (bind(d) || key_type_info(key_type, order, &t) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (n == 0) return ADLHIP_SUCCESS;
    if (!keys || !tmp || !work) return fail("null buffer passed to the typed sort");
    if (check_aligned16("sort", {keys, tmp, work})) return ADLHIP_FAILURE;
    const int kind = t.bytes == 4 ? ADLHIP_ELEM_U32 : ADLHIP_ELEM_U64;
    const size_t need = sort_work_bytes(d, kind, n, 8 * t.bytes, 1);
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_sort_typed_scratch_bytes)", work_bytes, need);
    return ADLHIP_BY_WIDTH(t.bytes, U, typed_keys_sort<U>(d, kind, t.kind, order, (U*)keys, (U*)tmp, work, work_bytes, n));
}

int adlhip_sort_pairs_typed(adlhip_device* d, int key_type, int order, void* keys, void* vals, int value_bytes, void* tmp_keys,
                            void* tmp_vals, void* work, size_t work_bytes, size_t n)
{
    TypeInfo t;
    if (bind(d) || key_type_info(key_type, order, &t) || soa_check_widths(t.bytes, value_bytes) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (n == 0) return ADLHIP_SUCCESS;
    if (!keys || !vals || !tmp_vals || !work || (t.bytes == 8 && !tmp_keys)) return fail("null buffer passed to the typed sort");
    if (check_aligned16("sort", {keys, vals, tmp_keys, tmp_vals, work})) return ADLHIP_FAILURE;
    const size_t need = soa_wide_layout(d, n).total;
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_sort_typed_scratch_bytes)", work_bytes, need);
#define ADLHIP_TP(K_, V_) typed_pairs_sort<K_, V_>(d, t.kind, order, (K_*)keys, (V_*)vals, (K_*)tmp_keys, (V_*)tmp_vals, work, n)
    return ADLHIP_BY_WIDTH(t.bytes, K, value_bytes == 16 ? ADLHIP_TP(K, V16) : ADLHIP_BY_WIDTH(value_bytes, V, ADLHIP_TP(K, V)));
#undef ADLHIP_TP
}

int adlhip_argsort_typed(adlhip_device* d, int key_type, int order, const void* keys_in, void* keys_out, uint32_t* index_out, void* work,
                         size_t work_bytes, size_t n)
{
    TypeInfo t;
    if (bind(d) || key_type_info(key_type, order, &t) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (n == 0) return ADLHIP_SUCCESS;
    if (!keys_in || !index_out || !work) return fail("null buffer passed to the typed argsort");
    if (keys_out == keys_in) return fail("argsort: d_keys_out must not be d_keys_in (adlhip_sort_pairs_typed sorts in place)");
    if (check_aligned16("sort", {keys_in, keys_out, index_out, work})) return ADLHIP_FAILURE;
    const size_t need = soa_wide_layout(d, n).total;
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_sort_typed_scratch_bytes)", work_bytes, need);
    // (no values: the gather's value pointers are null, V only names an instantiation that exists anyway)
    return ADLHIP_BY_WIDTH(t.bytes, U, typed_index_sort<U, uint32_t>(d, t.kind, order, (const U*)keys_in, (U*)keys_out, nullptr, nullptr, index_out, work, n));
}

// ---- top-k --------------------------------------------------------------------------------------------
int adlhip_topk_scratch_bytes(adlhip_device* d, int key_type, size_t n, size_t k, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    TypeInfo t;
    if (key_type_info(key_type, ADLHIP_ORDER_ASCENDING, &t) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (k > n) return fail("top-k: k = %zu exceeds n = %zu", k, n);
    if (work_bytes) *work_bytes = topk_layout(d, (size_t)t.bytes, n, k).total;
    return ADLHIP_SUCCESS;
}

int adlhip_topk_typed(adlhip_device* d, int key_type, int order, const void* keys_in, size_t n, size_t k, void* keys_out,
                      uint32_t* index_out, void* work, size_t work_bytes)
{
    TypeInfo t;
    if (bind(d) || key_type_info(key_type, order, &t) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (k > n) return fail("top-k: k = %zu exceeds n = %zu", k, n);
    if (k == 0) return ADLHIP_SUCCESS;   // (n == 0 included)
    if (!keys_out && !index_out) return fail("top-k: at least one of d_keys_out and d_index_out must be given");
    if (!keys_in || !work) return fail("null buffer passed to top-k");
    if (check_aligned16("top-k", {keys_in, keys_out, index_out, work})) return ADLHIP_FAILURE;
    const size_t in_bytes = n * (size_t)t.bytes;
    if (overlaps(keys_out, k * (size_t)t.bytes, keys_in, in_bytes) || overlaps(index_out, k * 4, keys_in, in_bytes))
        return fail("top-k: the outputs must not overlap d_keys_in");
    const size_t need = topk_layout(d, (size_t)t.bytes, n, k).total;
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_topk_scratch_bytes)", work_bytes, need);
    const bool select = d->topk_algo < 0 ? k <= n / kTopkSelectMaxFraction : d->topk_algo == 1;
    return ADLHIP_BY_WIDTH(t.bytes, U, select ? topk_by_select<U>(d, t.kind, order, (const U*)keys_in, (U*)keys_out, index_out, work, n, k)
                                              : topk_by_sort<U>(d, t.kind, order, (const U*)keys_in, (U*)keys_out, index_out, work, n, k));
}

int adlhip_topk_rows_scratch_bytes(adlhip_device* d, int key_type, size_t rows, size_t cols, size_t k, size_t* work_bytes)
{
    (void)rows;   // the rows share one work buffer
    return adlhip_topk_scratch_bytes(d, key_type, cols, k, work_bytes);
}

int adlhip_topk_rows_typed(adlhip_device* d, int key_type, int order, const void* keys_in, size_t rows, size_t cols, size_t row_stride,
                           size_t k, void* keys_out, uint32_t* index_out, void* work, size_t work_bytes)
{
    TypeInfo t;
    if (bind(d) || key_type_info(key_type, order, &t) || typed_check_n(cols)) return ADLHIP_FAILURE;
    if (k > cols) return fail("top-k of rows: k = %zu exceeds cols = %zu", k, cols);
    if (row_stride < cols) return fail("top-k of rows: row_stride = %zu is below cols = %zu", row_stride, cols);
    if (k == 0 || rows == 0) return ADLHIP_SUCCESS;   // (cols == 0 included)
    if (!keys_out && !index_out) return fail("top-k of rows: at least one of d_keys_out and d_index_out must be given");
    if (!keys_in || !work) return fail("null buffer passed to top-k of rows");
    if (check_aligned16("top-k", {keys_in, keys_out, index_out, work})) return ADLHIP_FAILURE;
    size_t in_elems = 0, out_elems = 0;
    if (__builtin_mul_overflow(rows - 1, row_stride, &in_elems) || __builtin_add_overflow(in_elems, cols, &in_elems) ||
        in_elems > (SIZE_MAX >> 4) || __builtin_mul_overflow(rows, k, &out_elems) || out_elems > (SIZE_MAX >> 4))
        return fail("top-k of rows: rows = %zu with row_stride = %zu, k = %zu is beyond the address space", rows, row_stride, k);
    const size_t in_bytes = in_elems * (size_t)t.bytes;
    if (overlaps(keys_out, out_elems * (size_t)t.bytes, keys_in, in_bytes) || overlaps(index_out, out_elems * 4, keys_in, in_bytes))
        return fail("top-k of rows: the outputs must not overlap d_keys_in");
    const size_t need = topk_layout(d, (size_t)t.bytes, cols, k).total;
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_topk_rows_scratch_bytes)", work_bytes, need);
    if (d->topk_rows_algo == 1 && k > (size_t)adlhip::kRowMaxK)
        return fail("top-k of rows: the row kernel (\"topk.rows_algo\" = 1) serves k <= %d, got %zu", adlhip::kRowMaxK, k);
    const bool kernel = d->topk_rows_algo < 0 ? k <= (size_t)adlhip::kRowMaxK && cols <= kTopkRowsMaxCols : d->topk_rows_algo == 1;
    return ADLHIP_BY_WIDTH(
        t.bytes, U, kernel ? topk_rows_kernel_path<U>(d, t.kind, order, (const U*)keys_in, rows, cols, row_stride, k, (U*)keys_out, index_out)
                           : topk_rows_loop<U>(d, t.kind, order, (const U*)keys_in, rows, cols, row_stride, k, (U*)keys_out, index_out, work));
}

// ---- sort along rows ----------------------------------------------------------------------------------
int adlhip_sort_rows_scratch_bytes(adlhip_device* d, int key_type, size_t rows, size_t cols, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    TypeInfo t;
    size_t n = 0;
    bool kernel = false;
    if (key_type_info(key_type, ADLHIP_ORDER_ASCENDING, &t) || sort_rows_elems(rows, cols, &n) || sort_rows_by_kernel(d, cols, &kernel))
        return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = kernel || n == 0 ? 0 : sort_rows_layout(d, (size_t)t.bytes, rows, cols).total;
    return ADLHIP_SUCCESS;
}

int adlhip_sort_rows_typed(adlhip_device* d, int key_type, int order, const void* keys_in, size_t rows, size_t cols, size_t row_stride,
                           void* keys_out, uint32_t* index_out, void* work, size_t work_bytes)
{
    TypeInfo t;
    size_t n = 0, in_elems = 0;
    if (bind(d) || key_type_info(key_type, order, &t) || sort_rows_elems(rows, cols, &n)) return ADLHIP_FAILURE;
    if (row_stride < cols) return fail("sort of rows: row_stride = %zu is below cols = %zu", row_stride, cols);
    if (n == 0) return ADLHIP_SUCCESS;
    if (!keys_out && !index_out) return fail("sort of rows: at least one of d_keys_out and d_index_out must be given");
    if (!keys_in) return fail("sort of rows: d_keys_in is NULL");
    bool kernel = false;
    if (sort_rows_by_kernel(d, cols, &kernel)) return ADLHIP_FAILURE;
    const size_t need = kernel ? 0 : sort_rows_layout(d, (size_t)t.bytes, rows, cols).total;
    if (need && !work) return fail("sort of rows: d_work is NULL");
    const struct { const void* p; const char* name; } bases[] = {{keys_in, "d_keys_in"}, {keys_out, "d_keys_out"}, {index_out, "d_index_out"}, {work, "d_work"}};
    for (const auto& b : bases)
        if (reinterpret_cast<uintptr_t>(b.p) & 15u) return fail("sort of rows: %s must be 16-byte aligned", b.name);
    if (__builtin_mul_overflow(rows - 1, row_stride, &in_elems) || __builtin_add_overflow(in_elems, cols, &in_elems) || in_elems > (SIZE_MAX >> 4))
        return fail("sort of rows: rows = %zu with row_stride = %zu is beyond the address space", rows, row_stride);
    const size_t in_bytes = in_elems * (size_t)t.bytes;
    if (overlaps(keys_out, n * (size_t)t.bytes, keys_in, in_bytes)) return fail("sort of rows: d_keys_out must not overlap d_keys_in");
    if (overlaps(index_out, n * 4, keys_in, in_bytes)) return fail("sort of rows: d_index_out must not overlap d_keys_in");
    if (work_bytes < need) return fail("sort of rows: work_bytes = %zu is below %zu (adlhip_sort_rows_scratch_bytes)", work_bytes, need);
    return ADLHIP_BY_WIDTH(
        t.bytes, U, kernel ? sort_rows_kernel_path<U>(d, t.kind, order, (const U*)keys_in, rows, cols, row_stride, (U*)keys_out, index_out)
                           : sort_rows_flat_path<U>(d, t.kind, order, (const U*)keys_in, rows, cols, row_stride, (U*)keys_out, index_out, work));
}

// ---- sort within segments --------------------------------------------------------------------------------
int adlhip_sort_segments_scratch_bytes(adlhip_device* d, int key_type, size_t n, size_t num_segments, size_t max_segment, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    TypeInfo t;
    bool kernel = false;
    if (key_type_info(key_type, ADLHIP_ORDER_ASCENDING, &t) || sort_segments_sizes(n, num_segments) ||
        sort_segments_by_kernel(d, max_segment, &kernel))
        return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = n == 0 || num_segments == 0 ? 0 : sort_segments_layout(d, kernel, n, num_segments).total;
    return ADLHIP_SUCCESS;
}

int adlhip_sort_segments_typed(adlhip_device* d, int key_type, int order, const void* keys_in, size_t n, const uint32_t* offsets,
                               size_t num_segments, size_t max_segment, int index_base, void* keys_out, uint32_t* index_out,
                               uint32_t* num_oversized, void* work, size_t work_bytes)
{
    TypeInfo t;
    if (bind(d) || key_type_info(key_type, order, &t) || sort_segments_sizes(n, num_segments)) return ADLHIP_FAILURE;
    if (index_base != ADLHIP_SEGMENT_INDEX_LOCAL && index_base != ADLHIP_SEGMENT_INDEX_GLOBAL)
        return fail("sort of segments: index_base must be ADLHIP_SEGMENT_INDEX_LOCAL (0) or ADLHIP_SEGMENT_INDEX_GLOBAL (1), got %d", index_base);
    if (reinterpret_cast<uintptr_t>(num_oversized) & 3u) return fail("sort of segments: d_num_oversized_out must be 4-byte aligned");
    bool kernel = false;
    if (sort_segments_by_kernel(d, max_segment, &kernel)) return ADLHIP_FAILURE;
    if (n == 0 || num_segments == 0) {
        if (num_oversized) HIPCHK(hipMemsetAsync(num_oversized, 0, 4, d->stream));
        return ADLHIP_SUCCESS;
    }
    if (!keys_out && !index_out) return fail("sort of segments: at least one of d_keys_out and d_index_out must be given");
    if (!keys_in) return fail("sort of segments: d_keys_in is NULL");
    if (!offsets) return fail("sort of segments: d_offsets is NULL");
    if (!work) return fail("sort of segments: d_work is NULL");
    const struct { const void* p; const char* name; } bases[] = {
        {keys_in, "d_keys_in"}, {offsets, "d_offsets"}, {keys_out, "d_keys_out"}, {index_out, "d_index_out"}, {work, "d_work"}};
    for (const auto& b : bases)
        if (reinterpret_cast<uintptr_t>(b.p) & 15u) return fail("sort of segments: %s must be 16-byte aligned", b.name);
    const size_t kb = (size_t)t.bytes;
    const struct { const void* p; size_t bytes; const char* name; } ins[] = {{keys_in, n * kb, "d_keys_in"}, {offsets, (num_segments + 1) * 4, "d_offsets"}},
        outs[] = {{keys_out, n * kb, "d_keys_out"}, {index_out, n * 4, "d_index_out"}, {num_oversized, 4, "d_num_oversized_out"}};
    for (const auto& in : ins)
        for (const auto& o : outs)
            if (overlaps(o.p, o.bytes, in.p, in.bytes)) return fail("sort of segments: %s must not overlap %s", o.name, in.name);
    const size_t need = sort_segments_layout(d, kernel, n, num_segments).total;
    if (work_bytes < need) return fail("sort of segments: work_bytes = %zu is below %zu (adlhip_sort_segments_scratch_bytes)", work_bytes, need);
    return ADLHIP_BY_WIDTH(t.bytes, U,
                           kernel ? sort_segments_kernel_path<U>(d, t.kind, order, (const U*)keys_in, n, offsets, num_segments, index_base,
                                                                 (U*)keys_out, index_out, num_oversized, work)
                                  : sort_segments_flat_path<U>(d, t.kind, order, (const U*)keys_in, n, offsets, num_segments, index_base,
                                                               (U*)keys_out, index_out, num_oversized, work));
}

// ---- unique / run-length encode ---------------------------------------------------------------------
static int check_key_bytes(const char* what, int key_bytes)
{
    if (key_bytes != 4 && key_bytes != 8) return fail("%s: key_bytes must be 4 or 8, got %d", what, key_bytes);
    return ADLHIP_SUCCESS;
}

int adlhip_run_length_encode_scratch_bytes(adlhip_device* d, int key_bytes, size_t n, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    if (check_key_bytes("run-length encode", key_bytes) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = runs_layout(d, n).total;
    return ADLHIP_SUCCESS;
}

int adlhip_run_length_encode(adlhip_device* d, int key_bytes, const void* keys_in, size_t n, void* unique_out, uint32_t* counts_out,
                             uint32_t* offsets_out, uint32_t* num_runs_out, void* work, size_t work_bytes)
{
    if (bind(d) || check_key_bytes("run-length encode", key_bytes) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (const int rc = count_word(d, "run-length encode", "d_num_runs_out", num_runs_out, n); rc || n == 0) return rc;
    if (check_buffers("run-length encode", {{keys_in, n * (size_t)key_bytes, "d_keys_in"}},
                      {{unique_out, n * (size_t)key_bytes, "d_unique_out"}, {counts_out, n * 4, "d_counts_out", false},
                       {offsets_out, (n + 1) * 4, "d_offsets_out", false}},
                      num_runs_out, work))
        return ADLHIP_FAILURE;
    const size_t need = runs_layout(d, n).total;
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_run_length_encode_scratch_bytes)", work_bytes, need);
    return ADLHIP_BY_WIDTH(key_bytes, U, runs_stage<U>(d, (const U*)keys_in, nullptr, n, (U*)unique_out, counts_out, offsets_out, nullptr,
                                                       nullptr, num_runs_out, work));
}

int adlhip_unique_scratch_bytes(adlhip_device* d, int key_type, size_t n, int want_index, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    TypeInfo t;
    if (key_type_info(key_type, ADLHIP_ORDER_ASCENDING, &t) || typed_check_n(n)) return ADLHIP_FAILURE;
    const UniqueLayout L = unique_layout(d, (size_t)t.bytes, n);
    if (work_bytes) *work_bytes = want_index ? std::max(L.keys_total, L.index_total) : L.keys_total;
    return ADLHIP_SUCCESS;
}

int adlhip_unique_typed(adlhip_device* d, int key_type, int order, const void* keys_in, size_t n, void* unique_out, uint32_t* counts_out,
                        uint32_t* offsets_out, uint32_t* first_index_out, uint32_t* inverse_out, uint32_t* num_unique_out, void* work,
                        size_t work_bytes)
{
    TypeInfo t;
    if (bind(d) || key_type_info(key_type, order, &t) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (const int rc = count_word(d, "unique", "d_num_unique_out", num_unique_out, n); rc || n == 0) return rc;
    if (check_buffers("unique", {{keys_in, n * (size_t)t.bytes, "d_keys_in"}},
                      {{unique_out, n * (size_t)t.bytes, "d_unique_out"}, {counts_out, n * 4, "d_counts_out", false},
                       {offsets_out, (n + 1) * 4, "d_offsets_out", false}, {first_index_out, n * 4, "d_first_index_out", false},
                       {inverse_out, n * 4, "d_inverse_out", false}},
                      num_unique_out, work))
        return ADLHIP_FAILURE;
    const bool index_path = d->unique_algo == 1 || first_index_out || inverse_out;
    const UniqueLayout L = unique_layout(d, (size_t)t.bytes, n);
    const size_t need = index_path ? L.index_total : L.keys_total;
    if (work_bytes < need)
        return fail("work buffer too small: %zu < %zu (adlhip_unique_scratch_bytes, want_index = %d)", work_bytes, need, index_path ? 1 : 0);
    return ADLHIP_BY_WIDTH(t.bytes, U, unique_run<U>(d, t, order, index_path, (const U*)keys_in, n, (U*)unique_out, counts_out, offsets_out,
                                                     first_index_out, inverse_out, num_unique_out, work));
}

// ---- reduce by key ----------------------------------------------------------------------------------
int adlhip_reduce_runs_scratch_bytes(adlhip_device* d, int key_bytes, int value_type, size_t n, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    TypeInfo v;
    if (check_key_bytes("reduce runs", key_bytes) || reduce_value_info(value_type, ADLHIP_REDUCE_SUM, &v) || typed_check_n(n))
        return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = reduce_layout(d, n).total;
    return ADLHIP_SUCCESS;
}

int adlhip_reduce_runs(adlhip_device* d, int key_bytes, const void* keys_in, int value_type, int op, const void* vals_in, size_t n,
                       void* unique_out, void* reduced_out, uint32_t* counts_out, uint32_t* offsets_out, uint32_t* num_runs_out, void* work,
                       size_t work_bytes)
{
    TypeInfo v;
    if (bind(d) || check_key_bytes("reduce runs", key_bytes) || reduce_value_info(value_type, op, &v) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (const int rc = count_word(d, "reduce runs", "d_num_runs_out", num_runs_out, n); rc || n == 0) return rc;
    if (check_buffers("reduce runs", {{keys_in, n * (size_t)key_bytes, "d_keys_in"}, {vals_in, n * (size_t)v.bytes, "d_vals_in"}},
                      {{unique_out, n * (size_t)key_bytes, "d_unique_out"}, {reduced_out, n * (size_t)v.bytes, "d_reduced_out"},
                       {counts_out, n * 4, "d_counts_out", false}, {offsets_out, (n + 1) * 4, "d_offsets_out", false}},
                      num_runs_out, work))
        return ADLHIP_FAILURE;
    const size_t need = reduce_layout(d, n).total;
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_reduce_runs_scratch_bytes)", work_bytes, need);
    return ADLHIP_BY_WIDTH(key_bytes, K, ADLHIP_BY_WIDTH(v.bytes, W, reduce_stage<K, W>(d, (const K*)keys_in, (const W*)vals_in, n, v.kind, op,
                           (K*)unique_out, (W*)reduced_out, counts_out, offsets_out, num_runs_out, work)));
}

int adlhip_reduce_by_key_scratch_bytes(adlhip_device* d, int key_type, int value_type, size_t n, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    TypeInfo t, v;
    if (key_type_info(key_type, ADLHIP_ORDER_ASCENDING, &t) || reduce_value_info(value_type, ADLHIP_REDUCE_SUM, &v) || typed_check_n(n))
        return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = reduce_by_key_layout(d, (size_t)t.bytes, (size_t)v.bytes, n).total;
    return ADLHIP_SUCCESS;
}

int adlhip_reduce_by_key_typed(adlhip_device* d, int key_type, int order, const void* keys_in, int value_type, int op, const void* vals_in,
                               size_t n, void* unique_out, void* reduced_out, uint32_t* counts_out, uint32_t* offsets_out,
                               uint32_t* num_unique_out, void* work, size_t work_bytes)
{
    TypeInfo t, v;
    if (bind(d) || key_type_info(key_type, order, &t) || reduce_value_info(value_type, op, &v) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (const int rc = count_word(d, "reduce by key", "d_num_unique_out", num_unique_out, n); rc || n == 0) return rc;
    if (check_buffers("reduce by key", {{keys_in, n * (size_t)t.bytes, "d_keys_in"}, {vals_in, n * (size_t)v.bytes, "d_vals_in"}},
                      {{unique_out, n * (size_t)t.bytes, "d_unique_out"}, {reduced_out, n * (size_t)v.bytes, "d_reduced_out"},
                       {counts_out, n * 4, "d_counts_out", false}, {offsets_out, (n + 1) * 4, "d_offsets_out", false}},
                      num_unique_out, work))
        return ADLHIP_FAILURE;
    const size_t need = reduce_by_key_layout(d, (size_t)t.bytes, (size_t)v.bytes, n).total;
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_reduce_by_key_scratch_bytes)", work_bytes, need);
    return ADLHIP_BY_WIDTH(t.bytes, K, ADLHIP_BY_WIDTH(v.bytes, W, reduce_by_key_run<K, W>(d, t, order, (const K*)keys_in, (const W*)vals_in, n,
                           v.kind, op, (K*)unique_out, (W*)reduced_out, counts_out, offsets_out, num_unique_out, work)));
}

// ---- typed scans ------------------------------------------------------------------------------------
int adlhip_scan_typed_scratch_bytes(adlhip_device* d, int value_type, size_t n, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    TypeInfo v;
    if (reduce_value_info(value_type, ADLHIP_REDUCE_SUM, &v) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = scan_layout(d).total;
    return ADLHIP_SUCCESS;
}

int adlhip_scan_typed(adlhip_device* d, int value_type, int op, int exclusive, const void* h_init, const void* vals_in, void* out, size_t n,
                      void* work, size_t work_bytes)
{
    TypeInfo v;
    bool done;
    if (bind(d) || reduce_value_info(value_type, op, &v)) return ADLHIP_FAILURE;
    if (const int rc = scan_check(d, "scan", "adlhip_scan_typed_scratch_bytes", 0, nullptr, v, exclusive, h_init, vals_in, out, n, work,
                                  work_bytes, &done); rc || done)
        return rc;
    return ADLHIP_BY_WIDTH(v.bytes, W, scan_stage<adlhip::ScanNoKey, W>(d, nullptr, (const W*)vals_in, (W*)out, n, v.kind, op, exclusive, h_init, work));
}

int adlhip_scan_by_key_scratch_bytes(adlhip_device* d, int key_bytes, int value_type, size_t n, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    TypeInfo v;
    if (check_key_bytes("scan by key", key_bytes) || reduce_value_info(value_type, ADLHIP_REDUCE_SUM, &v) || typed_check_n(n))
        return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = scan_layout(d).total;
    return ADLHIP_SUCCESS;
}

int adlhip_scan_by_key(adlhip_device* d, int key_bytes, const void* keys_in, int value_type, int op, int exclusive, const void* h_init,
                       const void* vals_in, void* out, size_t n, void* work, size_t work_bytes)
{
    TypeInfo v;
    bool done;
    if (bind(d) || check_key_bytes("scan by key", key_bytes) || reduce_value_info(value_type, op, &v)) return ADLHIP_FAILURE;
    if (const int rc = scan_check(d, "scan by key", "adlhip_scan_by_key_scratch_bytes", key_bytes, keys_in, v, exclusive, h_init, vals_in, out,
                                  n, work, work_bytes, &done); rc || done)
        return rc;
    return ADLHIP_BY_WIDTH(key_bytes, K, ADLHIP_BY_WIDTH(v.bytes, W, scan_stage<K, W>(d, (const K*)keys_in, (const W*)vals_in, (W*)out, n, v.kind,
                           op, exclusive, h_init, work)));
}

// ---- stream compaction ------------------------------------------------------------------------------
int adlhip_compact_scratch_bytes(adlhip_device* d, size_t n, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    if (typed_check_n(n)) return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = compact_work_bytes(d);
    return ADLHIP_SUCCESS;
}

int adlhip_compact_flagged(adlhip_device* d, int item_bytes, const void* items_in, const uint8_t* flags_in, size_t n, int partition,
                           void* items_out, uint32_t* index_out, uint32_t* num_selected_out, void* work, size_t work_bytes)
{
    const char* what = "compact flagged";
    if (bind(d) || compact_check_width(what, "item_bytes", item_bytes, true, items_in, items_out) || compact_check_partition(what, partition) ||
        typed_check_n(n))
        return ADLHIP_FAILURE;
    if (!items_out && !index_out) return fail("%s: at least one of d_items_out and d_index_out must be given", what);
    if (const int rc = count_word(d, what, "d_num_selected_out", num_selected_out, n); rc || n == 0) return rc;
    const size_t ib = n * (size_t)item_bytes;
    if (check_buffers(what, {{flags_in, n, "d_flags_in"}, {items_in, ib, "d_items_in", item_bytes != 0}},
                      {{items_out, ib, "d_items_out", false}, {index_out, n * 4, "d_index_out", false}}, num_selected_out, work))
        return ADLHIP_FAILURE;
    const size_t need = compact_work_bytes(d);
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_compact_scratch_bytes)", work_bytes, need);
    const adlhip::CompactPred pr = {0u, 0u, 0u};
    return ADLHIP_BY_WIDTH(item_bytes ? item_bytes : 4, V, compact_stage<uint8_t, V>(d, flags_in, pr, (const V*)items_in, n, partition, nullptr,
                                                                                      (V*)items_out, index_out, num_selected_out, work));
}

int adlhip_compact_if_typed(adlhip_device* d, int key_type, int cmp, const void* h_threshold, const void* keys_in, int value_bytes,
                            const void* vals_in, size_t n, int partition, void* keys_out, void* vals_out, uint32_t* index_out,
                            uint32_t* num_selected_out, void* work, size_t work_bytes)
{
    const char* what = "compact if";
    TypeInfo t;
    if (bind(d) || type_info("key_type", key_type, &t)) return ADLHIP_FAILURE;
    if (cmp < ADLHIP_CMP_LT || cmp > ADLHIP_CMP_NE) return fail("%s: cmp must be one of ADLHIP_CMP_LT .. ADLHIP_CMP_NE (0..5), got %d", what, cmp);
    if (compact_check_width(what, "value_bytes", value_bytes, true, vals_in, vals_out) || compact_check_partition(what, partition) ||
        typed_check_n(n))
        return ADLHIP_FAILURE;
    if (!h_threshold) return fail("%s: h_threshold is required", what);
    if (!keys_out && !vals_out && !index_out) return fail("%s: at least one of d_keys_out, d_vals_out and d_index_out must be given", what);
    if (const int rc = count_word(d, what, "d_num_selected_out", num_selected_out, n); rc || n == 0) return rc;
    const size_t kb = n * (size_t)t.bytes, vb = n * (size_t)value_bytes;
    if (check_buffers(what, {{keys_in, kb, "d_keys_in"}, {vals_in, vb, "d_vals_in", value_bytes != 0}},
                      {{keys_out, kb, "d_keys_out", false}, {vals_out, vb, "d_vals_out", false}, {index_out, n * 4, "d_index_out", false}},
                      num_selected_out, work))
        return ADLHIP_FAILURE;
    const size_t need = compact_work_bytes(d);
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_compact_scratch_bytes)", work_bytes, need);
    // the threshold's code, as the kernels encode the keys
    uint64_t bits = 0;
    __builtin_memcpy(&bits, h_threshold, (size_t)t.bytes);   // (little endian: a 4-byte key lands in the low dword)
    uint64_t code = 0;
#define ADLHIP_THRESHOLD(KIND_, DESC_) \
    code = t.bytes == 4 ? (uint64_t)adlhip::key_enc<uint32_t, KIND_, 0>((uint32_t)bits) : adlhip::key_enc<uint64_t, KIND_, 0>(bits)
    ADLHIP_TYPED_DISPATCH(t.kind, 0, ADLHIP_THRESHOLD);
#undef ADLHIP_THRESHOLD
    const adlhip::CompactPred pr = {(uint32_t)t.kind, (uint32_t)cmp, code};
    return ADLHIP_BY_WIDTH(t.bytes, K, ADLHIP_BY_WIDTH(value_bytes ? value_bytes : 4, V, compact_stage<K, V>(d, (const K*)keys_in, pr,
                           (const V*)vals_in, n, partition, (K*)keys_out, (V*)vals_out, index_out, num_selected_out, work)));
}

// ---- histograms --------------------------------------------------------------------------------------
int adlhip_histogram_scratch_bytes(adlhip_device* d, int key_type, size_t n, size_t num_bins, int by_edges, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    if (by_edges != 0 && by_edges != 1) return fail("histogram scratch: by_edges must be 0 (bincount) or 1 (range), got %d", by_edges);
    TypeInfo t;
    if (hist_check_mode("histogram scratch", key_type, num_bins, by_edges != 0, &t) || typed_check_n(n)) return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = hist_work_bytes(d, (size_t)t.bytes, n, num_bins, by_edges != 0);
    return ADLHIP_SUCCESS;
}

int adlhip_histogram_range_typed(adlhip_device* d, int key_type, const void* keys_in, size_t n, const void* edges_in, size_t num_bins,
                                 int include_upper, uint32_t* counts_out, void* work, size_t work_bytes)
{
    const char* what = "histogram range";
    TypeInfo t;
    bool done;
    if (bind(d) || hist_check_mode(what, key_type, num_bins, true, &t)) return ADLHIP_FAILURE;
    if (include_upper != 0 && include_upper != 1) return fail("%s: include_upper must be 0 or 1, got %d", what, include_upper);
    if (!edges_in) return fail("null buffer passed to %s", what);
    if (check_aligned16(what, {edges_in})) return ADLHIP_FAILURE;
    if (overlaps(counts_out, num_bins * 4, edges_in, (num_bins + 1) * (size_t)t.bytes)) return fail("%s: d_counts_out must not overlap d_edges_in", what);
    if (const int rc = hist_check(d, what, t, keys_in, n, edges_in, num_bins, true, counts_out, work, work_bytes, &done); rc || done) return rc;
    return ADLHIP_BY_WIDTH(t.bytes, U, hist_lds_stage<U, adlhip::kHistRange>(d, (const U*)keys_in, n, (const U*)edges_in, t.kind, num_bins, include_upper,
                                                                            counts_out, work));
}

int adlhip_bincount_typed(adlhip_device* d, int key_type, const void* keys_in, size_t n, size_t num_bins, uint32_t* counts_out, void* work,
                          size_t work_bytes)
{
    const char* what = "bincount";
    TypeInfo t;
    bool done;
    if (bind(d) || hist_check_mode(what, key_type, num_bins, false, &t)) return ADLHIP_FAILURE;
    if (const int rc = hist_check(d, what, t, keys_in, n, nullptr, num_bins, false, counts_out, work, work_bytes, &done); rc || done) return rc;
    if (hist_lds_path(d, false, num_bins))
        return ADLHIP_BY_WIDTH(t.bytes, U, hist_lds_stage<U, adlhip::kHistBincount>(d, (const U*)keys_in, n, (const U*)nullptr, t.kind, num_bins, 0,
                                                                                   counts_out, work));
    return ADLHIP_BY_WIDTH(t.bytes, U, hist_sorted_stage<U>(d, (const U*)keys_in, n, num_bins, counts_out, work));
}

// ---- merge of sorted sequences -------------------------------------------------------------------------
int adlhip_merge_scratch_bytes(adlhip_device* d, int key_type, int value_bytes, size_t na, size_t nb, size_t* work_bytes)
{
    const char* what = "merge scratch";
    if (!d) return fail("null device handle");
    TypeInfo t;
    size_t n;
    if (type_info("key_type", key_type, &t) || merge_check_value_bytes(what, value_bytes) || merge_total(what, na, nb, &n)) return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = merge_work_bytes(n);
    return ADLHIP_SUCCESS;
}

int adlhip_merge_typed(adlhip_device* d, int key_type, int order, const void* keys_a, const void* vals_a, size_t na, const void* keys_b,
                       const void* vals_b, size_t nb, int value_bytes, void* keys_out, void* vals_out, uint32_t* index_out, void* work,
                       size_t work_bytes)
{
    const char* what = "merge";
    TypeInfo t;
    size_t n;
    if (bind(d) || key_type_info(key_type, order, &t) || merge_check_value_bytes(what, value_bytes) || merge_total(what, na, nb, &n))
        return ADLHIP_FAILURE;
    if (value_bytes == 0 && (vals_a || vals_b || vals_out))
        return fail("%s: value_bytes is 0, so d_vals_a, d_vals_b and d_vals_out must be NULL", what);
    if (!keys_out && !vals_out && !index_out) return fail("%s: at least one of d_keys_out, d_vals_out and d_index_out must be given", what);
    if (n == 0) return ADLHIP_SUCCESS;
    const size_t kb = (size_t)t.bytes, vb = (size_t)value_bytes, va = vb ? vb : 1;
    if (merge_check_buffers(what,
                            {{keys_a, na * kb, "d_keys_a", na != 0, kb}, {keys_b, nb * kb, "d_keys_b", nb != 0, kb},
                             {vals_a, na * vb, "d_vals_a", vb && na, va}, {vals_b, nb * vb, "d_vals_b", vb && nb, va}},
                            {{keys_out, n * kb, "d_keys_out", false, 16}, {vals_out, n * vb, "d_vals_out", vb != 0, 16},
                             {index_out, n * 4, "d_index_out", false, 16}, {work, work_bytes, "d_work", true, 16}}))
        return ADLHIP_FAILURE;
    const size_t need = merge_work_bytes(n);
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_merge_scratch_bytes)", work_bytes, need);
    const adlhip::RedCodec codec = {(uint32_t)t.kind, (uint32_t)order};
    return ADLHIP_BY_WIDTH(t.bytes, K, ADLHIP_BY_WIDTH(value_bytes ? value_bytes : 4, V, merge_stage<K, V>(d, codec, (const K*)keys_a,
                           (const V*)vals_a, na, (const K*)keys_b, (const V*)vals_b, nb, (K*)keys_out, (V*)vals_out, index_out, work)));
}

// ---- set operations on sorted sequences ----------------------------------------------------------------
int adlhip_set_op_scratch_bytes(adlhip_device* d, int key_type, int value_bytes, size_t na, size_t nb, size_t* work_bytes)
{
    const char* what = "set op scratch";
    if (!d) return fail("null device handle");
    TypeInfo t;
    size_t n;
    if (type_info("key_type", key_type, &t) || merge_check_value_bytes(what, value_bytes) || merge_total(what, na, nb, &n)) return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = setop_work_bytes(d, n);
    return ADLHIP_SUCCESS;
}

int adlhip_set_op_typed(adlhip_device* d, int key_type, int order, int op, const void* keys_a, const void* vals_a, size_t na, const void* keys_b,
                        const void* vals_b, size_t nb, int value_bytes, void* keys_out, void* vals_out, uint32_t* index_out, uint32_t* num_out,
                        void* work, size_t work_bytes)
{
    const char* what = "set op";
    TypeInfo t;
    size_t n;
    if (bind(d) || key_type_info(key_type, order, &t)) return ADLHIP_FAILURE;
    if (op < ADLHIP_SETOP_INTERSECTION || op > ADLHIP_SETOP_SYMMETRIC_DIFFERENCE)
        return fail("%s: op must be one of ADLHIP_SETOP_INTERSECTION .. ADLHIP_SETOP_SYMMETRIC_DIFFERENCE (0..3), got %d", what, op);
    if (merge_check_value_bytes(what, value_bytes) || merge_total(what, na, nb, &n)) return ADLHIP_FAILURE;
    if (value_bytes == 0 && (vals_a || vals_b || vals_out))
        return fail("%s: value_bytes is 0, so d_vals_a, d_vals_b and d_vals_out must be NULL", what);
    if (!keys_out && !vals_out && !index_out) return fail("%s: at least one of d_keys_out, d_vals_out and d_index_out must be given", what);
    if (!num_out) return fail("%s: d_num_out is required", what);
    const bool both = op == ADLHIP_SETOP_UNION || op == ADLHIP_SETOP_SYMMETRIC_DIFFERENCE;
    const size_t cap = both ? n : na;   // what every output holds
    const size_t kb = (size_t)t.bytes, vb = (size_t)value_bytes, va = vb ? vb : 1;
    if (merge_check_buffers(what,
                            {{keys_a, na * kb, "d_keys_a", na != 0, kb}, {keys_b, nb * kb, "d_keys_b", nb != 0, kb},
                             {vals_a, na * vb, "d_vals_a", vb && na, va}, {vals_b, nb * vb, "d_vals_b", vb && nb, va}},
                            {{keys_out, cap * kb, "d_keys_out", false, 16}, {vals_out, cap * vb, "d_vals_out", vb && cap, 16},
                             {index_out, cap * 4, "d_index_out", false, 16}, {num_out, 4, "d_num_out", true, 4},
                             {work, work_bytes, "d_work", n != 0, 16}}))
        return ADLHIP_FAILURE;
    const size_t need = n ? setop_work_bytes(d, n) : 0;
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_set_op_scratch_bytes)", work_bytes, need);
    if (n == 0) {
        HIPCHK(hipMemsetAsync(num_out, 0, 4, d->stream));
        return ADLHIP_SUCCESS;
    }
    const adlhip::RedCodec codec = {(uint32_t)t.kind, (uint32_t)order};
    return ADLHIP_BY_WIDTH(t.bytes, K, ADLHIP_BY_WIDTH(value_bytes ? value_bytes : 4, V, setop_stage<K, V>(d, codec, (uint32_t)op,
                           (const K*)keys_a, (const V*)vals_a, na, (const K*)keys_b, (const V*)vals_b, nb, cap, (K*)keys_out, (V*)vals_out,
                           index_out, num_out, work)));
}

// ---- sorted search --------------------------------------------------------------------------------------
int adlhip_search_sorted_typed(adlhip_device* d, int key_type, int order, int side, const void* sorted, size_t m, const void* needles, size_t n,
                               uint32_t* pos_out)
{
    const char* what = "search sorted";
    TypeInfo t;
    if (bind(d) || key_type_info(key_type, order, &t)) return ADLHIP_FAILURE;
    if (side != ADLHIP_SEARCH_LEFT && side != ADLHIP_SEARCH_RIGHT)
        return fail("%s: side must be ADLHIP_SEARCH_LEFT (0) or ADLHIP_SEARCH_RIGHT (1), got %d", what, side);
    if (m > kSearchMaxElems) return fail("%s: m = %zu exceeds the supported maximum %zu", what, m, (size_t)kSearchMaxElems);
    if (n > kSearchMaxElems) return fail("%s: n = %zu exceeds the supported maximum %zu", what, n, (size_t)kSearchMaxElems);
    if (n == 0) return ADLHIP_SUCCESS;
    const size_t kb = (size_t)t.bytes;
    if (merge_check_buffers(what, {{m ? sorted : nullptr, m * kb, "d_sorted", m != 0, kb}, {needles, n * kb, "d_needles", true, 16}},
                            {{pos_out, n * 4, "d_pos_out", true, 16}}))
        return ADLHIP_FAILURE;
    const adlhip::RedCodec codec = {(uint32_t)t.kind, (uint32_t)order};
    return ADLHIP_BY_WIDTH(t.bytes, U, search_stage<U>(d, codec, side, (const U*)sorted, m, (const U*)needles, n, pos_out));
}

// ---- expansion of runs -----------------------------------------------------------------------------------
int adlhip_expand_scratch_bytes(adlhip_device* d, size_t num_runs, size_t cap, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    if (expand_check_sizes("expand scratch", "num_runs", num_runs, cap)) return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = expand_work_bytes(d, num_runs, cap);
    return ADLHIP_SUCCESS;
}

int adlhip_expand_runs(adlhip_device* d, const uint32_t* counts_in, size_t num_runs, int value_bytes, const void* vals_in, size_t cap,
                       uint32_t* run_out, uint32_t* rank_out, void* vals_out, uint64_t* num_out, void* work, size_t work_bytes)
{
    const char* what = "expand runs";
    if (bind(d) || merge_check_value_bytes(what, value_bytes) || expand_check_sizes(what, "num_runs", num_runs, cap)) return ADLHIP_FAILURE;
    if (value_bytes == 0 && (vals_in || vals_out)) return fail("%s: value_bytes is 0, so d_vals_in and d_vals_out must be NULL", what);
    if (cap == 0 && (run_out || rank_out || vals_out))
        return fail("%s: cap is 0, so d_run_out, d_rank_out and d_vals_out must be NULL", what);
    if (cap != 0 && !run_out && !rank_out && !vals_out)
        return fail("%s: cap is %zu, so at least one of d_run_out, d_rank_out and d_vals_out must be given", what, cap);
    if (vals_out && !vals_in) return fail("%s: d_vals_in is required with d_vals_out", what);
    const size_t n = num_runs, vb = (size_t)value_bytes, va = vb ? vb : 1;
    if (merge_check_buffers(what, {{counts_in, n * 4, "d_counts_in", n != 0, 4}, {vals_out ? vals_in : nullptr, n * vb, "d_vals_in", false, va}},
                            {{run_out, cap * 4, "d_run_out", false, 16}, {rank_out, cap * 4, "d_rank_out", false, 16},
                             {vals_out, cap * vb, "d_vals_out", false, 16}, {num_out, 8, "d_num_out", true, 8},
                             {work, work_bytes, "d_work", n != 0, 16}}))
        return ADLHIP_FAILURE;
    const size_t need = n ? expand_work_bytes(d, n, cap) : 0;
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_expand_scratch_bytes)", work_bytes, need);
    if (n == 0) {
        HIPCHK(hipMemsetAsync(num_out, 0, 8, d->stream));
        return ADLHIP_SUCCESS;
    }
    if (!vals_out)
        return expand_stage<adlhip::MergeNone>(d, counts_in, n, cap, (const adlhip::MergeNone*)nullptr, run_out, rank_out,
                                               (adlhip::MergeNone*)nullptr, num_out, work);
    return ADLHIP_BY_WIDTH(value_bytes, V, expand_stage<V>(d, counts_in, n, cap, (const V*)vals_in, run_out, rank_out, (V*)vals_out, num_out, work));
}

// ---- join of sorted sequences ----------------------------------------------------------------------------
int adlhip_join_scratch_bytes(adlhip_device* d, int key_type, size_t na, size_t nb, size_t cap, size_t* work_bytes)
{
    const char* what = "join scratch";
    if (!d) return fail("null device handle");
    TypeInfo t;
    size_t n;
    if (type_info("key_type", key_type, &t) || merge_total(what, na, nb, &n) || expand_check_sizes(what, "na", na, cap)) return ADLHIP_FAILURE;
    if (work_bytes) *work_bytes = join_work_bytes(d, na, cap);
    return ADLHIP_SUCCESS;
}

int adlhip_join_sorted_typed(adlhip_device* d, int key_type, int order, int kind, const void* keys_a, size_t na, const void* keys_b, size_t nb,
                             size_t cap, uint32_t* index_a_out, uint32_t* index_b_out, uint64_t* num_out, void* work, size_t work_bytes)
{
    const char* what = "join";
    TypeInfo t;
    size_t n;
    if (bind(d) || key_type_info(key_type, order, &t)) return ADLHIP_FAILURE;
    if (kind < ADLHIP_JOIN_INNER || kind > ADLHIP_JOIN_ANTI)
        return fail("%s: kind must be one of ADLHIP_JOIN_INNER .. ADLHIP_JOIN_ANTI (0..3), got %d", what, kind);
    if (merge_total(what, na, nb, &n) || expand_check_sizes(what, "na", na, cap)) return ADLHIP_FAILURE;
    if (cap == 0 && (index_a_out || index_b_out)) return fail("%s: cap is 0, so d_index_a_out and d_index_b_out must be NULL", what);
    if (cap != 0 && !index_a_out && !index_b_out)
        return fail("%s: cap is %zu, so at least one of d_index_a_out and d_index_b_out must be given", what, cap);
    const size_t kb = (size_t)t.bytes;
    if (merge_check_buffers(what, {{keys_a, na * kb, "d_keys_a", na != 0, kb}, {keys_b, nb * kb, "d_keys_b", nb != 0, kb}},
                            {{index_a_out, cap * 4, "d_index_a_out", false, 16}, {index_b_out, cap * 4, "d_index_b_out", false, 16},
                             {num_out, 8, "d_num_out", true, 8}, {work, work_bytes, "d_work", na != 0, 16}}))
        return ADLHIP_FAILURE;
    const size_t need = na ? join_work_bytes(d, na, cap) : 0;
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_join_scratch_bytes)", work_bytes, need);
    if (na == 0) {
        HIPCHK(hipMemsetAsync(num_out, 0, 8, d->stream));
        return ADLHIP_SUCCESS;
    }
    const adlhip::RedCodec codec = {(uint32_t)t.kind, (uint32_t)order};
    return ADLHIP_BY_WIDTH(t.bytes, K, join_stage<K>(d, codec, (uint32_t)kind, (const K*)keys_a, na, (const K*)keys_b, nb, cap, index_a_out,
                                                    index_b_out, num_out, work));
}

}  // extern "C"
