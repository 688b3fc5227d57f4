// large_plan_dump.cpp -- prints what oclradixsort_amd/csrc/large_plan.hpp decides, for tests/test_large_plan.py.  Host code only: no
// HIP call, no GPU, nothing of the library linked.
//
// stdin, one case per line:  kind sort_bits msd2 rank persist resident n offered
//   kind = ADLHIP_ELEM_*; msd2 / rank / persist / resident = "sort.msd2", "sort.rank", "sort.persist", "debug.resident_wgs";
//   offered = the work bytes the caller brings: l0 (nothing the large sort could use), l2, l1 (the large sort's term of the scratch
//   query at that level), m02 and m21 (the midpoints between them)
// stdout, one row per case: the case, then name=value pairs -- the sizing (l1, l2), the four layouts a (kind, n, sort_bits) can have
// with their totals (-1: not eligible), the preferred form, the plan and its layout, and whether a buffer of exactly the plan's
// work_bytes yields the same plan again.
#include "large_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>

using namespace adlhip_internal;

static const char* form_name(LargeForm f)
{
    return f == kLargeCursor ? "cursor" : f == kLargeStable ? "stable" : f == kLargeHybrid ? "hybrid" : "none";
}

static bool same_plan(const LargePlan& a, const LargePlan& b)
{
    return a.form == b.form && a.lean == b.lean && a.headroom_pct == b.headroom_pct && a.slab16 == b.slab16 && a.bin == b.bin &&
           a.work_bytes == b.work_bytes && a.L.total == b.L.total && a.L.stride_a == b.L.stride_a && a.L.stride_b == b.L.stride_b;
}

int main()
{
    adlhip_device d;   // the knobs' defaults; what a device answers at creation is set per case
    d.rank_mode = 1;
    int kind, sort_bits, msd2, rank, persist, resident;
    unsigned long long n_in;
    char offered_name[8];
    while (scanf("%d %d %d %d %d %d %llu %7s", &kind, &sort_bits, &msd2, &rank, &persist, &resident, &n_in, offered_name) == 8) {
        const size_t n = (size_t)n_in;
        d.msd2_path = msd2;
        d.rank_mode = rank;
        d.persist = persist;
        d.resident_wgs = resident;
        const size_t eb = kind == ADLHIP_ELEM_U32 ? 4 : 8;
        const int max_bits = kind == ADLHIP_ELEM_U64 ? 64 : 32;
        const bool keys = kind == ADLHIP_ELEM_U32 || kind == ADLHIP_ELEM_U64;
        const bool whole = sort_bits == max_bits;
        const size_t l1 = large_work_bytes_at(kind, n, sort_bits, 1), l2 = large_work_bytes_at(kind, n, sort_bits, 2);
        size_t offered;
        if (!strcmp(offered_name, "l0")) offered = 0;
        else if (!strcmp(offered_name, "l2")) offered = l2;
        else if (!strcmp(offered_name, "l1")) offered = l1;
        else if (!strcmp(offered_name, "m02")) offered = l2 / 2;
        else if (!strcmp(offered_name, "m21")) offered = l2 + (l1 - l2) / 2;
        else return 2;
        // the layouts this (kind, n, sort_bits) can have, by the header's own conditions
        const bool co = cursor_eligible(eb, keys, whole, n), so = stable_eligible(n);
        const long long t_cf = co ? (long long)large_layout({kLargeCursor, false}, n, eb, whole).total : -1;
        const long long t_cl = co ? (long long)large_layout({kLargeCursor, true}, n, eb, whole).total : -1;
        const long long t_sf = so ? (long long)large_layout({kLargeStable, false}, n, eb, whole).total : -1;
        const long long t_sl = so ? (long long)large_layout({kLargeStable, true}, n, eb, whole).total : -1;
        const LargeForm preferred = large_sort_form(&d, eb, keys, n, sort_bits, max_bits);
        const LargePlan P = large_plan(&d, eb, keys, n, sort_bits, max_bits, offered);
        const LargePlan again = large_plan(&d, eb, keys, n, sort_bits, max_bits, P.work_bytes);
        printf("%d %d %d %d %d %d %llu %s offered=%zu l1=%zu l2=%zu cursor_full=%lld cursor_lean=%lld stable_full=%lld stable_lean=%lld "
               "preferred=%s form=%s lean=%d headroom=%d slab16=%d bin=%d seg_shift=%u stride_a=%u stride_b=%u tier_b=%u pieces=%u slice=%u "
               "tiles_per_bucket=%u slab_b_in_tmp=%d total=%zu work_bytes=%zu again=%d\n",
               kind, sort_bits, msd2, rank, persist, resident, n_in, offered_name, offered, l1, l2, t_cf, t_cl, t_sf, t_sl,
               form_name(preferred), form_name(P.form), (int)P.lean, P.headroom_pct, (int)P.slab16, (int)P.bin, P.L.seg_shift, P.L.stride_a,
               P.L.stride_b, P.L.tier_b, P.L.pieces, P.L.slice, P.L.tiles_per_bucket, (int)P.L.slab_b_in_tmp, P.L.total, P.work_bytes,
               (int)(P.form == kLargeNone || same_plan(P, again)));
    }
    return 0;
}
