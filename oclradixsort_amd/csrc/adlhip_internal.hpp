// adlhip_internal.hpp -- what the library's three host units share.  handle.hip defines the runtime under everything: the error text,
// the handle (create, teardown, sync, buffers, map / unmap, events, profiling), the probes and the knob table.  adlhip.hip defines
// the sorts, the scan and the partitions, and what a handle owns for them (sort_state_create / sort_state_destroy, the idle table).
// primitives.hip defines what is built on top of the sorts (typed sort, top-k, unique, reduce by key, scans, compaction, histograms, merges, set operations, sorted search, joins).
// Not installed; nothing here is ABI.
#pragma once
#include "../../include/adlhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

namespace adlhip { struct DictBlock; }   // dict_build.hpp

namespace adlhip_internal {
// the largest table of the histogram's LDS path: the default and the ceiling of "debug.histogram_lds_bins".  primitives.hip asserts
// that it is what the count kernel's LDS is sized for (adlhip::kHistLdsBins, histogram_kernels.hpp)
constexpr int kHistogramLdsBinsMax = 8192;
// the table of the sorted search in LDS: the default and the ceiling of "debug.search_lds_keys".  primitives.hip asserts that it is the
// kernel's (adlhip::kSearchLdsKeys, search_kernels.hpp)
constexpr int kSearchLdsKeysMax = 4096;
struct ProfEntry {
    uint64_t launches = 0;
    double total_ms = 0.0;
};
struct PendingProf {
    const char* name;
    hipEvent_t e0, e1;
};
struct Staging {
    void* hptr;
    size_t bytes;      // bytes mapped
    hipEvent_t done;   // null while mapped; set at unmap
    size_t capacity;   // bytes of pinned memory behind hptr (>= bytes when it came from the pool)
};
struct PinnedBlock {
    void* hptr;
    size_t capacity;
};
}  // namespace adlhip_internal

struct adlhip_event {
    hipEvent_t ev;
};

struct adlhip_device {
    int idx = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    hipDeviceProp_t prop;
    uint64_t used_bytes = 0;
    // ---- knobs: one row each in kKnobs (handle.hip), in this order ---------------------------------------------------------------
    int sort_algo = -1;       // "sort.algo": -1 automatic by size, 0 onesweep, 1 three-kernel pass
    int mid_path = 1;         // "sort.mid": 16 Ki < n <= 2 Mi: MSD pass + LDS finish (three launches) instead of per-digit passes
    int msd2_path = 1;        // "sort.msd2": the large sort (msd2_sort for keys, msd2s_sort for pairs); 2 = forced (tests)
    int persist = 1;          // "sort.persist": the cursor passes of the large sort as persistent, prefetching kernels + the 16-bit finish
    int dict_path = 1;        // "sort.dict": the large sort's safety net first tries the counting sort for keys that take at most
                              // 256 values (dict_kernels.hpp); 0 = off
    int bin_finish = 1;       // "sort.binfinish": the large keys-only sort finishes its segments with one counting pass + compares
                              // (1: u64 keys, 2: u32 keys too, 0: the wave-per-segment LSD finish)
    int topk_algo = -1;       // "topk.algo": -1 selection up to kTopkSelectMaxFraction of n, the full argsort above; 0 / 1 force
                              // the argsort / the selection
    int topk_rows_algo = -1;  // "topk.rows_algo": -1 the row kernel while k <= kRowMaxK and cols <= kTopkRowsMaxCols, the per-row
                              // loop above; 0 / 1 force the loop / the row kernel
    int topk_rows_grid = 0;   // "debug.topk_rows_grid": workgroups of the row kernel at most (0: kTopkRowsWgsPerCu per CU)
    int sort_rows_algo = -1;  // "sort.rows_algo": -1 the row kernel while cols <= kRowCap, the flat path above; 0 / 1 force the flat
                              // path / the row kernel
    int sort_rows_grid = 0;   // "debug.sort_rows_grid": workgroups of the sort's row kernel at most (0: kSortRowsWgsPerCu per CU)
    int sort_segments_algo = -1;  // "sort.segments_algo": -1 the segment kernel while 0 < max_segment <= kRowCap, the flat path
                                  // otherwise; 0 / 1 force the flat path / the segment kernel
    int sort_segments_grid = 0;   // "debug.sort_segments_grid": workgroups of the segment kernel at most (0: what its LDS admits per CU)
    int unique_grid = 0;      // "debug.unique_grid": workgroups of the run stage at most (0: kUniqueWgsPerCu per CU)
    int reduce_grid = 0;      // "debug.reduce_grid": workgroups of the reduce stage at most (0: kReduceWgsPerCu per CU)
    int scan_grid = 0;        // "debug.scan_grid": workgroups of the scan stage at most (0: kScanWgsPerCu per CU)
    int compact_grid = 0;     // "debug.compact_grid": workgroups of the compaction at most (0: kCompactWgsPerCu per CU)
    int histogram_grid = 0;   // "debug.histogram_grid": workgroups of the histogram's count kernel at most (0: hist_grid_cap)
    int merge_grid = 0;       // "debug.merge_grid": workgroups of the merge's tile kernel at most (0: kMergeWgsPerCu per CU)
    int setop_grid = 0;       // "debug.setop_grid": workgroups of the set operations' count and emit kernels at most (0: kSetopWgsPerCu per CU)
    int search_grid = 0;      // "debug.search_grid": workgroups of the sorted search at most (0: kSearchWgsPerCu per CU)
    int join_grid = 0;        // "debug.join_grid": workgroups of the join's and the expansion's bounds, sum, starts and row kernels at most (0: kJoinWgsPerCu per CU)
    int persist_grid = 0;     // "debug.persist_grid": workgroups of the large sort's persistent passes, rounded up to a
                              // multiple of 8 (0: two per CU)
    // (with a rule of their own)
    int digit_bits = 8;       // "sort.digit_bits": 8 or 4
    int unique_algo = -1;     // "unique.algo": -1 the keys path unless first_index or inverse is asked, 1 always the index path
    int tile_variant = -1;    // "sort.tile": index into kVariants; -1 = best known per element size
    int net_lookback = 1;     // "sort.net_lookback": the large sort's safety net runs look-back passes (0: count-scan-scatter passes)
    int partition_lookback = 1;   // "partition.lookback": the MSB partition as one look-back pass where it pays (0: always three kernels)
    int profile = 0;          // "profile": an event pair around every launch
    int histogram_lds_bins = adlhip_internal::kHistogramLdsBinsMax;   // "debug.histogram_lds_bins": bincount takes the LDS path up to this many bins
    int search_lds_keys = adlhip_internal::kSearchLdsKeysMax;   // "debug.search_lds_keys": codes of the sorted search's table in LDS at most
    int resident_wgs = 0;     // "debug.resident_wgs": workgroups of <= 80 KiB LDS / 512 threads that are certainly resident at once (2 per
                              // CU); the paths whose kernels hold a grid-wide barrier over 256 workgroups are taken only when this is >= 256
    int rank_mode = 1;        // "sort.rank": 1 = lane-ordered DS atomic ranking (needs lds_ordered), 0 = ballot match
    int lds_ordered = 0;      // "sort.lds_ordered" (read only): result of the device self-test at creation
    // ---- not knobs ----------------------------------------------------------------------------------------------------------------
    int resident_wgs_device = 0;   // what the device answered at creation ("debug.resident_wgs" = 0 restores it)
    int mid_skip = 0;         // eligible sorts still to be sent down the per-digit passes after a skewed input (see mid_eligible)
    int mid2_skip = 0;        // keys-only sorts still to take the three-launch form after a slab overflow (see mid_sort_keys)
    int mid_backoff = 32, mid2_backoff = 64;
    // the sorts' device state (sort_state_create / sort_state_destroy, adlhip.hip)
    adlhip::DictBlock* d_dict = nullptr;    // the net's dictionary and counters (rebuilt by every net that uses them)
    uint32_t* d_msd2 = nullptr;   // the large sort's handle-owned words, allocated with the handle: cursors of pass 1 (256, one
                                  // 128-byte line each) and pass 2 (65536), overflow flag, done counter, the safety net's barrier
                                  // counter, the four sample words, ...; what each holds between sorts: kIdleTable
    uint32_t* d_mid_hist = nullptr;    // [16][4][256] slice histograms of the mid-size sort + 512 words of bucket cursors / flags
                                       // of its keys-only form (hybrid_kernels.hpp SegSlab): zero between sorts, but for the
                                       // barrier counter its first kernel clears (kIdleTable)
    // profiling
    std::vector<adlhip_internal::PendingProf> pending;
    std::vector<hipEvent_t> event_pool;
    std::map<std::string, adlhip_internal::ProfEntry> prof;
    std::vector<std::string> prof_order;
    // map/unmap staging; released staging blocks are pooled: pinning memory costs ~1 ms per 4 MiB, and the
    // reference's test maps every buffer two or three times (UnitTest/main.cpp:118-139)
    std::vector<adlhip_internal::Staging> staging;
    std::vector<adlhip_internal::PinnedBlock> pinned_pool;
    size_t pinned_pool_bytes = 0;
    // device-side fault words ([0] live, [1] sticky: onesweep_kernels.hpp raise_fault), checked at sync and by
    // adlhip_fault_check; [8] is the self-test's result slot
    uint32_t* d_fault = nullptr;
    uint32_t* h_fault = nullptr;   // pinned: [0..1] filled by adlhip_sync, [4] by the last adlhip_fault_check snapshot
    hipEvent_t fault_snap = nullptr;   // recorded behind the last snapshot copy; null = none pending
};

// the calling thread's error text (handle.hip; not in include/adlhip.h: sharded.cpp sets it too).  typed_keys_sort saves the text
// with adlhip_last_error and puts it back with this
extern "C" void adlhip_set_last_error(const char* text);

// a 16-byte value of the SoA and typed pair sorts.  In an unnamed namespace although both units use it: it is a template argument of
// their gather kernels, and so part of those kernels' names
namespace {
struct V16 {
    uint32_t x, y, z, w;
} __attribute__((aligned(16)));
}  // namespace

namespace adlhip_internal {
// ---- defined in handle.hip --------------------------------------------------------------------------------------------------------
int fail(const char* fmt, ...);             // sets the error text; returns ADLHIP_FAILURE
int bind(adlhip_device* d);
hipEvent_t take_event(adlhip_device* d);
int trace_level();                          // ADLHIP_TRACE
const char* intern(const std::string& s);   // kernel names (the profiler keeps the pointer until the events are folded)

// ---- defined in adlhip.hip --------------------------------------------------------------------------------------------------------
// What a handle owns for the sorts: d_mid_hist, d_msd2, d_dict, and what the device answers at creation (lds_ordered / rank_mode,
// resident_wgs).  create sets the error text and leaves what it has allocated to destroy, which frees whatever exists and calls
// neither fail nor HIPCHK (it is part of the handle's one teardown)
#pragma GCC visibility push(hidden)   // called between the library's own units only: kept out of its dynamic symbol table
int sort_state_create(adlhip_device* d);
void sort_state_destroy(adlhip_device* d);
int num_tile_variants();   // "sort.tile" accepts -1 .. num_tile_variants() - 1
// the knobs that are no field of the handle but words of the sorts' device state: "debug.idle_poke" (set), "stat.net_runs",
// "stat.net_counting", "debug.idle_dirty", "debug.idle_first", "debug.net_stamp0".."9" (get).  kNoSuchParam for any other name
constexpr int kNoSuchParam = -1;
int sort_set_param(adlhip_device* d, const char* name, int value);
int sort_get_param(adlhip_device* d, const char* name, int* value);
#pragma GCC visibility pop

struct SoaWideLayout {
    size_t off_pairs_a, off_pairs_b, off_kv, kv_bytes, total;
};
SoaWideLayout soa_wide_layout(const adlhip_device* d, size_t n);
int soa_check_widths(int key_bytes, int value_bytes);
size_t sort_work_bytes(const adlhip_device* d, int elem_kind, size_t n, int sort_bits, int level);
// the sort of adlhip_radix_sort_u32 / _u64 / _kv32 by element kind (ADLHIP_ELEM_U32, ADLHIP_ELEM_U64, ADLHIP_ELEM_KV32)
int sort_elements(adlhip_device* d, int elem_kind, void* data, void* tmp, void* work, size_t work_bytes, size_t n, int sort_bits);
// scan_single_kernel (radix_kernels.hpp) under the profile name `name`: dst = exclusive scan of src[0..n), the total to *d_total
int launch_scan_single(adlhip_device* d, const char* name, const uint32_t* src, uint32_t* dst, size_t n, uint32_t* d_total);

constexpr size_t kMaxElems = 0xFFF00000ull;   // 32-bit element indices inside the kernels
// Grid of the kernels that walk up to kMaxElems elements as `for (uint32_t i = ...; i < n; i += stride)` with stride = grid x 256 threads
// (typed_kernels.hpp, soa_wide_kernels.hpp, select_gather_kernel): the last i below n is followed by i + stride < n + stride, which must
// not pass 2^32, or the index wraps and the loop never ends.  So stride <= 2^32 - kMaxElems = 2^20: at most 4096 workgroups, which is
// what 16 workgroups per CU come to on 256 CUs; a device with more CUs is held to the same grid.
constexpr size_t kStride32MaxWgs = ((size_t(1) << 32) - kMaxElems) / 256;
inline size_t stride32_wgs(const hipDeviceProp_t& prop, size_t n)
{
    return std::min(std::min((n + 255) / 256, (size_t)prop.multiProcessorCount * 16), kStride32MaxWgs);
}
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return adlhip_internal::fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// Launch wrapper: optional hipEvent bracket per launch ("profile" = 1), error check after.
template <typename F>
int launch(adlhip_device* d, const char* name, F&& f)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (d->profile) {
        e0 = take_event(d);
        e1 = take_event(d);
        if (!e0 || !e1) return fail("hipEventCreate failed");
        HIPCHK(hipEventRecord(e0, d->stream));
    }
    // ADLHIP_TRACE=1 (debugging aid): name every launch on stderr and wait for it, so that the last line before a GPU fault
    // names the kernel that raised it
    // (ADLHIP_TRACE=2: names only, nothing waits)
    static const int trace = trace_level();
    if (trace) fprintf(stderr, "[adlhip] launch %s\n", name), fflush(stderr);
    f();
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("launch of %s failed: %s", name, hipGetErrorString(e));
    if (trace == 1 && (e = hipStreamSynchronize(d->stream)) != hipSuccess) return fail("%s: %s", name, hipGetErrorString(e));
    if (d->profile) {
        HIPCHK(hipEventRecord(e1, d->stream));
        d->pending.push_back({name, e0, e1});
    }
    return ADLHIP_SUCCESS;
}

}  // namespace adlhip_internal
