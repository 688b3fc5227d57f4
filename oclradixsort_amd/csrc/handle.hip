// handle.hip -- the runtime under the sorts: error text, the device handle (create, the one teardown, info, sync, fault words), buffers,
// copies, map / unmap with its pinned pool, events, the per-launch profiler, the probes, the key generator and the knobs.  Replaces
// Adl/CL/AdlCL.inl (device, buffers, copies, map/unmap) and Adl/CL/AdlKernelUtilsCL.inl (per-launch profiling).  It sees no sort header:
// what a handle owns for the sorts is behind sort_state_create / sort_state_destroy and sort_set_param / sort_get_param (adlhip.hip).
#include "adlhip_internal.hpp"

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "util_kernels.hpp"

using namespace adlhip_internal;

namespace {
thread_local char g_err[512] = "";
constexpr size_t kPinnedPoolMax = size_t(512) << 20;   // pinned staging kept for re-use per device handle
}  // namespace

namespace adlhip_internal {

int fail(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    if (getenv("ADLHIP_VERBOSE")) fprintf(stderr, "[adlhip] error: %s\n", g_err);
    return ADLHIP_FAILURE;
}

int bind(adlhip_device* d)
{
    if (!d) return fail("null device handle");
    HIPCHK(hipSetDevice(d->idx));
    return ADLHIP_SUCCESS;
}

hipEvent_t take_event(adlhip_device* d)
{
    if (!d->event_pool.empty()) {
        hipEvent_t e = d->event_pool.back();
        d->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

int trace_level()
{
    static const int level = getenv("ADLHIP_TRACE") ? atoi(getenv("ADLHIP_TRACE")) : 0;
    return level;
}

// Interned kernel names (the profiler keeps the pointer until the events are folded).
const char* intern(const std::string& s)
{
    static std::mutex mu;
    static std::map<std::string, std::string*> pool;
    std::lock_guard<std::mutex> lock(mu);
    auto it = pool.find(s);
    if (it == pool.end()) it = pool.emplace(s, new std::string(s)).first;
    return it->second->c_str();
}

}  // namespace adlhip_internal

namespace {

int fold_profile(adlhip_device* d)
{
    if (d->pending.empty()) return ADLHIP_SUCCESS;
    HIPCHK(hipStreamSynchronize(d->stream));
    for (auto& p : d->pending) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, p.e0, p.e1));
        auto it = d->prof.find(p.name);
        if (it == d->prof.end()) {
            d->prof_order.push_back(p.name);
            it = d->prof.emplace(p.name, ProfEntry()).first;
        }
        it->second.launches++;
        it->second.total_ms += ms;
        d->event_pool.push_back(p.e0);
        d->event_pool.push_back(p.e1);
    }
    d->pending.clear();
    return ADLHIP_SUCCESS;
}

void reap_staging(adlhip_device* d, bool all_done)
{
    for (size_t i = 0; i < d->staging.size();) {
        Staging& s = d->staging[i];
        if (s.done && (all_done || hipEventQuery(s.done) == hipSuccess)) {
            hipEventDestroy(s.done);
            if (d->pinned_pool_bytes + s.capacity <= kPinnedPoolMax) {
                d->pinned_pool.push_back({s.hptr, s.capacity});
                d->pinned_pool_bytes += s.capacity;
            } else {
                hipHostFree(s.hptr);
            }
            d->staging[i] = d->staging.back();
            d->staging.pop_back();
        } else {
            ++i;
        }
    }
}

// The one teardown: releases whatever of a handle exists and deletes it.  The end of adlhip_device_destroy and of every failure exit
// of create_common, so a new handle-owned resource is released here and nowhere else.  Calls neither fail nor HIPCHK: the message of
// the failure that led here survives.
void release_handle(adlhip_device* d)
{
    reap_staging(d, true);
    for (auto& s : d->staging) hipHostFree(s.hptr);
    for (auto& b : d->pinned_pool) hipHostFree(b.hptr);
    for (auto& p : d->pending) { hipEventDestroy(p.e0); hipEventDestroy(p.e1); }
    for (auto e : d->event_pool) hipEventDestroy(e);
    if (d->fault_snap) hipEventDestroy(d->fault_snap);
    sort_state_destroy(d);
    if (d->d_fault) hipFree(d->d_fault);
    if (d->h_fault) hipHostFree(d->h_fault);
    if (d->own_stream && d->stream) hipStreamDestroy(d->stream);
    delete d;
}

int create_common(int device_idx, void* stream, bool own, adlhip_device** out)
{
    if (!out) return fail("null out pointer");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail("no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device_idx < 0) device_idx = 0;
    if (device_idx >= n) device_idx = n - 1;   // AdlCL.inl:244 clamps the same way
    adlhip_device* d = new adlhip_device();
    d->idx = device_idx;
    d->own_stream = own;
    auto give_up = [d](int rc) { return release_handle(d), rc; };   // every failure exit: its message, then the one teardown
    if (hipSetDevice(device_idx) != hipSuccess || hipGetDeviceProperties(&d->prop, device_idx) != hipSuccess)
        return give_up(fail("cannot bind HIP device %d", device_idx));
    if (strncmp(d->prop.gcnArchName, "gfx950", 6) != 0 && !getenv("ADLHIP_ALLOW_ANY_ARCH"))
        return give_up(fail("adlhip is built for gfx950 only; device %d is %s", device_idx, d->prop.gcnArchName));
    if (own) {
        if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) return give_up(fail("hipStreamCreate failed"));
    } else {
        d->stream = reinterpret_cast<hipStream_t>(stream);
    }
    if (hipMalloc(&d->d_fault, 64) != hipSuccess || hipHostMalloc(&d->h_fault, 64) != hipSuccess ||
        hipMemsetAsync(d->d_fault, 0, 64, d->stream) != hipSuccess)
        return give_up(fail("cannot allocate the fault word"));
    memset(d->h_fault, 0, 64);
    if (sort_state_create(d)) return give_up(ADLHIP_FAILURE);   // (the message is sort_state_create's)
    if (const char* a = getenv("ADLHIP_SORT_ALGO")) { int v = atoi(a); if (v >= -1 && v <= 1) d->sort_algo = v; }
    if (const char* t = getenv("ADLHIP_SORT_TILE")) { int v = atoi(t); if (v >= -1 && v < num_tile_variants()) d->tile_variant = v; }
    if (const char* r = getenv("ADLHIP_SORT_RANK")) d->rank_mode = (atoi(r) && d->lds_ordered) ? 1 : 0;
    if (const char* m = getenv("ADLHIP_SORT_MID")) d->mid_path = atoi(m) ? 1 : 0;
    if (const char* m = getenv("ADLHIP_SORT_MSD2")) { int v = atoi(m); if (v >= 0 && v <= 2) d->msd2_path = v; }
    if (const char* b = getenv("ADLHIP_DIGIT_BITS")) { int v = atoi(b); d->digit_bits = v == 4 ? 4 : 8; }
    *out = d;
    return ADLHIP_SUCCESS;
}

int report_fault(adlhip_device* d, uint32_t code)
{
    hipMemsetAsync(d->d_fault, 0, 8, d->stream);
    if (code & 0x40000u)
        return fail("device-side fault 0x%x (a segment exceeded the LDS tile of the finishing pass); results are invalid", code);
    return fail("device-side fault 0x%x (look-back wait exceeded its bound); results are invalid", code);
}

// ---- knobs ------------------------------------------------------------------------------------
// One row per knob that is a field of the handle; adlhip_set_param and adlhip_get_param walk the same rows.  A set checks the range,
// if the row has a refusal text for it, then asks the row's rule, if it has one, which refuses the value in words of its own or
// normalises it in place; what is left is stored in the field, which a get reads back.  (The knobs that are no field:
// sort_set_param / sort_get_param, adlhip.hip.)
struct Knob {
    const char* name;
    int adlhip_device::*field;
    int lo, hi;            // the accepted range, ...
    const char* refusal;   // ... and what a value outside it is told (null: no range)
    int (*rule)(adlhip_device* d, int* value);
};
constexpr int kNoMax = INT_MAX;
int as_flag(adlhip_device*, int* v) { *v = *v ? 1 : 0; return ADLHIP_SUCCESS; }
static_assert(kHistogramLdsBinsMax == 8192, "the refusal text of debug.histogram_lds_bins");
static_assert(kSearchLdsKeysMax == 4096, "the refusal text of debug.search_lds_keys");
const Knob kKnobs[] = {
    {"sort.algo", &adlhip_device::sort_algo, -1, 1, "sort.algo must be -1, 0 or 1", nullptr},
    {"sort.mid", &adlhip_device::mid_path, 0, 3,
     "sort.mid must be 0 (off), 1 (on), 2 (keys: always the two-launch form) or 3 (always the three-launch form)", nullptr},
    {"sort.msd2", &adlhip_device::msd2_path, 0, 5,
     "sort.msd2 must be 0 (off), 1 (on), 2 (always, from 1 Mi elements; forms by size), 3 (always the stable passes), "
     "4 (always the cursor passes for whole keys) or 5 (always the hybrid form for whole keys)", nullptr},
    {"sort.persist", &adlhip_device::persist, 0, 1,
     "sort.persist must be 0 (one tile per workgroup, round 3) or 1 (persistent prefetching passes + 16-bit finish)", nullptr},
    {"sort.dict", &adlhip_device::dict_path, 0, 1,
     "sort.dict must be 0 (off) or 1 (counting sort for keys that take few distinct values)", nullptr},
    {"sort.binfinish", &adlhip_device::bin_finish, 0, 2,
     "sort.binfinish must be 0 (LSD finish), 1 (binning finish for whole u64 keys from 24 Mi keys up) or 2 (always, u32 keys too)", nullptr},
    {"topk.algo", &adlhip_device::topk_algo, -1, 1,
     "topk.algo must be -1 (by k), 0 (always the full argsort) or 1 (always the selection)", nullptr},
    {"topk.rows_algo", &adlhip_device::topk_rows_algo, -1, 1,
     "topk.rows_algo must be -1 (by k and cols), 0 (always the per-row loop) or 1 (always the row kernel)", nullptr},
    {"debug.topk_rows_grid", &adlhip_device::topk_rows_grid, 0, kNoMax, "debug.topk_rows_grid must be >= 0", nullptr},
    {"sort.rows_algo", &adlhip_device::sort_rows_algo, -1, 1,
     "sort.rows_algo must be -1 (by cols), 0 (always the flat path) or 1 (always the row kernel)", nullptr},
    {"debug.sort_rows_grid", &adlhip_device::sort_rows_grid, 0, kNoMax, "debug.sort_rows_grid must be >= 0", nullptr},
    {"sort.segments_algo", &adlhip_device::sort_segments_algo, -1, 1,
     "sort.segments_algo must be -1 (by max_segment), 0 (always the flat path) or 1 (always the segment kernel)", nullptr},
    {"debug.sort_segments_grid", &adlhip_device::sort_segments_grid, 0, kNoMax, "debug.sort_segments_grid must be >= 0", nullptr},
    {"debug.unique_grid", &adlhip_device::unique_grid, 0, kNoMax, "debug.unique_grid must be >= 0", nullptr},
    {"debug.reduce_grid", &adlhip_device::reduce_grid, 0, kNoMax, "debug.reduce_grid must be >= 0", nullptr},
    {"debug.scan_grid", &adlhip_device::scan_grid, 0, kNoMax, "debug.scan_grid must be >= 0", nullptr},
    {"debug.compact_grid", &adlhip_device::compact_grid, 0, kNoMax, "debug.compact_grid must be >= 0", nullptr},
    {"debug.histogram_grid", &adlhip_device::histogram_grid, 0, kNoMax, "debug.histogram_grid must be >= 0", nullptr},
    {"debug.merge_grid", &adlhip_device::merge_grid, 0, kNoMax, "debug.merge_grid must be >= 0", nullptr},
    {"debug.setop_grid", &adlhip_device::setop_grid, 0, kNoMax, "debug.setop_grid must be >= 0", nullptr},
    {"debug.search_grid", &adlhip_device::search_grid, 0, kNoMax, "debug.search_grid must be >= 0", nullptr},
    {"debug.join_grid", &adlhip_device::join_grid, 0, kNoMax, "debug.join_grid must be >= 0", nullptr},
    {"debug.persist_grid", &adlhip_device::persist_grid, 0, 4096, "debug.persist_grid must be in [0, 4096]", nullptr},
    // ---- with a rule of their own
    {"sort.digit_bits", &adlhip_device::digit_bits, 0, 0, nullptr,
     [](adlhip_device*, int* v) { return *v == 4 || *v == 8 ? ADLHIP_SUCCESS : fail("sort.digit_bits must be 4 or 8"); }},
    {"unique.algo", &adlhip_device::unique_algo, 0, 0, nullptr, [](adlhip_device*, int* v) {
         return *v == -1 || *v == 1 ? ADLHIP_SUCCESS : fail("unique.algo must be -1 (by the outputs asked) or 1 (always the index path)"); }},
    {"sort.tile", &adlhip_device::tile_variant, 0, 0, nullptr, [](adlhip_device*, int* v) {
         return *v >= -1 && *v < num_tile_variants() ? ADLHIP_SUCCESS : fail("sort.tile must be in [-1,%d)", num_tile_variants()); }},
    {"sort.net_lookback", &adlhip_device::net_lookback, 0, 0, nullptr, as_flag},
    {"partition.lookback", &adlhip_device::partition_lookback, 0, 0, nullptr, as_flag},
    {"profile", &adlhip_device::profile, 0, 0, nullptr, [](adlhip_device* d, int* v) {   // turning it off folds the pending events
         return bind(d) || (!*v && fold_profile(d)) ? ADLHIP_FAILURE : as_flag(d, v); }},
    {"debug.histogram_lds_bins", &adlhip_device::histogram_lds_bins, 0, kHistogramLdsBinsMax,
     "debug.histogram_lds_bins must be in [1, 8192], or 0 for the default",
     [](adlhip_device*, int* v) { if (!*v) *v = kHistogramLdsBinsMax; return ADLHIP_SUCCESS; }},
    {"debug.search_lds_keys", &adlhip_device::search_lds_keys, 0, kSearchLdsKeysMax,
     "debug.search_lds_keys must be in [2, 4096], or 0 for the default", [](adlhip_device*, int* v) {
         if (*v == 1) return fail("debug.search_lds_keys must be in [2, 4096], or 0 for the default");
         if (!*v) *v = kSearchLdsKeysMax;
         return ADLHIP_SUCCESS; }},
    // (what the paths with a grid-wide barrier may count on; 0 = the device's own answer again.  Tests stand in for a small partition with it)
    {"debug.resident_wgs", &adlhip_device::resident_wgs, 0, kNoMax, "debug.resident_wgs must be >= 0",
     [](adlhip_device* d, int* v) { if (!*v) *v = d->resident_wgs_device; return ADLHIP_SUCCESS; }},
    {"sort.rank", &adlhip_device::rank_mode, 0, 1, "sort.rank must be 0 or 1", [](adlhip_device* d, int* v) {
         return *v && !d->lds_ordered ? fail("sort.rank = 1 needs lane-ordered DS atomics; the device self-test failed") : ADLHIP_SUCCESS; }},
    {"sort.lds_ordered", &adlhip_device::lds_ordered, 0, 0, nullptr,   // the self-test's result: read only
     [](adlhip_device*, int*) { return fail("unknown parameter '%s'", "sort.lds_ordered"); }},
};

}  // namespace

// ================================================================================================
extern "C" {

const char* adlhip_version(void) { return "adlhip 0.2 (gfx950)"; }
const char* adlhip_last_error(void) { return g_err; }
// internal (not in include/adlhip.h): lets the library's other translation unit (sharded.cpp) set the calling thread's
// error text
void adlhip_set_last_error(const char* text) { snprintf(g_err, sizeof(g_err), "%s", text ? text : ""); }

int adlhip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int adlhip_device_create(int device_idx, adlhip_device** out) { return create_common(device_idx, nullptr, true, out); }

int adlhip_device_create_on_stream(int device_idx, void* hip_stream, adlhip_device** out)
{
    return create_common(device_idx, hip_stream, false, out);
}

int adlhip_device_destroy(adlhip_device* d)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (d->used_bytes != 0)   // Adl.inl:102 ADLASSERT( getUsedMemory() == 0 )
        return fail("device still has %llu live bytes; free every buffer first", (unsigned long long)d->used_bytes);
    hipStreamSynchronize(d->stream);
    release_handle(d);
    return ADLHIP_SUCCESS;
}

int adlhip_device_info(adlhip_device* d, adlhip_info* out)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!out) return fail("null info pointer");
    memset(out, 0, sizeof(*out));
    out->compute_units = d->prop.multiProcessorCount;
    out->wavefront_size = d->prop.warpSize;
    out->lds_bytes_per_cu = (int32_t)d->prop.maxSharedMemoryPerMultiProcessor;
    out->clock_khz = d->prop.clockRate;
    out->total_mem_bytes = d->prop.totalGlobalMem;
    out->max_alloc_bytes = d->prop.totalGlobalMem;
    snprintf(out->name, sizeof(out->name), "%s", d->prop.name);
    snprintf(out->arch, sizeof(out->arch), "%s", d->prop.gcnArchName);
    snprintf(out->vendor, sizeof(out->vendor), "Advanced Micro Devices, Inc.");
    return ADLHIP_SUCCESS;
}

uint64_t adlhip_used_bytes(adlhip_device* d) { return d ? d->used_bytes : 0; }

void* adlhip_stream(adlhip_device* d) { return d ? (void*)d->stream : nullptr; }

int adlhip_sync(adlhip_device* d)
{
    if (bind(d)) return ADLHIP_FAILURE;
    // pick up the device-side fault words together with the drain
    HIPCHK(hipMemcpyAsync(d->h_fault, d->d_fault, 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    reap_staging(d, true);
    uint32_t code = d->h_fault[1];
    if (d->fault_snap) {   // a snapshot taken before this drain has landed too
        code |= d->h_fault[4];
        d->h_fault[4] = 0;
        hipEventDestroy(d->fault_snap);
        d->fault_snap = nullptr;
    }
    if (code != 0) {
        d->h_fault[0] = d->h_fault[1] = 0;
        return report_fault(d, code);
    }
    return ADLHIP_SUCCESS;
}

int adlhip_fault_check(adlhip_device* d)
{
    if (bind(d)) return ADLHIP_FAILURE;
    uint32_t code = 0;
    if (d->fault_snap) {
        if (hipEventQuery(d->fault_snap) != hipSuccess) return ADLHIP_SUCCESS;   // the last snapshot is still in flight
        code = d->h_fault[4];
        d->h_fault[4] = 0;
    } else {
        HIPCHK(hipEventCreateWithFlags(&d->fault_snap, hipEventDisableTiming));
    }
    if (code != 0) report_fault(d, code);   // clears the device words BEFORE the next snapshot is taken: reported once
    HIPCHK(hipMemcpyAsync(d->h_fault + 4, d->d_fault + 1, 4, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipEventRecord(d->fault_snap, d->stream));
    return code != 0 ? ADLHIP_FAILURE : ADLHIP_SUCCESS;
}

int adlhip_flush(adlhip_device* d) { return bind(d); }

int adlhip_malloc(adlhip_device* d, size_t bytes, void** dptr)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!dptr) return fail("null out pointer");
    *dptr = nullptr;
    if (bytes == 0) return ADLHIP_SUCCESS;
    hipError_t e = hipMalloc(dptr, bytes);
    if (e != hipSuccess) {   // AdlCL.inl:390-406: log, leave m_ptr = 0
        *dptr = nullptr;
        return fail("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    d->used_bytes += bytes;
    if (trace_level()) fprintf(stderr, "[adlhip] malloc %p + %zu\n", *dptr, bytes);
    return ADLHIP_SUCCESS;
}

int adlhip_free(adlhip_device* d, void* dptr, size_t bytes)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!dptr) return ADLHIP_SUCCESS;
    if (trace_level()) fprintf(stderr, "[adlhip] free %p + %zu\n", dptr, bytes);
    HIPCHK(hipStreamSynchronize(d->stream));   // queued work may still use it
    HIPCHK(hipFree(dptr));
    d->used_bytes -= std::min<uint64_t>(bytes, d->used_bytes);
    return ADLHIP_SUCCESS;
}

int adlhip_memcpy_h2d(adlhip_device* d, void* dst, const void* src, size_t bytes)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (bytes == 0) return ADLHIP_SUCCESS;
    if (trace_level()) fprintf(stderr, "[adlhip] h2d %p <- %p + %zu\n", dst, src, bytes);
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, d->stream));
    return ADLHIP_SUCCESS;
}

int adlhip_memcpy_d2h(adlhip_device* d, void* dst, const void* src, size_t bytes)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (bytes == 0) return ADLHIP_SUCCESS;
    if (trace_level()) fprintf(stderr, "[adlhip] d2h %p <- %p + %zu\n", dst, src, bytes);
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, d->stream));
    return ADLHIP_SUCCESS;
}

int adlhip_memcpy_d2d(adlhip_device* d, void* dst, const void* src, size_t bytes)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (bytes == 0) return ADLHIP_SUCCESS;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, d->stream));
    return ADLHIP_SUCCESS;
}

int adlhip_memset(adlhip_device* d, void* dptr, int byte_value, size_t bytes)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (bytes == 0) return ADLHIP_SUCCESS;
    HIPCHK(hipMemsetAsync(dptr, byte_value, bytes, d->stream));
    return ADLHIP_SUCCESS;
}

int adlhip_fill_u32(adlhip_device* d, void* dptr, uint32_t pattern, size_t count)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (count == 0) return ADLHIP_SUCCESS;
    const int grid = (int)std::min<size_t>((count + 255) / 256, (size_t)d->prop.multiProcessorCount * 8);
    return launch(d, "fill_u32", [&] {
        hipLaunchKernelGGL(adlhip::fill_u32_kernel, dim3(grid), dim3(256), 0, d->stream, (uint32_t*)dptr, pattern, count);
    });
}

int adlhip_fill_pattern(adlhip_device* d, void* dptr, const void* pattern, size_t pattern_bytes, size_t count)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (pattern_bytes != 4 && pattern_bytes != 8 && pattern_bytes != 16) return fail("fill: pattern of %zu bytes (4, 8 or 16)", pattern_bytes);
    if (count == 0) return ADLHIP_SUCCESS;
    if (!dptr || !pattern) return fail("fill: null pointer");
    if (reinterpret_cast<uintptr_t>(dptr) % pattern_bytes) return fail("fill: destination not aligned to the pattern size");
    if (pattern_bytes == 4) {
        uint32_t v;
        memcpy(&v, pattern, 4);
        return adlhip_fill_u32(d, dptr, v, count);
    }
    uint4 p16;
    uint2 p8 = make_uint2(0u, 0u);
    uint2* tail = nullptr;
    uint4* dst = reinterpret_cast<uint4*>(dptr);
    size_t vecs = count;
    if (pattern_bytes == 16) {
        memcpy(&p16, pattern, 16);
    } else {
        memcpy(&p8, pattern, 8);
        p16 = make_uint4(p8.x, p8.y, p8.x, p8.y);
        uint2* d8 = reinterpret_cast<uint2*>(dptr);
        size_t c = count;
        if (reinterpret_cast<uintptr_t>(dptr) & 8u) {   // leading odd element: written through the tail slot of a first launch
            int rc = launch(d, "fill_pattern", [&] {
                hipLaunchKernelGGL(adlhip::fill_pattern16_kernel, dim3(1), dim3(256), 0, d->stream, (uint4*)nullptr, p16, (size_t)0, d8, p8);
            });
            if (rc) return rc;
            ++d8;
            if (--c == 0) return ADLHIP_SUCCESS;
        }
        dst = reinterpret_cast<uint4*>(d8);
        vecs = c / 2;
        if (c & 1) tail = d8 + (c - 1);
    }
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((vecs + 255) / 256, (size_t)d->prop.multiProcessorCount * 8));
    return launch(d, "fill_pattern", [&] {
        hipLaunchKernelGGL(adlhip::fill_pattern16_kernel, dim3(grid), dim3(256), 0, d->stream, dst, p16, vecs, tail, p8);
    });
}

int adlhip_map(adlhip_device* d, void* dptr, size_t bytes, void** hptr)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!hptr) return fail("null out pointer");
    *hptr = nullptr;
    reap_staging(d, false);
    if (bytes == 0) return ADLHIP_SUCCESS;
    void* h = nullptr;
    size_t cap = bytes;
    for (size_t i = 0; i < d->pinned_pool.size(); ++i) {   // smallest pooled block that fits without wasting more than half
        const PinnedBlock b = d->pinned_pool[i];
        if (b.capacity >= bytes && b.capacity <= 2 * bytes + 4096 && (!h || b.capacity < cap)) {
            h = b.hptr;
            cap = b.capacity;
        }
    }
    if (h) {
        for (size_t i = 0; i < d->pinned_pool.size(); ++i)
            if (d->pinned_pool[i].hptr == h) {
                d->pinned_pool[i] = d->pinned_pool.back();
                d->pinned_pool.pop_back();
                break;
            }
        d->pinned_pool_bytes -= cap;
    } else {
        HIPCHK(hipHostMalloc(&h, bytes));
    }
    hipError_t e = hipMemcpyAsync(h, dptr, bytes, hipMemcpyDeviceToHost, d->stream);
    if (e != hipSuccess) {
        hipHostFree(h);
        return fail("map: device->host copy failed: %s", hipGetErrorString(e));
    }
    d->staging.push_back({h, bytes, nullptr, cap});
    *hptr = h;
    return ADLHIP_SUCCESS;
}

int adlhip_unmap(adlhip_device* d, void* dptr, void* hptr, size_t bytes)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!hptr) return ADLHIP_SUCCESS;
    for (auto& s : d->staging) {
        if (s.hptr == hptr && !s.done) {
            if (bytes > s.bytes) return fail("unmap: %zu bytes exceeds the mapped %zu", bytes, s.bytes);
            if (bytes == 0) bytes = s.bytes;   // 0 = the whole mapping (Buffer::returnHostPtr carries no size)
            HIPCHK(hipMemcpyAsync(dptr, hptr, bytes, hipMemcpyHostToDevice, d->stream));
            hipEvent_t ev;
            HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            HIPCHK(hipEventRecord(ev, d->stream));
            s.done = ev;
            return ADLHIP_SUCCESS;
        }
    }
    return fail("unmap: pointer %p was not returned by adlhip_map", hptr);
}

// ---- synthetic inputs ---------------------------------------------------------------------------

int adlhip_generate_keys(adlhip_device* d, int elem_kind, void* dptr, size_t n, uint64_t seed, uint64_t first_index)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (elem_kind < ADLHIP_ELEM_U32 || elem_kind > ADLHIP_ELEM_U64) return fail("bad element kind %d", elem_kind);
    if (n == 0) return ADLHIP_SUCCESS;
    if (!dptr) return fail("null buffer");
    const uint64_t base = seed * 0x9E3779B97F4A7C15ull + first_index;
    const int grid = (int)std::min<size_t>((n + 255) / 256, (size_t)d->prop.multiProcessorCount * 16);
    return launch(d, "generate_keys", [&] {
        hipLaunchKernelGGL(adlhip::generate_keys_kernel, dim3(grid), dim3(256), 0, d->stream, dptr, n, base, first_index, elem_kind);
    });
}

// ---- knobs ------------------------------------------------------------------------------------

int adlhip_set_param(adlhip_device* d, const char* name, int value)
{
    if (!d || !name) return fail("null argument");
    for (const Knob& k : kKnobs) {
        if (strcmp(name, k.name)) continue;
        if (k.refusal && (value < k.lo || value > k.hi)) return fail("%s", k.refusal);
        if (k.rule && k.rule(d, &value)) return ADLHIP_FAILURE;   // (the text is the rule's)
        d->*k.field = value;
        return ADLHIP_SUCCESS;
    }
    const int rc = sort_set_param(d, name, value);
    return rc == kNoSuchParam ? fail("unknown parameter '%s'", name) : rc;
}

int adlhip_get_param(adlhip_device* d, const char* name, int* value)
{
    if (!d || !name || !value) return fail("null argument");
    for (const Knob& k : kKnobs) {
        if (strcmp(name, k.name)) continue;
        *value = d->*k.field;
        return ADLHIP_SUCCESS;
    }
    const int rc = sort_get_param(d, name, value);
    return rc == kNoSuchParam ? fail("unknown parameter '%s'", name) : rc;
}

// ---- events / profiling ---------------------------------------------------------------------------

int adlhip_event_create(adlhip_device* d, adlhip_event** out)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!out) return fail("null out pointer");
    adlhip_event* e = new adlhip_event();
    if (hipEventCreate(&e->ev) != hipSuccess) {
        delete e;
        return fail("hipEventCreate failed");
    }
    *out = e;
    return ADLHIP_SUCCESS;
}

int adlhip_event_record(adlhip_device* d, adlhip_event* ev)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!ev) return fail("null event");
    HIPCHK(hipEventRecord(ev->ev, d->stream));
    return ADLHIP_SUCCESS;
}

int adlhip_event_elapsed_ms(adlhip_device* d, adlhip_event* a, adlhip_event* b, float* ms)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!a || !b || !ms) return fail("null argument");
    HIPCHK(hipEventSynchronize(b->ev));
    HIPCHK(hipEventElapsedTime(ms, a->ev, b->ev));
    return ADLHIP_SUCCESS;
}

int adlhip_event_synchronize(adlhip_device* d, adlhip_event* ev)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!ev) return fail("null event");
    HIPCHK(hipEventSynchronize(ev->ev));   // (an event that was never recorded is complete)
    return ADLHIP_SUCCESS;
}

int adlhip_event_query(adlhip_device* d, adlhip_event* ev, int* done)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!ev || !done) return fail("null argument");
    const hipError_t e = hipEventQuery(ev->ev);
    if (e != hipSuccess && e != hipErrorNotReady) return fail("hipEventQuery failed: %s", hipGetErrorString(e));
    (void)hipGetLastError();   // hipErrorNotReady is an answer, not an error to leave behind
    *done = e == hipSuccess ? 1 : 0;
    return ADLHIP_SUCCESS;
}

int adlhip_event_destroy(adlhip_device* d, adlhip_event* ev)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!ev) return ADLHIP_SUCCESS;
    hipEventDestroy(ev->ev);
    delete ev;
    return ADLHIP_SUCCESS;
}

int adlhip_profile_reset(adlhip_device* d)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (fold_profile(d)) return ADLHIP_FAILURE;
    d->prof.clear();
    d->prof_order.clear();
    return ADLHIP_SUCCESS;
}

int adlhip_profile_count(adlhip_device* d)
{
    if (bind(d)) return -1;
    if (fold_profile(d)) return -1;
    return (int)d->prof_order.size();
}

int adlhip_profile_get(adlhip_device* d, int i, char name_out[64], uint64_t* launches, double* total_ms)
{
    if (!d) return fail("null device handle");
    if (i < 0 || i >= (int)d->prof_order.size()) return fail("profile index %d out of range", i);
    const std::string& nm = d->prof_order[i];
    const ProfEntry& e = d->prof[nm];
    if (name_out) snprintf(name_out, 64, "%s", nm.c_str());
    if (launches) *launches = e.launches;
    if (total_ms) *total_ms = e.total_ms;
    return ADLHIP_SUCCESS;
}

int adlhip_profile_write_csv(adlhip_device* d, const char* path)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!path) return fail("null path");
    if (fold_profile(d)) return ADLHIP_FAILURE;
    FILE* probe = fopen(path, "r");
    const bool fresh = probe == nullptr;
    if (probe) fclose(probe);
    FILE* f = fopen(path, "a");
    if (!f) return fail("cannot open %s for appending", path);
    if (fresh) fprintf(f, "\"kernel\",\"launches\",\"total_ms\",\"avg_ms\"\n");
    for (const std::string& nm : d->prof_order) {
        const ProfEntry& e = d->prof[nm];
        fprintf(f, "\"%s\",%llu,%.6f,%.6f\n", nm.c_str(), (unsigned long long)e.launches, e.total_ms,
                e.launches ? e.total_ms / (double)e.launches : 0.0);
    }
    fclose(f);
    return ADLHIP_SUCCESS;
}

// ---- probes ---------------------------------------------------------------------------------------

int adlhip_probe_copy(adlhip_device* d, void* dst, const void* src, size_t bytes)
{
    if (bind(d)) return ADLHIP_FAILURE;
    const size_t nvec = bytes / 16;
    if (nvec == 0) return ADLHIP_SUCCESS;
    const int grid = (int)std::min<size_t>((nvec + 255) / 256, (size_t)d->prop.multiProcessorCount * 8);
    return launch(d, "probe_copy", [&] {
        hipLaunchKernelGGL(adlhip::probe_copy_kernel, dim3(grid), dim3(256), 0, d->stream, (uint4*)dst, (const uint4*)src, nvec);
    });
}

// hints: bit 0 = non-temporal loads, bit 1 = non-temporal stores; grid_per_cu workgroups of 256 threads per CU (0 = 8)
int adlhip_probe_copy_ex(adlhip_device* d, void* dst, const void* src, size_t bytes, int hints, int grid_per_cu)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (hints < 0 || hints > 3 || grid_per_cu < 0 || grid_per_cu > 64) return fail("bad probe variant");
    const size_t nvec = bytes / 16;
    if (nvec == 0) return ADLHIP_SUCCESS;
    const int grid = (int)std::min<size_t>((nvec + 255) / 256, (size_t)d->prop.multiProcessorCount * (grid_per_cu ? grid_per_cu : 8));
    return launch(d, "probe_copy", [&] {
        switch (hints) {
        case 0: hipLaunchKernelGGL((adlhip::probe_copy_hint_kernel<false, false>), dim3(grid), dim3(256), 0, d->stream, (uint4*)dst, (const uint4*)src, nvec); break;
        case 1: hipLaunchKernelGGL((adlhip::probe_copy_hint_kernel<true, false>), dim3(grid), dim3(256), 0, d->stream, (uint4*)dst, (const uint4*)src, nvec); break;
        case 2: hipLaunchKernelGGL((adlhip::probe_copy_hint_kernel<false, true>), dim3(grid), dim3(256), 0, d->stream, (uint4*)dst, (const uint4*)src, nvec); break;
        default: hipLaunchKernelGGL((adlhip::probe_copy_hint_kernel<true, true>), dim3(grid), dim3(256), 0, d->stream, (uint4*)dst, (const uint4*)src, nvec); break;
        }
    });
}

int adlhip_probe_read_ex(adlhip_device* d, const void* src, size_t bytes, void* sink8, int hints, int grid_per_cu)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (hints < 0 || hints > 1 || grid_per_cu < 0 || grid_per_cu > 64) return fail("bad probe variant");
    const size_t nvec = bytes / 16;
    if (nvec == 0) return ADLHIP_SUCCESS;
    const int grid = (int)std::min<size_t>((nvec + 255) / 256, (size_t)d->prop.multiProcessorCount * (grid_per_cu ? grid_per_cu : 8));
    return launch(d, "probe_read", [&] {
        if (hints) hipLaunchKernelGGL((adlhip::probe_read_hint_kernel<true>), dim3(grid), dim3(256), 0, d->stream, (const uint4*)src, nvec, (unsigned long long*)sink8);
        else hipLaunchKernelGGL((adlhip::probe_read_hint_kernel<false>), dim3(grid), dim3(256), 0, d->stream, (const uint4*)src, nvec, (unsigned long long*)sink8);
    });
}

int adlhip_probe_read(adlhip_device* d, const void* src, size_t bytes, void* sink8)
{
    if (bind(d)) return ADLHIP_FAILURE;
    const size_t nvec = bytes / 16;
    if (nvec == 0) return ADLHIP_SUCCESS;
    const int grid = (int)std::min<size_t>((nvec + 255) / 256, (size_t)d->prop.multiProcessorCount * 8);
    return launch(d, "probe_read", [&] {
        hipLaunchKernelGGL(adlhip::probe_read_kernel, dim3(grid), dim3(256), 0, d->stream, (const uint4*)src, nvec,
                           (unsigned long long*)sink8);
    });
}

}  // extern "C"
