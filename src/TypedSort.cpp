// Pprims::sortKeys / Pprims::argsort: signed, floating-point and descending keys (no reference counterpart; the reference sorts
// u32 bit patterns, ascending: Tahoe/ParallelPrimitives/Pprims.h:38-41).  A TYPE_CL (HIP) device runs adlhip_sort_keys_typed /
// adlhip_argsort_typed; a TYPE_HOST device sorts on the CPU with std::stable_sort on the same total order, as the reference's
// host branches do for u32 keys (Pprims.cpp:202-212, :306-316).  Pprims::topK: adlhip_topk_typed, or a partial sort on (ordinal,
// position) on the host.  Pprims::topKRows: adlhip_topk_rows_typed, or the same partial sort per row.  Pprims::sortRows /
// argsortRows: adlhip_sort_rows_typed, or the host argsort per row.  Pprims::sortSegments / argsortSegments:
// adlhip_sort_segments_typed, or the host argsort per segment.  Pprims::unique:
// adlhip_unique_typed (it waits for the count), or the runs of the host argsort.  Pprims::reduceByKey: adlhip_reduce_by_key_typed (it
// waits for the count), or a loop over the runs of the host argsort.  Pprims::scanTyped / scanByKey: adlhip_scan_typed /
// adlhip_scan_by_key, or a plain loop, left to right.  Pprims::compactFlagged / compactIf: adlhip_compact_flagged /
// adlhip_compact_if_typed (they wait for the count), or a plain loop.  Pprims::histogramRange / binCount:
// adlhip_histogram_range_typed / adlhip_bincount_typed, or a plain loop.  Pprims::mergeKeys / mergePairs: adlhip_merge_typed, or a
// plain two-pointer loop in which a tie takes the first input.  Pprims::searchSorted: adlhip_search_sorted_typed, or a binary search
// per needle.  Pprims::setOp: adlhip_set_op_typed (it waits for the count), or
// thrust's two-pointer loops.  Pprims::joinSorted / expandRuns: adlhip_join_sorted_typed / adlhip_expand_runs (they wait for the
// count), or a two-pointer loop / a loop over the runs.
#include <Tahoe/ParallelPrimitives/Pprims.h>

#include <algorithm>
#include <cstring>
#include <vector>

namespace Tahoe {

namespace {

template <typename T> struct KeyTraits;
template <> struct KeyTraits<u32>       { typedef u32 Bits; enum { TYPE = ADLHIP_KEY_U32, SIGNED = 0, FLOAT = 0 }; };
template <> struct KeyTraits<int>       { typedef u32 Bits; enum { TYPE = ADLHIP_KEY_I32, SIGNED = 1, FLOAT = 0 }; };
template <> struct KeyTraits<float>     { typedef u32 Bits; enum { TYPE = ADLHIP_KEY_F32, SIGNED = 0, FLOAT = 1 }; };
template <> struct KeyTraits<u64>       { typedef u64 Bits; enum { TYPE = ADLHIP_KEY_U64, SIGNED = 0, FLOAT = 0 }; };
template <> struct KeyTraits<long long> { typedef u64 Bits; enum { TYPE = ADLHIP_KEY_I64, SIGNED = 1, FLOAT = 0 }; };
template <> struct KeyTraits<double>    { typedef u64 Bits; enum { TYPE = ADLHIP_KEY_F64, SIGNED = 0, FLOAT = 1 }; };

// the key's rank among all bit patterns of its width: unsigned order of the result is the order of the typed keys (floats: IEEE-754
// totalOrder) -- the host's statement of the device codec (oclradixsort_amd/csrc/typed_kernels.hpp)
template <typename T>
inline typename KeyTraits<T>::Bits ordinal(const T& key, bool descending)
{
    typedef typename KeyTraits<T>::Bits B;
    const B sign = (B)1 << (8 * sizeof(B) - 1);
    B b;
    memcpy(&b, &key, sizeof(B));
    if (KeyTraits<T>::SIGNED) b ^= sign;
    if (KeyTraits<T>::FLOAT) b ^= (b & sign) ? (B)~(B)0 : sign;
    return descending ? (B)~b : b;
}

template <typename B>
struct Ranked {
    B ord;
    u32 idx;
    bool operator<(const Ranked& o) const { return ord < o.ord; }
};

// order[j] = position of the j-th element of the sorted order (stable)
template <typename T>
void hostArgsort(const T* keys, int n, bool descending, std::vector<Ranked<typename KeyTraits<T>::Bits> >& order)
{
    order.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        order[i].ord = ordinal(keys[i], descending);
        order[i].idx = (u32)i;
    }
    std::stable_sort(order.begin(), order.end());
}

inline bool onDevice(const adl::Device* device)
{
    return device && device->getType() == adl::TYPE_CL && device->getProcType() == adl::Device::Config::DEVICE_GPU && device->hip() != 0;
}

}  // namespace

template <typename T>
void Pprims::sortKeysTyped(const adl::Device* device, const adl::Buffer<T>& inout, int n, bool descending)
{
    ADLASSERT(n >= 0);
    if (n <= 0) return;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)n <= inout.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return;
        T* host = inout.getHostPtr(n);
        adl::DeviceUtils::waitForCompletion(device);
        std::vector<Ranked<typename KeyTraits<T>::Bits> > order;
        hostArgsort(host, n, descending, order);
        std::vector<T> sorted((size_t)n);
        for (int j = 0; j < n; ++j) sorted[j] = host[order[j].idx];
        memcpy(host, sorted.data(), sizeof(T) * (size_t)n);
        inout.returnHostPtr(host);
        adl::DeviceUtils::waitForCompletion(device);
        return;
    }
    size_t tk = 0, tv = 0, wb = 0;
    const int rcq = adlhip_sort_typed_scratch_bytes(device->hip(), KeyTraits<T>::TYPE, 0, 0, (size_t)n, &tk, &tv, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, tk, wb);
    const int rc = adlhip_sort_keys_typed(device->hip(), KeyTraits<T>::TYPE, descending ? ADLHIP_ORDER_DESCENDING : ADLHIP_ORDER_ASCENDING,
                                          inout.m_ptr, m_tmp->m_ptr, m_work->m_ptr, (size_t)m_work->getSize(), (size_t)n);
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::sortKeys: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
}

template <typename T>
void Pprims::argsortTyped(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<u32>& indexOut, int n, bool descending)
{
    ADLASSERT(n >= 0);
    if (n <= 0) return;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)n <= keys.getSize() && (adl::u64)n <= indexOut.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return;
        T* host = keys.getHostPtr(n);
        u32* out = indexOut.getHostPtr(n);
        adl::DeviceUtils::waitForCompletion(device);
        std::vector<Ranked<typename KeyTraits<T>::Bits> > order;
        hostArgsort(host, n, descending, order);
        for (int j = 0; j < n; ++j) out[j] = order[j].idx;
        keys.returnHostPtr(host);
        indexOut.returnHostPtr(out);
        adl::DeviceUtils::waitForCompletion(device);
        return;
    }
    size_t tk = 0, tv = 0, wb = 0;
    const int rcq = adlhip_sort_typed_scratch_bytes(device->hip(), KeyTraits<T>::TYPE, 2, 0, (size_t)n, &tk, &tv, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, tk, wb);
    const int rc = adlhip_argsort_typed(device->hip(), KeyTraits<T>::TYPE, descending ? ADLHIP_ORDER_DESCENDING : ADLHIP_ORDER_ASCENDING,
                                        keys.m_ptr, 0, indexOut.m_ptr, m_work->m_ptr, (size_t)m_work->getSize(), (size_t)n);
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::argsort: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
}

template <typename T>
void Pprims::topKTyped(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<T>& keysOut, adl::Buffer<u32>& indexOut, int n, int k,
                       bool descending)
{
    ADLASSERT(n >= 0 && k >= 0 && k <= n);
    if (n <= 0 || k <= 0 || k > n) return;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)n <= keys.getSize() && (adl::u64)k <= keysOut.getSize() && (adl::u64)k <= indexOut.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return;
        typedef Ranked<typename KeyTraits<T>::Bits> R;
        T* host = keys.getHostPtr(n);
        T* kout = keysOut.getHostPtr(k);
        u32* out = indexOut.getHostPtr(k);
        adl::DeviceUtils::waitForCompletion(device);
        std::vector<R> order((size_t)n);
        for (int i = 0; i < n; ++i) {
            order[i].ord = ordinal(host[i], descending);
            order[i].idx = (u32)i;
        }
        // all (ordinal, position) composites are distinct, so the partial sort needs no stability
        std::partial_sort(order.begin(), order.begin() + k, order.end(),
                          [](const R& a, const R& b) { return a.ord != b.ord ? a.ord < b.ord : a.idx < b.idx; });
        for (int j = 0; j < k; ++j) {
            out[j] = order[j].idx;
            kout[j] = host[order[j].idx];
        }
        keys.returnHostPtr(host);
        keysOut.returnHostPtr(kout);
        indexOut.returnHostPtr(out);
        adl::DeviceUtils::waitForCompletion(device);
        return;
    }
    size_t wb = 0;
    const int rcq = adlhip_topk_scratch_bytes(device->hip(), KeyTraits<T>::TYPE, (size_t)n, (size_t)k, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 0, wb);
    const int rc = adlhip_topk_typed(device->hip(), KeyTraits<T>::TYPE, descending ? ADLHIP_ORDER_DESCENDING : ADLHIP_ORDER_ASCENDING,
                                     keys.m_ptr, (size_t)n, (size_t)k, keysOut.m_ptr, (uint32_t*)indexOut.m_ptr, m_work->m_ptr,
                                     (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::topK: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
}

template <typename T>
void Pprims::topKRowsTyped(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<T>& keysOut, adl::Buffer<u32>& indexOut, int rows,
                           int cols, int k, bool descending, int rowStride)
{
    const int stride = rowStride ? rowStride : cols;
    ADLASSERT(rows >= 0 && cols >= 0 && k >= 0 && k <= cols && stride >= cols);
    if (rows <= 0 || k <= 0 || k > cols || stride < cols) return;
    ADLASSERT(device != 0);
    const adl::u64 inElems = (adl::u64)(rows - 1) * (adl::u64)stride + (adl::u64)cols, outElems = (adl::u64)rows * (adl::u64)k;
    ADLASSERT(inElems <= keys.getSize() && outElems <= keysOut.getSize() && outElems <= indexOut.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return;
        typedef Ranked<typename KeyTraits<T>::Bits> R;
        T* host = keys.getHostPtr(inElems);
        T* kout = keysOut.getHostPtr(outElems);
        u32* out = indexOut.getHostPtr(outElems);
        adl::DeviceUtils::waitForCompletion(device);
        std::vector<R> order((size_t)cols);
        for (int r = 0; r < rows; ++r) {
            const T* row = host + (size_t)r * (size_t)stride;
            for (int i = 0; i < cols; ++i) {
                order[i].ord = ordinal(row[i], descending);
                order[i].idx = (u32)i;
            }
            // all (ordinal, column) composites of a row are distinct, so the partial sort needs no stability
            std::partial_sort(order.begin(), order.begin() + k, order.end(),
                              [](const R& a, const R& b) { return a.ord != b.ord ? a.ord < b.ord : a.idx < b.idx; });
            for (int j = 0; j < k; ++j) {
                out[(size_t)r * k + j] = order[j].idx;
                kout[(size_t)r * k + j] = row[order[j].idx];
            }
        }
        keys.returnHostPtr(host);
        keysOut.returnHostPtr(kout);
        indexOut.returnHostPtr(out);
        adl::DeviceUtils::waitForCompletion(device);
        return;
    }
    size_t wb = 0;
    const int rcq = adlhip_topk_rows_scratch_bytes(device->hip(), KeyTraits<T>::TYPE, (size_t)rows, (size_t)cols, (size_t)k, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 0, wb);
    const int rc = adlhip_topk_rows_typed(device->hip(), KeyTraits<T>::TYPE, descending ? ADLHIP_ORDER_DESCENDING : ADLHIP_ORDER_ASCENDING,
                                          keys.m_ptr, (size_t)rows, (size_t)cols, (size_t)stride, (size_t)k, keysOut.m_ptr,
                                          (uint32_t*)indexOut.m_ptr, m_work->m_ptr, (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::topKRows: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
}

template <typename T>
void Pprims::sortRowsTyped(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<T>* keysOut, adl::Buffer<u32>& indexOut, int rows,
                           int cols, bool descending, int rowStride)
{
    const int stride = rowStride ? rowStride : cols;
    ADLASSERT(rows >= 0 && cols >= 0 && stride >= cols);
    if (rows <= 0 || cols <= 0 || stride < cols) return;
    ADLASSERT(device != 0);
    const adl::u64 inElems = (adl::u64)(rows - 1) * (adl::u64)stride + (adl::u64)cols, outElems = (adl::u64)rows * (adl::u64)cols;
    ADLASSERT(inElems <= keys.getSize() && (!keysOut || outElems <= keysOut->getSize()) && outElems <= indexOut.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return;
        T* host = keys.getHostPtr(inElems);
        T* kout = keysOut ? keysOut->getHostPtr(outElems) : 0;
        u32* out = indexOut.getHostPtr(outElems);
        adl::DeviceUtils::waitForCompletion(device);
        std::vector<Ranked<typename KeyTraits<T>::Bits> > order;
        for (int r = 0; r < rows; ++r) {
            const T* row = host + (size_t)r * (size_t)stride;
            hostArgsort(row, cols, descending, order);
            for (int j = 0; j < cols; ++j) {
                out[(size_t)r * cols + j] = order[j].idx;
                if (kout) kout[(size_t)r * cols + j] = row[order[j].idx];
            }
        }
        keys.returnHostPtr(host);
        if (keysOut) keysOut->returnHostPtr(kout);
        indexOut.returnHostPtr(out);
        adl::DeviceUtils::waitForCompletion(device);
        return;
    }
    size_t wb = 0;
    const int rcq = adlhip_sort_rows_scratch_bytes(device->hip(), KeyTraits<T>::TYPE, (size_t)rows, (size_t)cols, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 0, wb);
    const int rc = adlhip_sort_rows_typed(device->hip(), KeyTraits<T>::TYPE, descending ? ADLHIP_ORDER_DESCENDING : ADLHIP_ORDER_ASCENDING,
                                          keys.m_ptr, (size_t)rows, (size_t)cols, (size_t)stride, keysOut ? keysOut->m_ptr : 0,
                                          (uint32_t*)indexOut.m_ptr, m_work->m_ptr, (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::sortRows: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
}

template <typename K>
void Pprims::sortRows(const adl::Device* device, const adl::Buffer<K>& keys, adl::Buffer<K>& keysOut, adl::Buffer<u32>& indexOut, int rows, int cols,
                      bool descending, int rowStride)
{
    sortRowsTyped<K>(device, keys, &keysOut, indexOut, rows, cols, descending, rowStride);
}

template <typename K>
void Pprims::argsortRows(const adl::Device* device, const adl::Buffer<K>& keys, adl::Buffer<u32>& indexOut, int rows, int cols, bool descending,
                         int rowStride)
{
    sortRowsTyped<K>(device, keys, 0, indexOut, rows, cols, descending, rowStride);
}

#define TAHOE_SORT_ROWS(K)                                                                                                                       \
    template void Pprims::sortRows<K>(const adl::Device*, const adl::Buffer<K>&, adl::Buffer<K>&, adl::Buffer<u32>&, int, int, bool, int); \
    template void Pprims::argsortRows<K>(const adl::Device*, const adl::Buffer<K>&, adl::Buffer<u32>&, int, int, bool, int);
TAHOE_SORT_ROWS(int)
TAHOE_SORT_ROWS(float)
TAHOE_SORT_ROWS(long long)
TAHOE_SORT_ROWS(double)
TAHOE_SORT_ROWS(u32)
TAHOE_SORT_ROWS(u64)
#undef TAHOE_SORT_ROWS

template <typename T>
void Pprims::sortSegmentsTyped(const adl::Device* device, const adl::Buffer<T>& keys, const adl::Buffer<u32>& offsets, adl::Buffer<T>* keysOut,
                               adl::Buffer<u32>& indexOut, int n, int numSegments, int maxSegment, bool descending, bool globalIndex)
{
    ADLASSERT(n >= 0 && numSegments >= 0 && maxSegment >= 0);
    if (n <= 0 || numSegments <= 0 || maxSegment < 0) return;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)n <= keys.getSize() && (adl::u64)numSegments + 1 <= offsets.getSize() && (!keysOut || (adl::u64)n <= keysOut->getSize()) &&
              (adl::u64)n <= indexOut.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return;
        T* host = keys.getHostPtr(n);
        u32* off = offsets.getHostPtr(numSegments + 1);
        T* kout = keysOut ? keysOut->getHostPtr(n) : 0;
        u32* out = indexOut.getHostPtr(n);
        adl::DeviceUtils::waitForCompletion(device);
        std::vector<Ranked<typename KeyTraits<T>::Bits> > order;
        for (int s = 0; s < numSegments; ++s) {   // every offset clamped to [previous, n], as the device clamps it
            const u32 lo = off[s] < (u32)n ? off[s] : (u32)n;
            const u32 hi = off[s + 1] < lo ? lo : (off[s + 1] < (u32)n ? off[s + 1] : (u32)n);
            hostArgsort(host + lo, (int)(hi - lo), descending, order);
            for (u32 j = 0; j < hi - lo; ++j) {
                out[lo + j] = order[j].idx + (globalIndex ? lo : 0u);
                if (kout) kout[lo + j] = host[lo + order[j].idx];
            }
        }
        keys.returnHostPtr(host);
        offsets.returnHostPtr(off);
        if (keysOut) keysOut->returnHostPtr(kout);
        indexOut.returnHostPtr(out);
        adl::DeviceUtils::waitForCompletion(device);
        return;
    }
    size_t wb = 0;
    const int rcq = adlhip_sort_segments_scratch_bytes(device->hip(), KeyTraits<T>::TYPE, (size_t)n, (size_t)numSegments, (size_t)maxSegment, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 0, wb);
    const int rc = adlhip_sort_segments_typed(device->hip(), KeyTraits<T>::TYPE, descending ? ADLHIP_ORDER_DESCENDING : ADLHIP_ORDER_ASCENDING,
                                              keys.m_ptr, (size_t)n, (const uint32_t*)offsets.m_ptr, (size_t)numSegments, (size_t)maxSegment,
                                              globalIndex ? ADLHIP_SEGMENT_INDEX_GLOBAL : ADLHIP_SEGMENT_INDEX_LOCAL, keysOut ? keysOut->m_ptr : 0,
                                              (uint32_t*)indexOut.m_ptr, 0, m_work->m_ptr, (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::sortSegments: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
}

template <typename K>
void Pprims::sortSegments(const adl::Device* device, const adl::Buffer<K>& keys, const adl::Buffer<u32>& offsets, adl::Buffer<K>& keysOut,
                          adl::Buffer<u32>& indexOut, int n, int numSegments, int maxSegment, bool descending, bool globalIndex)
{
    sortSegmentsTyped<K>(device, keys, offsets, &keysOut, indexOut, n, numSegments, maxSegment, descending, globalIndex);
}

template <typename K>
void Pprims::argsortSegments(const adl::Device* device, const adl::Buffer<K>& keys, const adl::Buffer<u32>& offsets, adl::Buffer<u32>& indexOut,
                             int n, int numSegments, int maxSegment, bool descending, bool globalIndex)
{
    sortSegmentsTyped<K>(device, keys, offsets, 0, indexOut, n, numSegments, maxSegment, descending, globalIndex);
}

#define TAHOE_SORT_SEGMENTS(K)                                                                                                                \
    template void Pprims::sortSegments<K>(const adl::Device*, const adl::Buffer<K>&, const adl::Buffer<u32>&, adl::Buffer<K>&, adl::Buffer<u32>&, \
                                          int, int, int, bool, bool);                                                                       \
    template void Pprims::argsortSegments<K>(const adl::Device*, const adl::Buffer<K>&, const adl::Buffer<u32>&, adl::Buffer<u32>&, int, int, int, \
                                             bool, bool);
TAHOE_SORT_SEGMENTS(int)
TAHOE_SORT_SEGMENTS(float)
TAHOE_SORT_SEGMENTS(long long)
TAHOE_SORT_SEGMENTS(double)
TAHOE_SORT_SEGMENTS(u32)
TAHOE_SORT_SEGMENTS(u64)
#undef TAHOE_SORT_SEGMENTS

template <typename T>
int Pprims::uniqueTyped(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<T>& uniqueOut, adl::Buffer<u32>& countsOut, int n,
                        bool descending)
{
    ADLASSERT(n >= 0);
    if (n <= 0) return 0;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)n <= keys.getSize() && (adl::u64)n <= uniqueOut.getSize() && (adl::u64)n <= countsOut.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return 0;
        T* host = keys.getHostPtr(n);
        T* uout = uniqueOut.getHostPtr(n);
        u32* cnt = countsOut.getHostPtr(n);
        adl::DeviceUtils::waitForCompletion(device);
        std::vector<Ranked<typename KeyTraits<T>::Bits> > order;
        hostArgsort(host, n, descending, order);
        int runs = 0;
        for (int j = 0; j < n; ++j) {   // equal ordinals are equal bits: the ordinal is a bijection
            if (j == 0 || order[j].ord != order[j - 1].ord) {
                uout[runs] = host[order[j].idx];
                cnt[runs] = 0;
                ++runs;
            }
            ++cnt[runs - 1];
        }
        keys.returnHostPtr(host);
        uniqueOut.returnHostPtr(uout);
        countsOut.returnHostPtr(cnt);
        adl::DeviceUtils::waitForCompletion(device);
        return runs;
    }
    size_t wb = 0;
    const int rcq = adlhip_unique_scratch_bytes(device->hip(), KeyTraits<T>::TYPE, (size_t)n, 0, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 16, wb);   // m_tmp holds the count word
    const int rc = adlhip_unique_typed(device->hip(), KeyTraits<T>::TYPE, descending ? ADLHIP_ORDER_DESCENDING : ADLHIP_ORDER_ASCENDING,
                                       keys.m_ptr, (size_t)n, uniqueOut.m_ptr, (uint32_t*)countsOut.m_ptr, 0, 0, 0, (uint32_t*)m_tmp->m_ptr,
                                       m_work->m_ptr, (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::unique: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
    if (rc != ADLHIP_SUCCESS) return 0;
    unsigned char word[4] = {0, 0, 0, 0};
    m_tmp->read(word, 4);
    adl::DeviceUtils::waitForCompletion(device);
    u32 runs = 0;
    memcpy(&runs, word, 4);
    return (int)runs;
}

namespace {

// acc = op(acc, v) on the host, with the device's meaning: integer sums wrap (computed on the unsigned bits), float sums are IEEE adds,
// min / max compare ordinals and keep the winner's bits
template <typename V>
inline void hostReduceStep(V& acc, const V& v, int op)
{
    typedef typename KeyTraits<V>::Bits B;
    if (op == ADLHIP_REDUCE_SUM) {
        if (KeyTraits<V>::FLOAT) {
            acc = (V)(acc + v);
        } else {
            B a, b;
            memcpy(&a, &acc, sizeof(B));
            memcpy(&b, &v, sizeof(B));
            a = (B)(a + b);
            memcpy(&acc, &a, sizeof(B));
        }
        return;
    }
    const B oa = ordinal(acc, false), ov = ordinal(v, false);
    if (op == ADLHIP_REDUCE_MIN ? ov < oa : ov > oa) memcpy(&acc, &v, sizeof(V));
}

}  // namespace

template <typename K, typename V>
int Pprims::reduceByKey(const adl::Device* device, const adl::Buffer<K>& keys, const adl::Buffer<V>& values, adl::Buffer<K>& uniqueOut,
                        adl::Buffer<V>& reducedOut, int n, int op, bool descending)
{
    ADLASSERT(n >= 0);
    ADLASSERT(op == ADLHIP_REDUCE_SUM || op == ADLHIP_REDUCE_MIN || op == ADLHIP_REDUCE_MAX);
    if (n <= 0) return 0;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)n <= keys.getSize() && (adl::u64)n <= values.getSize() && (adl::u64)n <= uniqueOut.getSize() &&
              (adl::u64)n <= reducedOut.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return 0;
        K* host = keys.getHostPtr(n);
        V* vals = values.getHostPtr(n);
        K* uout = uniqueOut.getHostPtr(n);
        V* rout = reducedOut.getHostPtr(n);
        adl::DeviceUtils::waitForCompletion(device);
        std::vector<Ranked<typename KeyTraits<K>::Bits> > order;
        hostArgsort(host, n, descending, order);
        int runs = 0;
        for (int j = 0; j < n; ++j) {   // equal ordinals are equal bits: the ordinal is a bijection
            if (j == 0 || order[j].ord != order[j - 1].ord) {
                uout[runs] = host[order[j].idx];
                memcpy(&rout[runs], &vals[order[j].idx], sizeof(V));   // a run of one element keeps its bits
                ++runs;
            } else {
                hostReduceStep(rout[runs - 1], vals[order[j].idx], op);
            }
        }
        keys.returnHostPtr(host);
        values.returnHostPtr(vals);
        uniqueOut.returnHostPtr(uout);
        reducedOut.returnHostPtr(rout);
        adl::DeviceUtils::waitForCompletion(device);
        return runs;
    }
    size_t wb = 0;
    const int rcq = adlhip_reduce_by_key_scratch_bytes(device->hip(), KeyTraits<K>::TYPE, KeyTraits<V>::TYPE, (size_t)n, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 16, wb);   // m_tmp holds the count word
    const int rc = adlhip_reduce_by_key_typed(device->hip(), KeyTraits<K>::TYPE, descending ? ADLHIP_ORDER_DESCENDING : ADLHIP_ORDER_ASCENDING,
                                              keys.m_ptr, KeyTraits<V>::TYPE, op, values.m_ptr, (size_t)n, uniqueOut.m_ptr, reducedOut.m_ptr, 0, 0,
                                              (uint32_t*)m_tmp->m_ptr, m_work->m_ptr, (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::reduceByKey: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
    if (rc != ADLHIP_SUCCESS) return 0;
    unsigned char word[4] = {0, 0, 0, 0};
    m_tmp->read(word, 4);
    adl::DeviceUtils::waitForCompletion(device);
    u32 runs = 0;
    memcpy(&runs, word, 4);
    return (int)runs;
}

#define TAHOE_REDUCE(K, V)                                                                                                          \
    template int Pprims::reduceByKey<K, V>(const adl::Device*, const adl::Buffer<K>&, const adl::Buffer<V>&, adl::Buffer<K>&,       \
                                           adl::Buffer<V>&, int, int, bool);
#define TAHOE_REDUCE_KEY(K)                                                                                                         \
    TAHOE_REDUCE(K, int) TAHOE_REDUCE(K, float) TAHOE_REDUCE(K, long long) TAHOE_REDUCE(K, double) TAHOE_REDUCE(K, u32) TAHOE_REDUCE(K, u64)
TAHOE_REDUCE_KEY(int)
TAHOE_REDUCE_KEY(float)
TAHOE_REDUCE_KEY(long long)
TAHOE_REDUCE_KEY(double)
TAHOE_REDUCE_KEY(u32)
TAHOE_REDUCE_KEY(u64)
#undef TAHOE_REDUCE_KEY
#undef TAHOE_REDUCE

namespace {

// what an exclusive scan without an init writes at a head: zero bits for sums, the last / first pattern of V in ascending order for
// MIN / MAX (the inverse of ordinal() at all ones / at 0)
template <typename V>
inline V hostScanIdentity(int op)
{
    typedef typename KeyTraits<V>::Bits B;
    const B sign = (B)1 << (8 * sizeof(B) - 1);
    B b = 0;
    if (op != ADLHIP_REDUCE_SUM) {
        b = op == ADLHIP_REDUCE_MIN ? (B)~(B)0 : (B)0;   // the ordinal
        if (KeyTraits<V>::FLOAT) b = (b & sign) ? (B)(b ^ sign) : (B)~b;
        if (KeyTraits<V>::SIGNED) b ^= sign;
    }
    V v;
    memcpy(&v, &b, sizeof(B));
    return v;
}

// keys == 0: one segment
template <typename K, typename V>
void hostScan(const K* keys, const V* src, V* dst, int n, int op, bool exclusive)
{
    V acc = V();
    for (int i = 0; i < n; ++i) {
        const bool head = i == 0 || (keys && memcmp(&keys[i], &keys[i - 1], sizeof(K)) != 0);
        V x;
        memcpy(&x, &src[i], sizeof(V));   // (dst may be src)
        V out = head ? hostScanIdentity<V>(op) : acc;
        if (head) memcpy(&acc, &x, sizeof(V));   // a segment's first element keeps its bits
        else hostReduceStep(acc, x, op);
        if (!exclusive) out = acc;
        memcpy(&dst[i], &out, sizeof(V));
    }
}

}  // namespace

template <typename K, typename V>
void Pprims::scanByKey(const adl::Device* device, const adl::Buffer<K>& keys, const adl::Buffer<V>& src, adl::Buffer<V>& dst, int n, int op,
                       bool exclusive)
{
    ADLASSERT(n >= 0);
    ADLASSERT(op == ADLHIP_REDUCE_SUM || op == ADLHIP_REDUCE_MIN || op == ADLHIP_REDUCE_MAX);
    if (n <= 0) return;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)n <= keys.getSize() && (adl::u64)n <= src.getSize() && (adl::u64)n <= dst.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return;
        K* host = keys.getHostPtr(n);
        V* in = src.getHostPtr(n);
        V* out = dst.m_ptr == src.m_ptr ? in : dst.getHostPtr(n);
        adl::DeviceUtils::waitForCompletion(device);
        hostScan<K, V>(host, in, out, n, op, exclusive);
        keys.returnHostPtr(host);
        if (out != in) dst.returnHostPtr(out);
        src.returnHostPtr(in);
        adl::DeviceUtils::waitForCompletion(device);
        return;
    }
    size_t wb = 0;
    const int rcq = adlhip_scan_by_key_scratch_bytes(device->hip(), (int)sizeof(K), KeyTraits<V>::TYPE, (size_t)n, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 0, wb);
    const int rc = adlhip_scan_by_key(device->hip(), (int)sizeof(K), keys.m_ptr, KeyTraits<V>::TYPE, op, exclusive ? 1 : 0, 0, src.m_ptr,
                                      dst.m_ptr, (size_t)n, m_work->m_ptr, (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::scanByKey: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
}

template <typename V>
void Pprims::scanTyped(const adl::Device* device, const adl::Buffer<V>& src, adl::Buffer<V>& dst, int n, int op, bool exclusive)
{
    ADLASSERT(n >= 0);
    ADLASSERT(op == ADLHIP_REDUCE_SUM || op == ADLHIP_REDUCE_MIN || op == ADLHIP_REDUCE_MAX);
    if (n <= 0) return;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)n <= src.getSize() && (adl::u64)n <= dst.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return;
        V* in = src.getHostPtr(n);
        V* out = dst.m_ptr == src.m_ptr ? in : dst.getHostPtr(n);
        adl::DeviceUtils::waitForCompletion(device);
        hostScan<u32, V>(0, in, out, n, op, exclusive);
        if (out != in) dst.returnHostPtr(out);
        src.returnHostPtr(in);
        adl::DeviceUtils::waitForCompletion(device);
        return;
    }
    size_t wb = 0;
    const int rcq = adlhip_scan_typed_scratch_bytes(device->hip(), KeyTraits<V>::TYPE, (size_t)n, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 0, wb);
    const int rc = adlhip_scan_typed(device->hip(), KeyTraits<V>::TYPE, op, exclusive ? 1 : 0, 0, src.m_ptr, dst.m_ptr, (size_t)n, m_work->m_ptr,
                                     (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::scanTyped: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
}

#define TAHOE_SCAN(K, V)                                                                                                            \
    template void Pprims::scanByKey<K, V>(const adl::Device*, const adl::Buffer<K>&, const adl::Buffer<V>&, adl::Buffer<V>&, int, int, bool);
#define TAHOE_SCAN_KEY(K)                                                                                                           \
    TAHOE_SCAN(K, int) TAHOE_SCAN(K, float) TAHOE_SCAN(K, long long) TAHOE_SCAN(K, double) TAHOE_SCAN(K, u32) TAHOE_SCAN(K, u64)
TAHOE_SCAN_KEY(int)
TAHOE_SCAN_KEY(float)
TAHOE_SCAN_KEY(long long)
TAHOE_SCAN_KEY(double)
TAHOE_SCAN_KEY(u32)
TAHOE_SCAN_KEY(u64)
#undef TAHOE_SCAN_KEY
#undef TAHOE_SCAN
#define TAHOE_SCAN_PLAIN(V) template void Pprims::scanTyped<V>(const adl::Device*, const adl::Buffer<V>&, adl::Buffer<V>&, int, int, bool);
TAHOE_SCAN_PLAIN(int)
TAHOE_SCAN_PLAIN(float)
TAHOE_SCAN_PLAIN(long long)
TAHOE_SCAN_PLAIN(double)
TAHOE_SCAN_PLAIN(u32)
TAHOE_SCAN_PLAIN(u64)
#undef TAHOE_SCAN_PLAIN

namespace {

// keep[i] -> the stable order: the kept positions, then (partition) the others; returns the number kept
inline int hostCompactOrder(const std::vector<unsigned char>& keep, bool partition, std::vector<u32>& order)
{
    const int n = (int)keep.size();
    order.clear();
    for (int i = 0; i < n; ++i)
        if (keep[i]) order.push_back((u32)i);
    const int kept = (int)order.size();
    if (partition)
        for (int i = 0; i < n; ++i)
            if (!keep[i]) order.push_back((u32)i);
    return kept;
}

template <typename T>
inline void hostGather(const adl::Buffer<T>& src, adl::Buffer<T>& dst, const std::vector<u32>& order, int n)
{
    T* in = src.getHostPtr(n);
    T* out = dst.getHostPtr(n);
    adl::DeviceUtils::waitForCompletion(src.m_device);
    for (size_t j = 0; j < order.size(); ++j) memcpy(&out[j], &in[order[j]], sizeof(T));
    src.returnHostPtr(in);
    dst.returnHostPtr(out);
}

inline void hostWriteIndex(adl::Buffer<u32>* indexOut, const std::vector<u32>& order, int n)
{
    if (!indexOut) return;
    u32* out = indexOut->getHostPtr(n);
    adl::DeviceUtils::waitForCompletion(indexOut->m_device);
    for (size_t j = 0; j < order.size(); ++j) out[j] = order[j];
    indexOut->returnHostPtr(out);
}

inline bool hostCompare(int cmp, bool lt, bool eq)
{
    switch (cmp) {
    case ADLHIP_CMP_LT: return lt;
    case ADLHIP_CMP_LE: return lt || eq;
    case ADLHIP_CMP_GT: return !lt && !eq;
    case ADLHIP_CMP_GE: return !lt;
    case ADLHIP_CMP_EQ: return eq;
    default: return !eq;
    }
}

}  // namespace

template <typename T>
int Pprims::compactFlagged(const adl::Device* device, const adl::Buffer<T>& items, const adl::Buffer<unsigned char>& flags, adl::Buffer<T>& itemsOut,
                           adl::Buffer<u32>* indexOut, int n, bool partition)
{
    ADLASSERT(n >= 0);
    if (n <= 0) return 0;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)n <= items.getSize() && (adl::u64)n <= flags.getSize() && (adl::u64)n <= itemsOut.getSize() &&
              (!indexOut || (adl::u64)n <= indexOut->getSize()));
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return 0;
        unsigned char* f = flags.getHostPtr(n);
        adl::DeviceUtils::waitForCompletion(device);
        std::vector<unsigned char> keep(f, f + n);
        flags.returnHostPtr(f);
        std::vector<u32> order;
        const int kept = hostCompactOrder(keep, partition, order);
        hostGather(items, itemsOut, order, n);
        hostWriteIndex(indexOut, order, n);
        adl::DeviceUtils::waitForCompletion(device);
        return kept;
    }
    size_t wb = 0;
    const int rcq = adlhip_compact_scratch_bytes(device->hip(), (size_t)n, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 16, wb);   // m_tmp holds the count word
    const int rc = adlhip_compact_flagged(device->hip(), (int)sizeof(T), items.m_ptr, (const uint8_t*)flags.m_ptr, (size_t)n, partition ? 1 : 0,
                                          itemsOut.m_ptr, indexOut ? (uint32_t*)indexOut->m_ptr : 0, (uint32_t*)m_tmp->m_ptr, m_work->m_ptr,
                                          (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::compactFlagged: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
    if (rc != ADLHIP_SUCCESS) return 0;
    unsigned char word[4] = {0, 0, 0, 0};
    m_tmp->read(word, 4);
    adl::DeviceUtils::waitForCompletion(device);
    u32 kept = 0;
    memcpy(&kept, word, 4);
    return (int)kept;
}

template <typename K, typename V>
int Pprims::compactIf(const adl::Device* device, const adl::Buffer<K>& keys, const adl::Buffer<V>* values, int cmp, K threshold,
                      adl::Buffer<K>& keysOut, adl::Buffer<V>* valuesOut, adl::Buffer<u32>* indexOut, int n, bool partition)
{
    ADLASSERT(n >= 0);
    ADLASSERT(cmp >= ADLHIP_CMP_LT && cmp <= ADLHIP_CMP_NE);
    ADLASSERT((values != 0) == (valuesOut != 0));
    if (n <= 0) return 0;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)n <= keys.getSize() && (adl::u64)n <= keysOut.getSize() && (!values || (adl::u64)n <= values->getSize()) &&
              (!valuesOut || (adl::u64)n <= valuesOut->getSize()) && (!indexOut || (adl::u64)n <= indexOut->getSize()));
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return 0;
        K* host = keys.getHostPtr(n);
        adl::DeviceUtils::waitForCompletion(device);
        const typename KeyTraits<K>::Bits t = ordinal(threshold, false);
        std::vector<unsigned char> keep((size_t)n);
        for (int i = 0; i < n; ++i) {
            const typename KeyTraits<K>::Bits o = ordinal(host[i], false);
            keep[i] = hostCompare(cmp, o < t, o == t) ? 1 : 0;
        }
        keys.returnHostPtr(host);
        std::vector<u32> order;
        const int kept = hostCompactOrder(keep, partition, order);
        hostGather(keys, keysOut, order, n);
        if (values) hostGather(*values, *valuesOut, order, n);
        hostWriteIndex(indexOut, order, n);
        adl::DeviceUtils::waitForCompletion(device);
        return kept;
    }
    size_t wb = 0;
    const int rcq = adlhip_compact_scratch_bytes(device->hip(), (size_t)n, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 16, wb);   // m_tmp holds the count word
    const int rc = adlhip_compact_if_typed(device->hip(), KeyTraits<K>::TYPE, cmp, &threshold, keys.m_ptr, values ? (int)sizeof(V) : 0,
                                           values ? values->m_ptr : 0, (size_t)n, partition ? 1 : 0, keysOut.m_ptr,
                                           valuesOut ? valuesOut->m_ptr : 0, indexOut ? (uint32_t*)indexOut->m_ptr : 0, (uint32_t*)m_tmp->m_ptr,
                                           m_work->m_ptr, (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::compactIf: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
    if (rc != ADLHIP_SUCCESS) return 0;
    unsigned char word[4] = {0, 0, 0, 0};
    m_tmp->read(word, 4);
    adl::DeviceUtils::waitForCompletion(device);
    u32 kept = 0;
    memcpy(&kept, word, 4);
    return (int)kept;
}

#define TAHOE_COMPACT(K, V)                                                                                                         \
    template int Pprims::compactIf<K, V>(const adl::Device*, const adl::Buffer<K>&, const adl::Buffer<V>*, int, K, adl::Buffer<K>&, \
                                         adl::Buffer<V>*, adl::Buffer<u32>*, int, bool);
#define TAHOE_COMPACT_KEY(K)                                                                                                        \
    TAHOE_COMPACT(K, int) TAHOE_COMPACT(K, float) TAHOE_COMPACT(K, long long) TAHOE_COMPACT(K, double) TAHOE_COMPACT(K, u32)        \
    TAHOE_COMPACT(K, u64)                                                                                                           \
    template int Pprims::compactFlagged<K>(const adl::Device*, const adl::Buffer<K>&, const adl::Buffer<unsigned char>&, adl::Buffer<K>&, \
                                           adl::Buffer<u32>*, int, bool);
TAHOE_COMPACT_KEY(int)
TAHOE_COMPACT_KEY(float)
TAHOE_COMPACT_KEY(long long)
TAHOE_COMPACT_KEY(double)
TAHOE_COMPACT_KEY(u32)
TAHOE_COMPACT_KEY(u64)
#undef TAHOE_COMPACT_KEY
#undef TAHOE_COMPACT

// ---- histograms: adlhip_histogram_range_typed / adlhip_bincount_typed, or a plain loop ----
template <typename T>
void Pprims::histogramRange(const adl::Device* device, const adl::Buffer<T>& keys, const adl::Buffer<T>& edges, adl::Buffer<u32>& counts, int n,
                            int numBins, bool includeUpper)
{
    ADLASSERT(n >= 0);
    ADLASSERT(numBins >= 1 && numBins <= ADLHIP_HISTOGRAM_MAX_RANGE_BINS);
    if (n < 0 || numBins < 1 || numBins > ADLHIP_HISTOGRAM_MAX_RANGE_BINS) return;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)n <= keys.getSize() && (adl::u64)numBins + 1 <= edges.getSize() && (adl::u64)numBins <= counts.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return;
        typedef typename KeyTraits<T>::Bits B;
        T* e = edges.getHostPtr(numBins + 1);
        T* k = n ? keys.getHostPtr(n) : 0;
        u32* c = counts.getHostPtr(numBins);
        adl::DeviceUtils::waitForCompletion(device);
        std::vector<B> code((size_t)numBins + 1);
        for (int b = 0; b <= numBins; ++b) code[b] = ordinal(e[b], false);
        for (int b = 0; b < numBins; ++b) c[b] = 0;
        int upperBin = numBins - 1;   // where a key equal to the last edge goes: the last bin whose lower edge is below it
        while (upperBin > 0 && !(code[upperBin] < code[numBins])) --upperBin;
        if (!(code[upperBin] < code[numBins])) upperBin = numBins - 1;
        for (int i = 0; i < n; ++i) {
            const B o = ordinal(k[i], false);
            const int pos = (int)(std::upper_bound(code.begin(), code.end(), o) - code.begin());   // edges <= the key
            if (pos >= 1 && pos <= numBins) ++c[pos - 1];
            else if (pos > numBins && includeUpper && o == code[numBins]) ++c[upperBin];
        }
        edges.returnHostPtr(e);
        if (k) keys.returnHostPtr(k);
        counts.returnHostPtr(c);
        adl::DeviceUtils::waitForCompletion(device);
        return;
    }
    size_t wb = 0;
    const int rcq = adlhip_histogram_scratch_bytes(device->hip(), KeyTraits<T>::TYPE, (size_t)n, (size_t)numBins, 1, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 0, wb);
    const int rc = adlhip_histogram_range_typed(device->hip(), KeyTraits<T>::TYPE, keys.m_ptr, (size_t)n, edges.m_ptr, (size_t)numBins,
                                                includeUpper ? 1 : 0, (uint32_t*)counts.m_ptr, m_work->m_ptr, (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::histogramRange: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
}

template <typename T>
void Pprims::binCount(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<u32>& counts, int n, int numBins)
{
    ADLASSERT(!KeyTraits<T>::FLOAT);
    ADLASSERT(n >= 0 && numBins >= 1);
    if (n < 0 || numBins < 1) return;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)n <= keys.getSize() && (adl::u64)numBins <= counts.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return;
        typedef typename KeyTraits<T>::Bits B;
        T* k = n ? keys.getHostPtr(n) : 0;
        u32* c = counts.getHostPtr(numBins);
        adl::DeviceUtils::waitForCompletion(device);
        for (int b = 0; b < numBins; ++b) c[b] = 0;
        for (int i = 0; i < n; ++i) {
            B bits;
            memcpy(&bits, &k[i], sizeof(B));   // a negative key is a large unsigned number
            if (bits < (B)numBins) ++c[(size_t)bits];
        }
        if (k) keys.returnHostPtr(k);
        counts.returnHostPtr(c);
        adl::DeviceUtils::waitForCompletion(device);
        return;
    }
    size_t wb = 0;
    const int rcq = adlhip_histogram_scratch_bytes(device->hip(), KeyTraits<T>::TYPE, (size_t)n, (size_t)numBins, 0, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 0, wb);
    const int rc = adlhip_bincount_typed(device->hip(), KeyTraits<T>::TYPE, keys.m_ptr, (size_t)n, (size_t)numBins, (uint32_t*)counts.m_ptr,
                                         m_work->m_ptr, (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::binCount: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
}

#define TAHOE_HISTOGRAM(T)                                                                                                                  \
    template void Pprims::histogramRange<T>(const adl::Device*, const adl::Buffer<T>&, const adl::Buffer<T>&, adl::Buffer<u32>&, int, int, bool);
#define TAHOE_BINCOUNT(T) template void Pprims::binCount<T>(const adl::Device*, const adl::Buffer<T>&, adl::Buffer<u32>&, int, int);
TAHOE_HISTOGRAM(int)
TAHOE_HISTOGRAM(float)
TAHOE_HISTOGRAM(long long)
TAHOE_HISTOGRAM(double)
TAHOE_HISTOGRAM(u32)
TAHOE_HISTOGRAM(u64)
TAHOE_BINCOUNT(int)
TAHOE_BINCOUNT(long long)
TAHOE_BINCOUNT(u32)
TAHOE_BINCOUNT(u64)
#undef TAHOE_BINCOUNT
#undef TAHOE_HISTOGRAM

// ---- merge of sorted sequences: adlhip_merge_typed, or a plain two-pointer loop ----
template <typename K, typename V>
void Pprims::mergePairs(const adl::Device* device, const adl::Buffer<K>& keysA, const adl::Buffer<V>* valuesA, const adl::Buffer<K>& keysB,
                        const adl::Buffer<V>* valuesB, adl::Buffer<K>& keysOut, adl::Buffer<V>* valuesOut, adl::Buffer<u32>* indexOut, int na,
                        int nb, bool descending)
{
    ADLASSERT(na >= 0 && nb >= 0);
    ADLASSERT((valuesA != 0) == (valuesOut != 0) && (valuesB != 0) == (valuesOut != 0));
    ADLASSERT((long long)na + nb <= 0x7fffffffLL);   // (the facade counts in int)
    if (na < 0 || nb < 0 || (long long)na + nb > 0x7fffffffLL || na + nb == 0) return;
    const int n = na + nb;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)na <= keysA.getSize() && (adl::u64)nb <= keysB.getSize() && (adl::u64)n <= keysOut.getSize() &&
              (!valuesA || (adl::u64)na <= valuesA->getSize()) && (!valuesB || (adl::u64)nb <= valuesB->getSize()) &&
              (!valuesOut || (adl::u64)n <= valuesOut->getSize()) && (!indexOut || (adl::u64)n <= indexOut->getSize()));
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return;
        K* a = na ? keysA.getHostPtr(na) : 0;
        K* b = nb ? keysB.getHostPtr(nb) : 0;
        V* va = valuesA && na ? valuesA->getHostPtr(na) : 0;
        V* vb = valuesB && nb ? valuesB->getHostPtr(nb) : 0;
        K* out = keysOut.getHostPtr(n);
        V* vout = valuesOut ? valuesOut->getHostPtr(n) : 0;
        u32* idx = indexOut ? indexOut->getHostPtr(n) : 0;
        adl::DeviceUtils::waitForCompletion(device);
        int i = 0, j = 0;
        for (int o = 0; o < n; ++o) {   // b goes first only where it is strictly in front: a tie takes a
            const bool takeB = i >= na || (j < nb && ordinal(b[j], descending) < ordinal(a[i], descending));
            out[o] = takeB ? b[j] : a[i];
            if (vout) vout[o] = takeB ? vb[j] : va[i];
            if (idx) idx[o] = takeB ? (u32)(na + j) : (u32)i;
            if (takeB) ++j;
            else ++i;
        }
        if (a) keysA.returnHostPtr(a);
        if (b) keysB.returnHostPtr(b);
        if (va) valuesA->returnHostPtr(va);
        if (vb) valuesB->returnHostPtr(vb);
        keysOut.returnHostPtr(out);
        if (vout) valuesOut->returnHostPtr(vout);
        if (idx) indexOut->returnHostPtr(idx);
        adl::DeviceUtils::waitForCompletion(device);
        return;
    }
    const int vbytes = valuesOut ? (int)sizeof(V) : 0;
    size_t wb = 0;
    const int rcq = adlhip_merge_scratch_bytes(device->hip(), KeyTraits<K>::TYPE, vbytes, (size_t)na, (size_t)nb, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 0, wb);
    const int rc = adlhip_merge_typed(device->hip(), KeyTraits<K>::TYPE, descending ? ADLHIP_ORDER_DESCENDING : ADLHIP_ORDER_ASCENDING,
                                      keysA.m_ptr, valuesA ? valuesA->m_ptr : 0, (size_t)na, keysB.m_ptr, valuesB ? valuesB->m_ptr : 0,
                                      (size_t)nb, vbytes, keysOut.m_ptr, valuesOut ? valuesOut->m_ptr : 0,
                                      indexOut ? (uint32_t*)indexOut->m_ptr : 0, m_work->m_ptr, (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::merge: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
}

#define TAHOE_MERGE(K, V)                                                                                                           \
    template void Pprims::mergePairs<K, V>(const adl::Device*, const adl::Buffer<K>&, const adl::Buffer<V>*, const adl::Buffer<K>&, \
                                           const adl::Buffer<V>*, adl::Buffer<K>&, adl::Buffer<V>*, adl::Buffer<u32>*, int, int, bool);
#define TAHOE_MERGE_KEY(K) \
    TAHOE_MERGE(K, int) TAHOE_MERGE(K, float) TAHOE_MERGE(K, long long) TAHOE_MERGE(K, double) TAHOE_MERGE(K, u32) TAHOE_MERGE(K, u64)
TAHOE_MERGE_KEY(int)
TAHOE_MERGE_KEY(float)
TAHOE_MERGE_KEY(long long)
TAHOE_MERGE_KEY(double)
TAHOE_MERGE_KEY(u32)
TAHOE_MERGE_KEY(u64)
#undef TAHOE_MERGE_KEY
#undef TAHOE_MERGE

// ---- set operations on sorted sequences: adlhip_set_op_typed, or thrust's two-pointer loops ----
template <typename K, typename V>
int Pprims::setOp(const adl::Device* device, int op, const adl::Buffer<K>& keysA, const adl::Buffer<V>* valuesA, const adl::Buffer<K>& keysB,
                  const adl::Buffer<V>* valuesB, adl::Buffer<K>& keysOut, adl::Buffer<V>* valuesOut, adl::Buffer<u32>* indexOut, int na, int nb,
                  bool descending)
{
    ADLASSERT(na >= 0 && nb >= 0);
    ADLASSERT(op >= ADLHIP_SETOP_INTERSECTION && op <= ADLHIP_SETOP_SYMMETRIC_DIFFERENCE);
    ADLASSERT((valuesA != 0) == (valuesOut != 0) && (valuesB != 0) == (valuesOut != 0));
    ADLASSERT((long long)na + nb <= 0x7fffffffLL);   // (the facade counts in int)
    if (na < 0 || nb < 0 || (long long)na + nb > 0x7fffffffLL || na + nb == 0) return 0;
    if (op < ADLHIP_SETOP_INTERSECTION || op > ADLHIP_SETOP_SYMMETRIC_DIFFERENCE) return 0;
    const bool both = op == ADLHIP_SETOP_UNION || op == ADLHIP_SETOP_SYMMETRIC_DIFFERENCE;
    const int cap = both ? na + nb : na;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)na <= keysA.getSize() && (adl::u64)nb <= keysB.getSize() && (adl::u64)cap <= keysOut.getSize() &&
              (!valuesA || (adl::u64)na <= valuesA->getSize()) && (!valuesB || (adl::u64)nb <= valuesB->getSize()) &&
              (!valuesOut || (adl::u64)cap <= valuesOut->getSize()) && (!indexOut || (adl::u64)cap <= indexOut->getSize()));
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return 0;
        if (cap == 0) return 0;
        K* a = na ? keysA.getHostPtr(na) : 0;
        K* b = nb ? keysB.getHostPtr(nb) : 0;
        V* va = valuesA && na ? valuesA->getHostPtr(na) : 0;
        V* vb = valuesB && nb ? valuesB->getHostPtr(nb) : 0;
        K* out = keysOut.getHostPtr(cap);
        V* vout = valuesOut ? valuesOut->getHostPtr(cap) : 0;
        u32* idx = indexOut ? indexOut->getHostPtr(cap) : 0;
        adl::DeviceUtils::waitForCompletion(device);
        const bool keepOnlyA = op != ADLHIP_SETOP_INTERSECTION;   // an element of A with nothing equal left in B
        const bool keepEqual = op == ADLHIP_SETOP_INTERSECTION || op == ADLHIP_SETOP_UNION;   // a pair of equal elements: A's
        int i = 0, j = 0, o = 0;
        while (i < na || j < nb) {
            const bool onlyA = j >= nb || (i < na && ordinal(a[i], descending) < ordinal(b[j], descending));
            const bool onlyB = !onlyA && (i >= na || ordinal(b[j], descending) < ordinal(a[i], descending));
            const bool fromB = onlyB;
            const bool keep = onlyA ? keepOnlyA : (onlyB ? both : keepEqual);
            if (keep) {
                out[o] = fromB ? b[j] : a[i];
                if (vout) vout[o] = fromB ? vb[j] : va[i];
                if (idx) idx[o] = fromB ? (u32)(na + j) : (u32)i;
                ++o;
            }
            if (!onlyB) ++i;
            if (!onlyA) ++j;
        }
        if (a) keysA.returnHostPtr(a);
        if (b) keysB.returnHostPtr(b);
        if (va) valuesA->returnHostPtr(va);
        if (vb) valuesB->returnHostPtr(vb);
        keysOut.returnHostPtr(out);
        if (vout) valuesOut->returnHostPtr(vout);
        if (idx) indexOut->returnHostPtr(idx);
        adl::DeviceUtils::waitForCompletion(device);
        return o;
    }
    const int vbytes = valuesOut ? (int)sizeof(V) : 0;
    size_t wb = 0;
    const int rcq = adlhip_set_op_scratch_bytes(device->hip(), KeyTraits<K>::TYPE, vbytes, (size_t)na, (size_t)nb, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 16, wb);   // m_tmp holds the count word
    const int rc = adlhip_set_op_typed(device->hip(), KeyTraits<K>::TYPE, descending ? ADLHIP_ORDER_DESCENDING : ADLHIP_ORDER_ASCENDING, op,
                                       keysA.m_ptr, valuesA ? valuesA->m_ptr : 0, (size_t)na, keysB.m_ptr, valuesB ? valuesB->m_ptr : 0,
                                       (size_t)nb, vbytes, keysOut.m_ptr, valuesOut ? valuesOut->m_ptr : 0,
                                       indexOut ? (uint32_t*)indexOut->m_ptr : 0, (uint32_t*)m_tmp->m_ptr, m_work->m_ptr,
                                       (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::setOp: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
    if (rc != ADLHIP_SUCCESS) return 0;
    unsigned char word[4] = {0, 0, 0, 0};
    m_tmp->read(word, 4);
    adl::DeviceUtils::waitForCompletion(device);
    u32 kept = 0;
    memcpy(&kept, word, 4);
    return (int)kept;
}

#define TAHOE_SETOP(K, V)                                                                                                           \
    template int Pprims::setOp<K, V>(const adl::Device*, int, const adl::Buffer<K>&, const adl::Buffer<V>*, const adl::Buffer<K>&, \
                                     const adl::Buffer<V>*, adl::Buffer<K>&, adl::Buffer<V>*, adl::Buffer<u32>*, int, int, bool);
#define TAHOE_SETOP_KEY(K) \
    TAHOE_SETOP(K, int) TAHOE_SETOP(K, float) TAHOE_SETOP(K, long long) TAHOE_SETOP(K, double) TAHOE_SETOP(K, u32) TAHOE_SETOP(K, u64)
TAHOE_SETOP_KEY(int)
TAHOE_SETOP_KEY(float)
TAHOE_SETOP_KEY(long long)
TAHOE_SETOP_KEY(double)
TAHOE_SETOP_KEY(u32)
TAHOE_SETOP_KEY(u64)
#undef TAHOE_SETOP_KEY
#undef TAHOE_SETOP

// ---- sorted search: adlhip_search_sorted_typed, or a plain binary search per needle ----
template <typename K>
void Pprims::searchSorted(const adl::Device* device, const adl::Buffer<K>& sortedKeys, const adl::Buffer<K>& needles, adl::Buffer<u32>& posOut, int m,
                          int n, bool descending, bool right)
{
    ADLASSERT(m >= 0 && n >= 0);
    if (m < 0 || n <= 0) return;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)m <= sortedKeys.getSize() && (adl::u64)n <= needles.getSize() && (adl::u64)n <= posOut.getSize());
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return;
        K* s = m ? sortedKeys.getHostPtr(m) : 0;
        K* x = needles.getHostPtr(n);
        u32* pos = posOut.getHostPtr(n);
        adl::DeviceUtils::waitForCompletion(device);
        for (int i = 0; i < n; ++i) {   // the first position whose element is not below (right: is above) the needle
            int lo = 0, hi = m;
            while (lo < hi) {
                const int mid = lo + (hi - lo) / 2;
                const bool before = right ? !(ordinal(x[i], descending) < ordinal(s[mid], descending))
                                          : ordinal(s[mid], descending) < ordinal(x[i], descending);
                if (before) lo = mid + 1;
                else hi = mid;
            }
            pos[i] = (u32)lo;
        }
        if (s) sortedKeys.returnHostPtr(s);
        needles.returnHostPtr(x);
        posOut.returnHostPtr(pos);
        adl::DeviceUtils::waitForCompletion(device);
        return;
    }
    const int rc = adlhip_search_sorted_typed(device->hip(), KeyTraits<K>::TYPE, descending ? ADLHIP_ORDER_DESCENDING : ADLHIP_ORDER_ASCENDING,
                                              right ? ADLHIP_SEARCH_RIGHT : ADLHIP_SEARCH_LEFT, m ? sortedKeys.m_ptr : 0, (size_t)m, needles.m_ptr,
                                              (size_t)n, (uint32_t*)posOut.m_ptr);
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::searchSorted: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
}

#define TAHOE_SEARCH(K) \
    template void Pprims::searchSorted<K>(const adl::Device*, const adl::Buffer<K>&, const adl::Buffer<K>&, adl::Buffer<u32>&, int, int, bool, bool);
TAHOE_SEARCH(int)
TAHOE_SEARCH(float)
TAHOE_SEARCH(long long)
TAHOE_SEARCH(double)
TAHOE_SEARCH(u32)
TAHOE_SEARCH(u64)
#undef TAHOE_SEARCH

// ---- join of sorted sequences: adlhip_join_sorted_typed, or a two-pointer loop ----
template <typename K>
unsigned long long Pprims::joinSorted(const adl::Device* device, int kind, const adl::Buffer<K>& keysA, const adl::Buffer<K>& keysB,
                                      adl::Buffer<u32>* indexA, adl::Buffer<u32>* indexB, int na, int nb, int cap, bool descending)
{
    ADLASSERT(na >= 0 && nb >= 0 && cap >= 0);
    ADLASSERT(kind >= ADLHIP_JOIN_INNER && kind <= ADLHIP_JOIN_ANTI);
    ADLASSERT((long long)na + nb <= 0x7fffffffLL && (long long)na + cap <= 0x7fffffffLL);   // (the facade counts in int)
    ADLASSERT(cap ? (indexA || indexB) : (!indexA && !indexB));
    if (na <= 0 || nb < 0 || cap < 0 || (long long)na + nb > 0x7fffffffLL || (long long)na + cap > 0x7fffffffLL) return 0;
    if (kind < ADLHIP_JOIN_INNER || kind > ADLHIP_JOIN_ANTI || (cap ? (!indexA && !indexB) : (indexA || indexB))) return 0;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)na <= keysA.getSize() && (adl::u64)nb <= keysB.getSize() && (!indexA || (adl::u64)cap <= indexA->getSize()) &&
              (!indexB || (adl::u64)cap <= indexB->getSize()));
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return 0;
        K* a = keysA.getHostPtr(na);
        K* b = nb ? keysB.getHostPtr(nb) : 0;
        u32* ia = indexA ? indexA->getHostPtr(cap) : 0;
        u32* ib = indexB ? indexB->getHostPtr(cap) : 0;
        adl::DeviceUtils::waitForCompletion(device);
        unsigned long long total = 0;
        int lo = 0;
        for (int i = 0; i < na; ++i) {
            while (lo < nb && ordinal(b[lo], descending) < ordinal(a[i], descending)) ++lo;   // (A is sorted: lo only moves on)
            int m = 0;
            while (lo + m < nb && ordinal(b[lo + m], descending) == ordinal(a[i], descending)) ++m;
            const int rows = kind == ADLHIP_JOIN_INNER ? m : kind == ADLHIP_JOIN_LEFT ? (m ? m : 1) : kind == ADLHIP_JOIN_SEMI ? (m ? 1 : 0) : (m ? 0 : 1);
            for (int r = 0; r < rows && total + (unsigned long long)r < (unsigned long long)cap; ++r) {
                if (ia) ia[total + r] = (u32)i;
                if (ib) ib[total + r] = m && kind != ADLHIP_JOIN_ANTI ? (u32)(lo + r) : ADLHIP_JOIN_NONE;
            }
            total += (unsigned long long)rows;
        }
        keysA.returnHostPtr(a);
        if (b) keysB.returnHostPtr(b);
        if (ia) indexA->returnHostPtr(ia);
        if (ib) indexB->returnHostPtr(ib);
        adl::DeviceUtils::waitForCompletion(device);
        return total;
    }
    size_t wb = 0;
    const int rcq = adlhip_join_scratch_bytes(device->hip(), KeyTraits<K>::TYPE, (size_t)na, (size_t)nb, (size_t)cap, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 16, wb);   // m_tmp holds the count word
    const int rc = adlhip_join_sorted_typed(device->hip(), KeyTraits<K>::TYPE, descending ? ADLHIP_ORDER_DESCENDING : ADLHIP_ORDER_ASCENDING, kind,
                                            keysA.m_ptr, (size_t)na, nb ? keysB.m_ptr : 0, (size_t)nb, (size_t)cap,
                                            indexA ? (uint32_t*)indexA->m_ptr : 0, indexB ? (uint32_t*)indexB->m_ptr : 0, (uint64_t*)m_tmp->m_ptr,
                                            m_work->m_ptr, (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::joinSorted: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
    if (rc != ADLHIP_SUCCESS) return 0;
    unsigned char word[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    m_tmp->read(word, 8);
    adl::DeviceUtils::waitForCompletion(device);
    unsigned long long total = 0;
    memcpy(&total, word, 8);
    return total;
}

#define TAHOE_JOIN(K)                                                                                                                     \
    template unsigned long long Pprims::joinSorted<K>(const adl::Device*, int, const adl::Buffer<K>&, const adl::Buffer<K>&, adl::Buffer<u32>*, \
                                                      adl::Buffer<u32>*, int, int, int, bool);
TAHOE_JOIN(int)
TAHOE_JOIN(float)
TAHOE_JOIN(long long)
TAHOE_JOIN(double)
TAHOE_JOIN(u32)
TAHOE_JOIN(u64)
#undef TAHOE_JOIN

// ---- expansion of runs: adlhip_expand_runs, or a loop over the runs ----
template <typename V>
unsigned long long Pprims::expandRuns(const adl::Device* device, const adl::Buffer<u32>& counts, const adl::Buffer<V>* values, adl::Buffer<u32>* runOut,
                                      adl::Buffer<u32>* rankOut, adl::Buffer<V>* valuesOut, int numRuns, int cap)
{
    ADLASSERT(numRuns >= 0 && cap >= 0 && (long long)numRuns + cap <= 0x7fffffffLL);
    ADLASSERT(cap ? (runOut || rankOut || valuesOut) : (!runOut && !rankOut && !valuesOut));
    ADLASSERT(!valuesOut || values);
    if (numRuns <= 0 || cap < 0 || (long long)numRuns + cap > 0x7fffffffLL || (valuesOut && !values)) return 0;
    if (cap ? (!runOut && !rankOut && !valuesOut) : (runOut || rankOut || valuesOut)) return 0;
    ADLASSERT(device != 0);
    ADLASSERT((adl::u64)numRuns <= counts.getSize() && (!valuesOut || (adl::u64)numRuns <= values->getSize()) &&
              (!runOut || (adl::u64)cap <= runOut->getSize()) && (!rankOut || (adl::u64)cap <= rankOut->getSize()) &&
              (!valuesOut || (adl::u64)cap <= valuesOut->getSize()));
    if (!onDevice(device)) {
        ADLASSERT(device->getType() == adl::TYPE_HOST);   // a HIP device never falls back to the CPU
        if (device->getType() != adl::TYPE_HOST) return 0;
        u32* c = counts.getHostPtr(numRuns);
        V* v = valuesOut ? values->getHostPtr(numRuns) : 0;
        u32* run = runOut ? runOut->getHostPtr(cap) : 0;
        u32* rank = rankOut ? rankOut->getHostPtr(cap) : 0;
        V* vout = valuesOut ? valuesOut->getHostPtr(cap) : 0;
        adl::DeviceUtils::waitForCompletion(device);
        unsigned long long total = 0;
        for (int i = 0; i < numRuns; ++i) {
            for (u32 r = 0; r < c[i] && total + r < (unsigned long long)cap; ++r) {
                if (run) run[total + r] = (u32)i;
                if (rank) rank[total + r] = r;
                if (vout) vout[total + r] = v[i];
            }
            total += c[i];
        }
        counts.returnHostPtr(c);
        if (v) values->returnHostPtr(v);
        if (run) runOut->returnHostPtr(run);
        if (rank) rankOut->returnHostPtr(rank);
        if (vout) valuesOut->returnHostPtr(vout);
        adl::DeviceUtils::waitForCompletion(device);
        return total;
    }
    size_t wb = 0;
    const int rcq = adlhip_expand_scratch_bytes(device->hip(), (size_t)numRuns, (size_t)cap, &wb);
    ADLASSERT(rcq == ADLHIP_SUCCESS);
    reserve(device, 16, wb);   // m_tmp holds the count word
    const int rc = adlhip_expand_runs(device->hip(), (const uint32_t*)counts.m_ptr, (size_t)numRuns, valuesOut ? (int)sizeof(V) : 0,
                                      valuesOut ? values->m_ptr : 0, (size_t)cap, runOut ? (uint32_t*)runOut->m_ptr : 0,
                                      rankOut ? (uint32_t*)rankOut->m_ptr : 0, valuesOut ? valuesOut->m_ptr : 0, (uint64_t*)m_tmp->m_ptr,
                                      m_work->m_ptr, (size_t)m_work->getSize());
    if (rc != ADLHIP_SUCCESS) TH_LOG_ERROR("Pprims::expandRuns: %s\n", adlhip_last_error());
    ADLASSERT(rc == ADLHIP_SUCCESS);
    if (rc != ADLHIP_SUCCESS) return 0;
    unsigned char word[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    m_tmp->read(word, 8);
    adl::DeviceUtils::waitForCompletion(device);
    unsigned long long total = 0;
    memcpy(&total, word, 8);
    return total;
}

#define TAHOE_EXPAND(V)                                                                                                                     \
    template unsigned long long Pprims::expandRuns<V>(const adl::Device*, const adl::Buffer<u32>&, const adl::Buffer<V>*, adl::Buffer<u32>*, \
                                                      adl::Buffer<u32>*, adl::Buffer<V>*, int, int);
TAHOE_EXPAND(int)
TAHOE_EXPAND(float)
TAHOE_EXPAND(long long)
TAHOE_EXPAND(double)
TAHOE_EXPAND(u32)
TAHOE_EXPAND(u64)
#undef TAHOE_EXPAND

#define TAHOE_TYPED(T)                                                                                                              \
    void Pprims::sortKeys(const adl::Device* device, const adl::Buffer<T>& inout, int n, bool descending)                         \
    {                                                                                                                               \
        sortKeysTyped<T>(device, inout, n, descending);                                                                             \
    }                                                                                                                               \
    void Pprims::argsort(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<u32>& indexOut, int n, bool descending) \
    {                                                                                                                               \
        argsortTyped<T>(device, keys, indexOut, n, descending);                                                                     \
    }                                                                                                                               \
    void Pprims::topK(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<T>& keysOut, adl::Buffer<u32>& indexOut,  \
                      int n, int k, bool descending)                                                                                \
    {                                                                                                                               \
        topKTyped<T>(device, keys, keysOut, indexOut, n, k, descending);                                                            \
    }                                                                                                                               \
    void Pprims::topKRows(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<T>& keysOut, adl::Buffer<u32>& indexOut, \
                          int rows, int cols, int k, bool descending, int rowStride)                                                \
    {                                                                                                                               \
        topKRowsTyped<T>(device, keys, keysOut, indexOut, rows, cols, k, descending, rowStride);                                    \
    }                                                                                                                               \
    int Pprims::unique(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<T>& uniqueOut, adl::Buffer<u32>& countsOut, \
                       int n, bool descending)                                                                                      \
    {                                                                                                                               \
        return uniqueTyped<T>(device, keys, uniqueOut, countsOut, n, descending);                                                   \
    }
TAHOE_TYPED(int)
TAHOE_TYPED(float)
TAHOE_TYPED(long long)
TAHOE_TYPED(double)
TAHOE_TYPED(u32)
TAHOE_TYPED(u64)
#undef TAHOE_TYPED

}  // namespace Tahoe
