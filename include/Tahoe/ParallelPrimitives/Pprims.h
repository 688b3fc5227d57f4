// Tahoe/ParallelPrimitives/Pprims.h -- the parallel-primitives object of the reference
// (Tahoe/ParallelPrimitives/Pprims.h:11-48) over the MI355X HIP back-end:
//   scan      exclusive prefix sum                                   (reference Pprims.h:35)
//   radixSort {u32 key, u32 value} pairs, stable                     (reference Pprims.h:38)
//   radixSort u32 keys                                               (reference Pprims.h:41)
//   radixSort u64 keys                                               (new: BASELINE config #5)
//   copy / fill                                                      (reference Pprims.cpp:31-120, commented out there)
//   sortKeys / argsort  signed, float and descending keys            (new: adlhip_sort_keys_typed / adlhip_argsort_typed)
//   topK      the first k entries of argsort, by selection           (new: adlhip_topk_typed)
//   topKRows  topK of every row of a rows x cols matrix              (new: adlhip_topk_rows_typed)
//   sortRows / argsortRows  every row of a rows x cols matrix sorted (new: adlhip_sort_rows_typed)
//   sortSegments / argsortSegments  every segment [offsets[s], offsets[s + 1]) sorted (new: adlhip_sort_segments_typed)
//   unique    distinct keys in sorted order and their counts         (new: adlhip_unique_typed)
//   reduceByKey  sum / min / max of the values of every distinct key  (new: adlhip_reduce_by_key_typed)
// Same argument meaning; differences, all supersets: any n >= 0 (the reference needs n % 256 == 0 for
// keys), scan has no 1,048,576-element limit, sortBits < 32 also works on 64-bit keys up to 64.
// Device work is enqueued and the call returns (no sync), as in the reference's GPU branches.
// A TYPE_HOST device takes the CPU path (Tahoe::RadixSort::sort), exactly as Pprims.cpp:202-212/306-316;
// a TYPE_CL (HIP) device never falls back to the CPU.
#pragma once
#include <Adl/Adl.h>
#include <Tahoe/Math/Math.h>
#include <Tahoe/ParallelPrimitives/uArray.h>   // the reference's Pprims.h pulls uArray / Array in for its users

namespace Tahoe {

class Pprims {
public:
    TH_DECLARE_ALLOCATOR(Pprims);

    Pprims();
    ~Pprims();

    void cacheKernel(bool cache) { m_cacheKernel = cache; }   // kernels are built ahead of time; kept for API parity

    enum {
        SCAN_BLOCK_SIZE = 128,
        RSORT_BITS_PER_PASS = 8,
        RSORT_NUM_TABLES = (1 << RSORT_BITS_PER_PASS),
        R32SORT_DATA_ALIGNMENT = 256,   // the reference's requirement on n; not needed here
        R32SORT_WG_SIZE = 64,
        R32SORT_ELEMENTS_PER_WORK_ITEM = (256 / R32SORT_WG_SIZE),
        R32SORT_BITS_PER_PASS = 4,      // the reference's digit width; select with adlhip "sort.digit_bits"
    };

    // copy / fill (Pprims.cpp:31-120 -- present but commented out in the reference, with CopyIntKernel / CopyF4Kernel /
    // FillIntKernel / FillU32Kernel / FillF4Kernel of ClKernels/PprimsKernels.cl): first n elements, enqueued
    void copy(const adl::Device* device, adl::Buffer<int>& dst, const adl::Buffer<int>& src, int n);
    void copy(const adl::Device* device, adl::Buffer<float4>& dst, const adl::Buffer<float4>& src, int n);
    void fill(const adl::Device* device, adl::Buffer<int>& dst, int src, int n);
    void fill(const adl::Device* device, adl::Buffer<u32>& dst, u32 src, int n);
    void fill(const adl::Device* device, adl::Buffer<float4>& dst, const float4& src, int n);

    void scan(const adl::Device* device, adl::Buffer<int>& dst, const adl::Buffer<int>& src, int n, u32* sumOut = 0);

    // inout.x: key, inout.y: value
    void radixSort(const adl::Device* device, const adl::Buffer<uint2>& inout, int n, int sortBits = 32);

    void radixSort(const adl::Device* device, const adl::Buffer<u32>& inout, int n, int sortBits = 32);

    void radixSort(const adl::Device* device, const adl::Buffer<u64>& inout, int n, int sortBits = 64);

    // separate key and value buffers (the layout of the reference's never-launched SoA kernel,
    // RadixSortKeyValueKernels.cl:354-509): ascending by key, stable, values follow their keys
    void radixSort(const adl::Device* device, const adl::Buffer<u32>& keys, const adl::Buffer<u32>& values, int n,
                   int sortBits = 32);
    // the same with 64-bit values and / or 64-bit keys: {32 key bits, index} pairs are sorted, keys and values
    // gathered once at the end (adlhip_radix_sort_soa)
    void radixSort(const adl::Device* device, const adl::Buffer<u32>& keys, const adl::Buffer<u64>& values, int n,
                   int sortBits = 32);
    void radixSort(const adl::Device* device, const adl::Buffer<u64>& keys, const adl::Buffer<u32>& values, int n,
                   int sortBits = 64);
    void radixSort(const adl::Device* device, const adl::Buffer<u64>& keys, const adl::Buffer<u64>& values, int n,
                   int sortBits = 64);

    // typed keys (no reference counterpart): signed integers by value, floats in IEEE-754 totalOrder (-NaN < -inf < ... < -0 < +0
    // < ... < +inf < +NaN), ascending or descending, in place.  A TYPE_HOST device sorts on the CPU (std::stable_sort on the same
    // order, src/TypedSort.cpp)
    void sortKeys(const adl::Device* device, const adl::Buffer<int>& inout, int n, bool descending = false);
    void sortKeys(const adl::Device* device, const adl::Buffer<float>& inout, int n, bool descending = false);
    void sortKeys(const adl::Device* device, const adl::Buffer<long long>& inout, int n, bool descending = false);
    void sortKeys(const adl::Device* device, const adl::Buffer<double>& inout, int n, bool descending = false);
    void sortKeys(const adl::Device* device, const adl::Buffer<u32>& inout, int n, bool descending = false);
    void sortKeys(const adl::Device* device, const adl::Buffer<u64>& inout, int n, bool descending = false);
    // indexOut[j] = position in keys of the j-th element of the sorted order; stable (equal keys in input order, descending too);
    // keys is left intact
    void argsort(const adl::Device* device, const adl::Buffer<int>& keys, adl::Buffer<u32>& indexOut, int n, bool descending = false);
    void argsort(const adl::Device* device, const adl::Buffer<float>& keys, adl::Buffer<u32>& indexOut, int n, bool descending = false);
    void argsort(const adl::Device* device, const adl::Buffer<long long>& keys, adl::Buffer<u32>& indexOut, int n, bool descending = false);
    void argsort(const adl::Device* device, const adl::Buffer<double>& keys, adl::Buffer<u32>& indexOut, int n, bool descending = false);
    void argsort(const adl::Device* device, const adl::Buffer<u32>& keys, adl::Buffer<u32>& indexOut, int n, bool descending = false);
    void argsort(const adl::Device* device, const adl::Buffer<u64>& keys, adl::Buffer<u32>& indexOut, int n, bool descending = false);
    // the first k entries of argsort: indexOut[j] (j < k) = position of the j-th smallest (descending: largest) key, ties by ascending
    // position; keysOut[j] = that key.  keys is left intact.  A TYPE_HOST device sorts (ordinal, position) on the CPU
    void topK(const adl::Device* device, const adl::Buffer<int>& keys, adl::Buffer<int>& keysOut, adl::Buffer<u32>& indexOut, int n, int k,
              bool descending = false);
    void topK(const adl::Device* device, const adl::Buffer<float>& keys, adl::Buffer<float>& keysOut, adl::Buffer<u32>& indexOut, int n, int k,
              bool descending = false);
    void topK(const adl::Device* device, const adl::Buffer<long long>& keys, adl::Buffer<long long>& keysOut, adl::Buffer<u32>& indexOut, int n, int k,
              bool descending = false);
    void topK(const adl::Device* device, const adl::Buffer<double>& keys, adl::Buffer<double>& keysOut, adl::Buffer<u32>& indexOut, int n, int k,
              bool descending = false);
    void topK(const adl::Device* device, const adl::Buffer<u32>& keys, adl::Buffer<u32>& keysOut, adl::Buffer<u32>& indexOut, int n, int k,
              bool descending = false);
    void topK(const adl::Device* device, const adl::Buffer<u64>& keys, adl::Buffer<u64>& keysOut, adl::Buffer<u32>& indexOut, int n, int k,
              bool descending = false);
    // topK of every row of a rows x cols matrix, row r at element r * rowStride (0: cols): indexOut[r * k + j] = column of the j-th
    // smallest (descending: largest) key of row r, ties by ascending column; keysOut[r * k + j] = that key.  keys is left intact.  A
    // TYPE_HOST device partially sorts (ordinal, column) per row on the CPU
    void topKRows(const adl::Device* device, const adl::Buffer<int>& keys, adl::Buffer<int>& keysOut, adl::Buffer<u32>& indexOut, int rows,
                  int cols, int k, bool descending = false, int rowStride = 0);
    void topKRows(const adl::Device* device, const adl::Buffer<float>& keys, adl::Buffer<float>& keysOut, adl::Buffer<u32>& indexOut, int rows,
                  int cols, int k, bool descending = false, int rowStride = 0);
    void topKRows(const adl::Device* device, const adl::Buffer<long long>& keys, adl::Buffer<long long>& keysOut, adl::Buffer<u32>& indexOut, int rows,
                  int cols, int k, bool descending = false, int rowStride = 0);
    void topKRows(const adl::Device* device, const adl::Buffer<double>& keys, adl::Buffer<double>& keysOut, adl::Buffer<u32>& indexOut, int rows,
                  int cols, int k, bool descending = false, int rowStride = 0);
    void topKRows(const adl::Device* device, const adl::Buffer<u32>& keys, adl::Buffer<u32>& keysOut, adl::Buffer<u32>& indexOut, int rows,
                  int cols, int k, bool descending = false, int rowStride = 0);
    void topKRows(const adl::Device* device, const adl::Buffer<u64>& keys, adl::Buffer<u64>& keysOut, adl::Buffer<u32>& indexOut, int rows,
                  int cols, int k, bool descending = false, int rowStride = 0);
    // the distinct keys among the first n of keys, in the order of sortKeys(descending), and how often each occurs: uniqueOut[r] and
    // countsOut[r] for r < R; both hold n elements, those at R and beyond are left alone.  Keys are equal when their bits are (-0 and
    // +0 are two keys, NaNs with different payloads too).  keys is left intact.  Unlike the calls above this one WAITS and returns R.
    // A TYPE_HOST device sorts on the CPU (std::stable_sort on the same order)
    int unique(const adl::Device* device, const adl::Buffer<int>& keys, adl::Buffer<int>& uniqueOut, adl::Buffer<u32>& countsOut, int n,
               bool descending = false);
    int unique(const adl::Device* device, const adl::Buffer<float>& keys, adl::Buffer<float>& uniqueOut, adl::Buffer<u32>& countsOut, int n,
               bool descending = false);
    int unique(const adl::Device* device, const adl::Buffer<long long>& keys, adl::Buffer<long long>& uniqueOut, adl::Buffer<u32>& countsOut, int n,
               bool descending = false);
    int unique(const adl::Device* device, const adl::Buffer<double>& keys, adl::Buffer<double>& uniqueOut, adl::Buffer<u32>& countsOut, int n,
               bool descending = false);
    int unique(const adl::Device* device, const adl::Buffer<u32>& keys, adl::Buffer<u32>& uniqueOut, adl::Buffer<u32>& countsOut, int n,
               bool descending = false);
    int unique(const adl::Device* device, const adl::Buffer<u64>& keys, adl::Buffer<u64>& uniqueOut, adl::Buffer<u32>& countsOut, int n,
               bool descending = false);

    // op (ADLHIP_REDUCE_SUM / _MIN / _MAX) over the values of every distinct key among the first n of keys: uniqueOut[r] in the order
    // of sortKeys(descending), reducedOut[r] the result for that key, r < R; both hold n elements, those at R and beyond are left alone.
    // K and V: int, float, long long, double, u32, u64, independently.  Integer sums wrap; float sums are IEEE adds in an unspecified
    // but reproducible association; min / max follow the ascending order of sortKeys (floats: totalOrder) whatever `descending` says,
    // and return the bits of an element.  keys and values are left intact.  Like unique this one WAITS and returns R.  A TYPE_HOST
    // device sorts on the CPU (std::stable_sort on the same order) and reduces in a loop
    template <typename K, typename V>
    int reduceByKey(const adl::Device* device, const adl::Buffer<K>& keys, const adl::Buffer<V>& values, adl::Buffer<K>& uniqueOut,
                    adl::Buffer<V>& reducedOut, int n, int op = ADLHIP_REDUCE_SUM, bool descending = false);

    // dst[i] = op (ADLHIP_REDUCE_SUM / _MIN / _MAX) over src[0 .. i] (exclusive: over src[0 .. i - 1]; dst[0] = the operator's identity
    // pattern: zero bits, the last / first pattern of V in the ascending order of sortKeys for MIN / MAX) for the first n elements.  V:
    // int, float, long long, double, u32, u64.  Integer sums wrap; float sums are IEEE adds in an unspecified but reproducible
    // association; min / max follow the order of sortKeys (floats: totalOrder) and return the bits of an element; the first element
    // comes back bit for bit.  dst may be src.  Enqueues and returns.  A TYPE_HOST device runs a plain loop, left to right
    template <typename V>
    void scanTyped(const adl::Device* device, const adl::Buffer<V>& src, adl::Buffer<V>& dst, int n, int op = ADLHIP_REDUCE_SUM,
                   bool exclusive = false);
    // scanTyped within every run of adjacent keys with identical bits (keys already grouped; A A B A is three runs): the scan starts
    // again at every run's first element.  K and V independently of the six types.  dst may be src, not keys
    template <typename K, typename V>
    void scanByKey(const adl::Device* device, const adl::Buffer<K>& keys, const adl::Buffer<V>& src, adl::Buffer<V>& dst, int n,
                   int op = ADLHIP_REDUCE_SUM, bool exclusive = false);

    // stream compaction: the elements i < n whose flag byte is non-zero, in input order, to itemsOut[0 .. S) and -- where indexOut is
    // given -- their positions to indexOut[0 .. S).  partition: a stable partition, the rejected elements follow in input order at
    // [S, n); without it nothing at S and beyond is written.  T: int, float, long long, double, u32, u64; items are copied bit for bit.
    // The outputs hold n elements.  items and flags are left intact.  Like unique this one WAITS and returns S.  A TYPE_HOST device
    // runs a plain loop
    template <typename T>
    int compactFlagged(const adl::Device* device, const adl::Buffer<T>& items, const adl::Buffer<unsigned char>& flags, adl::Buffer<T>& itemsOut,
                       adl::Buffer<u32>* indexOut, int n, bool partition = false);
    // the same for the elements with keys[i] cmp threshold (ADLHIP_CMP_LT .. ADLHIP_CMP_NE) in the ascending order of sortKeys: integers
    // by value, floats by totalOrder (NaNs are ordered, -0 is below +0); EQ / NE compare bits.  values / valuesOut (both or neither; V
    // independently of K) travel with their keys
    template <typename K, typename V>
    int compactIf(const adl::Device* device, const adl::Buffer<K>& keys, const adl::Buffer<V>* values, int cmp, K threshold,
                  adl::Buffer<K>& keysOut, adl::Buffer<V>* valuesOut, adl::Buffer<u32>* indexOut, int n, bool partition = false);
    template <typename K>
    int compactIf(const adl::Device* device, const adl::Buffer<K>& keys, int cmp, K threshold, adl::Buffer<K>& keysOut,
                  adl::Buffer<u32>* indexOut, int n, bool partition = false)
    {
        return compactIf<K, u32>(device, keys, (const adl::Buffer<u32>*)0, cmp, threshold, keysOut, (adl::Buffer<u32>*)0, indexOut, n, partition);
    }

    // histogram by edges: counts[b] = the keys i < n with edges[b] <= keys[i] < edges[b + 1] for b < numBins (at most
    // ADLHIP_HISTOGRAM_MAX_RANGE_BINS), in the ascending order of sortKeys: integers by value, floats by totalOrder (-0 below +0, NaNs
    // at the two ends).  edges holds numBins + 1 non-decreasing keys.  Keys outside the edges are ignored; includeUpper closes the
    // last bin as numpy.histogram does.  T: int, float, long long, double, u32, u64.  keys and edges are left intact.  Enqueues
    // and returns.  A TYPE_HOST device runs a plain loop
    template <typename T>
    void histogramRange(const adl::Device* device, const adl::Buffer<T>& keys, const adl::Buffer<T>& edges, adl::Buffer<u32>& counts, int n,
                        int numBins, bool includeUpper = false);
    // counts[v] = the keys i < n with value v for 0 <= v < numBins; negative keys and keys >= numBins are ignored.  T: int, long long,
    // u32, u64
    template <typename T>
    void binCount(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<u32>& counts, int n, int numBins);

    // merge of sorted sequences: the first na keys of keysA and the first nb keys of keysB, each sorted in the order of
    // sortKeys(descending), merged stably into keysOut[0 .. na + nb) -- what sortKeys gives for the concatenation, with one read and one
    // write per element.  Where keys are equal (same bits) those of keysA come first.  valuesA / valuesB / valuesOut (all or none; V
    // independently of K) travel with their keys; indexOut, where given, receives every output element's position in A || B (i for
    // A[i], na + i for B[i]).  K, V: int, float, long long, double, u32, u64.  The inputs are left intact and may be the same
    // Buffer; no output may be an input.  Inputs that are not sorted give an output in unspecified order.  Enqueues and returns.  A
    // TYPE_HOST device runs a plain two-pointer loop
    template <typename K, typename V>
    void mergePairs(const adl::Device* device, const adl::Buffer<K>& keysA, const adl::Buffer<V>* valuesA, const adl::Buffer<K>& keysB,
                    const adl::Buffer<V>* valuesB, adl::Buffer<K>& keysOut, adl::Buffer<V>* valuesOut, adl::Buffer<u32>* indexOut, int na, int nb,
                    bool descending = false);
    template <typename K>
    void mergeKeys(const adl::Device* device, const adl::Buffer<K>& keysA, const adl::Buffer<K>& keysB, adl::Buffer<K>& keysOut,
                   adl::Buffer<u32>* indexOut, int na, int nb, bool descending = false)
    {
        mergePairs<K, u32>(device, keysA, (const adl::Buffer<u32>*)0, keysB, (const adl::Buffer<u32>*)0, keysOut, (adl::Buffer<u32>*)0, indexOut, na,
                           nb, descending);
    }

    // set operations on sorted sequences: op = ADLHIP_SETOP_INTERSECTION / UNION / DIFFERENCE / SYMMETRIC_DIFFERENCE of the first na keys
    // of keysA and the first nb keys of keysB, each sorted in the order of sortKeys(descending), with thrust's multiset semantics: of
    // a key that occurs m times in A and n times in B the result holds min(m, n) copies (the first of A's), max(m, n) (A's, then the
    // last of B's), max(m - n, 0) (the last of A's) or |m - n| (the last of A's or of B's).  Keys are equal when their bits are.
    // Returns the number S of result elements (it waits for it): keysOut[0 .. S) in the order of mergeKeys, valuesOut[0 .. S) the kept
    // elements' own values (valuesA / valuesB / valuesOut: all or none), indexOut[0 .. S) their positions in A || B.  The outputs
    // hold na elements for intersection and difference, na + nb for the other two.  K, V: int, float, long long, double, u32, u64.
    // A TYPE_HOST device runs thrust's two-pointer loops
    template <typename K, typename V>
    int setOp(const adl::Device* device, int op, const adl::Buffer<K>& keysA, const adl::Buffer<V>* valuesA, const adl::Buffer<K>& keysB,
              const adl::Buffer<V>* valuesB, adl::Buffer<K>& keysOut, adl::Buffer<V>* valuesOut, adl::Buffer<u32>* indexOut, int na, int nb,
              bool descending = false);

    // sorted search: posOut[i], i < n = where needles[i] would be inserted among the first m keys of sortedKeys -- sorted in the order
    // of sortKeys(descending) -- to keep them sorted: the number of keys in front of the needle (right: in front of it or equal to it)
    // in that order, always in [0, m].  thrust lower_bound / upper_bound, numpy.searchsorted.  K: int, float, long long, double, u32,
    // u64; floats in totalOrder, equal means equal bits.  The inputs are left intact and may be the same Buffer; posOut may be
    // neither.  A sequence that is not sorted gives unspecified positions in [0, m].  Enqueues and returns.  A TYPE_HOST device runs a
    // plain binary search per needle
    template <typename K>
    void searchSorted(const adl::Device* device, const adl::Buffer<K>& sortedKeys, const adl::Buffer<K>& needles, adl::Buffer<u32>& posOut, int m,
                      int n, bool descending = false, bool right = false);

    // join of sorted sequences: kind = ADLHIP_JOIN_INNER / LEFT / SEMI / ANTI of the first na keys of keysA with the first nb keys of
    // keysB, each sorted in the order of sortKeys(descending), as pairs of positions: A[i] with m equal keys in B, the first at lo,
    // gives the rows (i, lo) .. (i, lo + m - 1) (INNER), the same or (i, ADLHIP_JOIN_NONE) where m is 0 (LEFT), (i, lo) once where
    // m > 0 (SEMI), (i, ADLHIP_JOIN_NONE) where m is 0 (ANTI), ordered by i, then by the position in B.  Keys are equal when their
    // bits are.  Returns the exact number T of rows (it waits for it), whatever cap is; rows below min(T, cap) are written to indexA
    // and indexB (cap elements each; either may be 0), nothing beyond.  cap = 0 without outputs only counts.  K: int, float, long
    // long, double, u32, u64.  The inputs are left intact and may be the same Buffer.  A TYPE_HOST device runs a two-pointer loop
    template <typename K>
    unsigned long long joinSorted(const adl::Device* device, int kind, const adl::Buffer<K>& keysA, const adl::Buffer<K>& keysB,
                                  adl::Buffer<u32>* indexA, adl::Buffer<u32>* indexB, int na, int nb, int cap, bool descending = false);

    // expansion of runs (run-length decode, the inverse of runLengthEncode): counts[i] rows for every run i < numRuns, in the order of
    // the runs; row o of run i, whose rows start at start[i] = counts[0] + .. + counts[i - 1], gets runOut[o] = i, rankOut[o] =
    // o - start[i] and valuesOut[o] = values[i].  Returns T, the sum of the counts (it waits for it), whatever cap is; rows below
    // min(T, cap) are written to whichever outputs are given (cap elements each), nothing beyond.  cap = 0 without outputs only
    // counts.  V: int, float, long long, double, u32, u64.  A TYPE_HOST device runs a loop over the runs
    template <typename V>
    unsigned long long expandRuns(const adl::Device* device, const adl::Buffer<u32>& counts, const adl::Buffer<V>* values, adl::Buffer<u32>* runOut,
                                  adl::Buffer<u32>* rankOut, adl::Buffer<V>* valuesOut, int numRuns, int cap);

    // sort along rows: every row of a rows x cols matrix sorted on its own, row r at element r * rowStride (0: cols), in the order of
    // sortKeys(descending) and stably: indexOut[r * cols + j] = column of the j-th element of row r, equal keys by ascending column in
    // both orders; keysOut[r * cols + j] = that key.  torch.sort(dim=-1, stable=True), cub::DeviceSegmentedSort on equal segments.  K:
    // int, float, long long, double, u32, u64.  keys is left intact; the outputs are dense rows x cols.  argsortRows writes the
    // columns alone.  Enqueues and returns.  A TYPE_HOST device runs a stable sort per row on the ordinals
    template <typename K>
    void sortRows(const adl::Device* device, const adl::Buffer<K>& keys, adl::Buffer<K>& keysOut, adl::Buffer<u32>& indexOut, int rows, int cols,
                  bool descending = false, int rowStride = 0);
    template <typename K>
    void argsortRows(const adl::Device* device, const adl::Buffer<K>& keys, adl::Buffer<u32>& indexOut, int rows, int cols, bool descending = false,
                     int rowStride = 0);

    // sort within segments: segment s < numSegments is elements [offsets[s], offsets[s + 1]) of the n keys (offsets: numSegments + 1
    // ascending entries, the first 0, the last n; empty segments may stand anywhere), sorted on its own in the order of
    // sortKeys(descending) and stably: indexOut[offsets[s] + j] = position inside the segment of its j-th element (plus offsets[s] with
    // globalIndex), equal keys by ascending position in both orders; keysOut[offsets[s] + j] = that key.  cub::DeviceSegmentedSort.
    // maxSegment: an upper bound on the longest segment, 0 = unknown (adlhip_sort_segments_typed chooses its path from it; a segment
    // longer than a bound of 4096 or less comes back in input order).  K: int, float, long long, double, u32, u64.  keys is left
    // intact.  argsortSegments writes the indices alone.  Enqueues and returns.  A TYPE_HOST device runs a stable sort per segment on
    // the ordinals, whatever maxSegment says
    template <typename K>
    void sortSegments(const adl::Device* device, const adl::Buffer<K>& keys, const adl::Buffer<u32>& offsets, adl::Buffer<K>& keysOut,
                      adl::Buffer<u32>& indexOut, int n, int numSegments, int maxSegment = 0, bool descending = false, bool globalIndex = false);
    template <typename K>
    void argsortSegments(const adl::Device* device, const adl::Buffer<K>& keys, const adl::Buffer<u32>& offsets, adl::Buffer<u32>& indexOut, int n,
                         int numSegments, int maxSegment = 0, bool descending = false, bool globalIndex = false);

private:
    template <typename T> void sortSegmentsTyped(const adl::Device* device, const adl::Buffer<T>& keys, const adl::Buffer<u32>& offsets,
                                                 adl::Buffer<T>* keysOut, adl::Buffer<u32>& indexOut, int n, int numSegments, int maxSegment,
                                                 bool descending, bool globalIndex);
    template <typename T> int uniqueTyped(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<T>& uniqueOut, adl::Buffer<u32>& countsOut,
                                          int n, bool descending);
    template <typename T> void sortRowsTyped(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<T>* keysOut, adl::Buffer<u32>& indexOut,
                                             int rows, int cols, bool descending, int rowStride);
    template <typename T> void topKRowsTyped(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<T>& keysOut, adl::Buffer<u32>& indexOut,
                                             int rows, int cols, int k, bool descending, int rowStride);
    template <typename T> void topKTyped(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<T>& keysOut, adl::Buffer<u32>& indexOut, int n,
                                         int k, bool descending);
    template <typename T> void sortKeysTyped(const adl::Device* device, const adl::Buffer<T>& inout, int n, bool descending);
    template <typename T> void argsortTyped(const adl::Device* device, const adl::Buffer<T>& keys, adl::Buffer<u32>& indexOut, int n, bool descending);
    // device scratch owned by the object and grown lazily (reference: m_u32WorkBuffer[0] = ping-pong data,
    // m_u32WorkBuffer[1] = histogram table; Pprims.h:44-45)
    void reserve(const adl::Device* device, size_t tmpBytes, size_t workBytes);
    void sortSoaWide(const adl::Device* device, void* keys, int keyBytes, void* values, int valueBytes, int n, int sortBits);
    adl::Buffer<unsigned char>* m_tmp;
    adl::Buffer<unsigned char>* m_work;
    bool m_cacheKernel;
};

}  // namespace Tahoe
