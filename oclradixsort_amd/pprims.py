"""Python mirror of `Tahoe::Pprims` (Tahoe/ParallelPrimitives/Pprims.h:11-48) over the HIP back-end.

    p = Pprims()
    p.radixSort(device, buffer_u32, n, sortBits=32)        # Pprims.h:41
    p.radixSort(device, buffer_uint2, n, sortBits=32)      # Pprims.h:38  (dtype uint64 = {key, value})
    p.radixSort64(device, buffer_u64, n, sortBits=64)      # 64-bit keys (no reference counterpart)
    p.scan(device, dst, src, n, sumOut=None)               # Pprims.h:35
    p.sortKeys(device, buffer, n, descending=False)        # uint32 / int32 / float32 / uint64 / int64 / float64 keys
    p.sortPairs(device, keys, values, n, descending=False) # the same keys with values of 4, 8 or 16 bytes, stable
    p.argsort(device, keys, n, descending=False)           # -> Buffer(uint32): the stable sorting permutation
    p.topk(device, keys, n, k, descending=False)           # -> Buffer(uint32): its first k entries, by selection
    p.topkRows(device, keys, rows, cols, k)                # -> Buffer(uint32): rows x k columns, top-k of every row
    p.sortRows(device, keys, rows, cols, keysOut=out)      # -> Buffer(uint32): rows x cols columns, the stable argsort of every row
    p.sortSegments(device, keys, offsets, S, maxSegment=m) # -> Buffer(uint32): the stable argsort of every segment [offsets[s], offsets[s+1])
    p.unique(device, keys, n, counts=True, inverse=True)   # -> UniqueResult: distinct keys in sorted order, counts, inverse, ...
    p.runLengthEncode(device, keys, n, counts=True)        # -> UniqueResult: the runs of keys that are already grouped
    p.reduceByKey(device, keys, values, n, op="sum")       # -> ReduceResult: distinct keys in sorted order, sum / min / max of their values
    p.reduceRuns(device, keys, values, n, op="sum")        # -> ReduceResult: the same per run of keys that are already grouped
    p.scanTyped(device, dst, src, n, op="sum")             # inclusive / exclusive prefix sum, min or max of typed values
    p.scanByKey(device, keys, dst, src, n, op="sum")       # the same within every run of keys that are already grouped
    p.compactFlagged(device, flags, n, items=buf)          # -> CompactResult: the items whose flag byte is non-zero, in input order
    p.compactIf(device, keys, n, "lt", x, values=buf)      # -> CompactResult: the keys (and their values) that compare so with x
    p.histogramRange(device, keys, n, edges, num_bins)     # -> Buffer(uint32): the keys per bin [edges[b], edges[b + 1])
    p.binCount(device, keys, n, num_bins)                  # -> Buffer(uint32): the keys per value 0 .. num_bins - 1
    p.mergeKeys(device, a, b, out, na, nb)                 # the stable merge of two sorted key Buffers (mergePairs: with values)
    p.setOp(device, "intersection", a, b, out, na, nb)     # -> SetOpResult: also "union", "difference", "symmetric_difference"
    p.searchSorted(device, sortedKeys, needles, posOut, m, n)   # every needle's lower (right=True: upper) bound in m sorted keys
    p.joinSorted(device, "inner", a, b, na, nb, cap=c, indexA=True, indexB=True)   # -> JoinResult: also "left", "semi", "anti"
    p.expandRuns(device, counts, numRuns, cap=c, runOut=True)   # -> ExpandResult: run-length decode, repeat_interleave

Like the reference object it owns lazily grown device scratch (m_u32WorkBuffer[0] = ping-pong data
buffer, m_u32WorkBuffer[1] = histogram table; Pprims.h:44-45, Pprims.cpp:226-232, :332-337) and must be
destroyed (close()) before DeviceUtils.deallocate, which refuses while memory is live (Adl.inl:102).
Calls enqueue and return without synchronising, as the reference's GPU branches do.
"""
import collections
import ctypes

import numpy as np

from . import _lib
from ._lib import AdlHipError, check
from .adl import Buffer

ELEM_U32 = 0
ELEM_KV32 = 1
ELEM_U64 = 2
ELEM_SOA32 = 3

# ADLHIP_KEY_* by element type (include/adlhip.h, "typed keys, order, argsort")
KEY_TYPES = {np.dtype(np.uint32): 0, np.dtype(np.int32): 1, np.dtype(np.float32): 2,
             np.dtype(np.uint64): 3, np.dtype(np.int64): 4, np.dtype(np.float64): 5}

# What unique / runLengthEncode return: device Buffers (None where not asked).  `count` is a one-element uint32 Buffer that holds R, the
# number of runs; unique, counts and firstIndex have n elements of which the first R are written, offsets n + 1 (R + 1 written), inverse n.
UniqueResult = collections.namedtuple("UniqueResult", "unique counts offsets firstIndex inverse count")

# ADLHIP_REDUCE_* by name (include/adlhip.h, "reduce values by key")
REDUCE_OPS = {"sum": 0, "min": 1, "max": 2}

# What reduceByKey / reduceRuns return: device Buffers (None where not asked).  `count` is a one-element uint32 Buffer that holds R;
# unique, reduced and counts have n elements of which the first R are written, offsets n + 1 (R + 1 written).
ReduceResult = collections.namedtuple("ReduceResult", "unique reduced counts offsets count")

# ADLHIP_CMP_* by name (include/adlhip.h, "stream compaction")
CMP_OPS = {"lt": 0, "le": 1, "gt": 2, "ge": 3, "eq": 4, "ne": 5, "<": 0, "<=": 1, ">": 2, ">=": 3, "==": 4, "!=": 5}

# What compactFlagged / compactIf return: device Buffers (None where not asked).  `count` is a one-element uint32 Buffer that holds S,
# the number of selected elements; items (compactIf: the keys), values and index have n elements of which the first S are written --
# all n with partition=True, the rejected elements behind the selected ones.
CompactResult = collections.namedtuple("CompactResult", "items values index count")

# ADLHIP_SETOP_* (include/adlhip.h, "set operations on sorted sequences")
SET_OPS = {"intersection": 0, "union": 1, "difference": 2, "symmetric_difference": 3}

# What setOp returns: device Buffers (None where not asked).  `count` is a one-element uint32 Buffer that holds S, the number of result
# elements; keys, values and index hold na (intersection, difference) or na + nb elements, of which the first S are written.
SetOpResult = collections.namedtuple("SetOpResult", "keys values index count")

# ADLHIP_JOIN_* (include/adlhip.h, "expansion of runs and join of sorted sequences"); JOIN_NONE stands for "no match" in indexB
JOIN_KINDS = {"inner": 0, "left": 1, "semi": 2, "anti": 3}
JOIN_NONE = 0xFFFFFFFF
JOIN_MAX_ELEMS = 0xFFF00000

# What joinSorted returns: device Buffers (None where not asked).  `count` is a one-element uint64 Buffer that holds T, the exact number
# of rows, whatever cap was; indexA and indexB hold cap elements, of which the first min(T, cap) are written.
JoinResult = collections.namedtuple("JoinResult", "indexA indexB count")

# What expandRuns returns: the same for run, rank and values.
ExpandResult = collections.namedtuple("ExpandResult", "run rank values count")

# ADLHIP_HISTOGRAM_MAX_RANGE_BINS and ADLHIP_HISTOGRAM_TILE (include/adlhip.h, "histograms"): the most bins histogramRange takes, and
# the elements of a tile of its count kernel (tests place their sizes around it)
HISTOGRAM_MAX_RANGE_BINS = 4096
HISTOGRAM_TILE = 2048


class Pprims:
    SCAN_BLOCK_SIZE = 128               # Pprims.h:24 (kept for API parity; unused by the HIP kernels)
    R32SORT_DATA_ALIGNMENT = 256        # Pprims.h:28: the reference needs n % 256 == 0; this build does not
    R32SORT_WG_SIZE = 64                # Pprims.h:29
    R32SORT_BITS_PER_PASS = 4           # Pprims.h:31: available via device.setParam("sort.digit_bits", 4)

    def __init__(self):
        self.m_tmp = None       # m_u32WorkBuffer[0]
        self.m_work = None      # m_u32WorkBuffer[1]
        self.m_cacheKernel = True
        self._sum_keep = None

    def cacheKernel(self, cache):   # Pprims.h:20 -- kernels are compiled ahead of time; nothing to cache
        self.m_cacheKernel = bool(cache)

    def close(self):
        for b in (self.m_tmp, self.m_work):
            if b is not None:
                b.release()
        self.m_tmp = self.m_work = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- scratch (uArray::setSize semantics: grow-only, contents not preserved)
    def _scratch(self, device, tmp_bytes, work_bytes):
        if self.m_tmp is None or self.m_tmp.m_device is not device:
            self.close()
            self.m_tmp = Buffer(device, 0, np.uint8)
            self.m_work = Buffer(device, 0, np.uint8)
        if self.m_tmp.getSize() < tmp_bytes:
            self.m_tmp.setSize(tmp_bytes)
        if self.m_work.getSize() < work_bytes:
            self.m_work.setSize(work_bytes)

    def reserve(self, device, kind, n):
        """Size the scratch for sorts of up to n elements of `kind` now, so that later calls do not grow it
        (growing syncs the device and reallocates, uArray.h:124-132)."""
        tb = ctypes.c_size_t()
        wb = ctypes.c_size_t()
        check(_lib.load().adlhip_radix_sort_scratch_bytes(device._h, kind, int(n), ctypes.byref(tb), ctypes.byref(wb)),
              "adlhip_radix_sort_scratch_bytes")
        self._scratch(device, (2 if kind == ELEM_SOA32 else 1) * tb.value, wb.value)

    def _sort(self, device, kind, fn, inout, n, sortBits):
        if device is None:
            raise AdlHipError("radixSort needs a device (the Python mirror has no host fallback)")
        n = int(n)
        lib = _lib.load()
        tb = ctypes.c_size_t()
        wb = ctypes.c_size_t()
        # full-speed scratch for a sort on these bits (level 1; a sort on fewer bits than the key has needs more)
        check(lib.adlhip_radix_sort_scratch_bytes_for(device._h, kind, n, int(sortBits), 1, ctypes.byref(tb), ctypes.byref(wb)),
              "adlhip_radix_sort_scratch_bytes_for")
        self._scratch(device, tb.value, wb.value)
        check(fn(device._h, inout.ptr(), self.m_tmp.ptr(), self.m_work.ptr(), self.m_work.getSize(), n, int(sortBits)),
              "radixSort")

    def radixSort(self, device, inout, n, sortBits=32):
        """u32 keys (dtype uint32) or {u32 key, u32 value} pairs (dtype uint64, key in the low dword)."""
        lib = _lib.load()
        if inout.dtype == np.uint32:
            self._sort(device, ELEM_U32, lib.adlhip_radix_sort_u32, inout, n, sortBits)
        elif inout.dtype == np.uint64:
            self._sort(device, ELEM_KV32, lib.adlhip_radix_sort_kv32, inout, n, sortBits)
        else:
            raise AdlHipError("radixSort: unsupported element type %s" % inout.dtype)

    def radixSortSoA(self, device, keys, values, n, sortBits=None):
        """Key-value sort on separate key and value buffers (structure of arrays): ascending by key,
        stable, values follow their keys.  Same contract as radixSort on {key, value} pairs.  Keys: uint32 or
        uint64; values: any element type of 4, 8 or 16 bytes (u32 + u32 is the reference kernel's own layout,
        RadixSortKeyValueKernels.cl:354-509)."""
        kb, vb = keys.dtype.itemsize, values.dtype.itemsize
        if keys.dtype not in (np.uint32, np.uint64) or vb not in (4, 8, 16):
            raise AdlHipError("radixSortSoA: keys %s / values %s unsupported" % (keys.dtype, values.dtype))
        if sortBits is None:
            sortBits = 8 * kb
        if device is None:
            raise AdlHipError("radixSortSoA needs a device")
        n = int(n)
        lib = _lib.load()
        tk = ctypes.c_size_t()
        tv = ctypes.c_size_t()
        wb = ctypes.c_size_t()
        check(lib.adlhip_radix_sort_soa_scratch_bytes(device._h, kb, vb, n, int(sortBits), ctypes.byref(tk), ctypes.byref(tv),
                                                      ctypes.byref(wb)), "adlhip_radix_sort_soa_scratch_bytes")
        self._scratch(device, tk.value + tv.value, wb.value)          # tmp keys + tmp values, back to back
        tmp_k = self.m_tmp.ptr()
        tmp_v = ctypes.c_void_p(self.m_tmp.m_ptr + tk.value) if self.m_tmp.m_ptr else None
        check(lib.adlhip_radix_sort_soa(device._h, keys.ptr(), kb, values.ptr(), vb, tmp_k, tmp_v, self.m_work.ptr(),
                                        self.m_work.getSize(), n, int(sortBits)), "radixSortSoA")

    def radixSort64(self, device, inout, n, sortBits=64):
        assert inout.dtype == np.uint64
        self._sort(device, ELEM_U64, _lib.load().adlhip_radix_sort_u64, inout, n, sortBits)

    # -- typed keys, order, argsort (no reference counterpart; include/adlhip.h adlhip_sort_*_typed)
    @staticmethod
    def _key_type(buf, what):
        kt = KEY_TYPES.get(np.dtype(buf.dtype))
        if kt is None:
            raise AdlHipError("%s: unsupported key type %s (uint32, int32, float32, uint64, int64, float64)" % (what, buf.dtype))
        return kt

    def _typed_scratch(self, device, key_type, mode, value_bytes, n):
        tk = ctypes.c_size_t()
        tv = ctypes.c_size_t()
        wb = ctypes.c_size_t()
        check(_lib.load().adlhip_sort_typed_scratch_bytes(device._h, key_type, mode, value_bytes, n, ctypes.byref(tk),
                                                          ctypes.byref(tv), ctypes.byref(wb)), "adlhip_sort_typed_scratch_bytes")
        self._scratch(device, tk.value + tv.value, wb.value)          # tmp keys + tmp values, back to back
        return tk.value

    def sortKeys(self, device, buf, n, descending=False):
        """Sorts n keys of buf.dtype in place: signed integers by value, floats in IEEE-754 totalOrder (-NaN < -inf < ... < -0 <
        +0 < ... < +inf < +NaN), ascending or descending.  Two streaming sweeps (encode, decode) around the unsigned sort."""
        if device is None:
            raise AdlHipError("sortKeys needs a device")
        kt = self._key_type(buf, "sortKeys")
        n = int(n)
        self._typed_scratch(device, kt, 0, 0, n)
        check(_lib.load().adlhip_sort_keys_typed(device._h, kt, 1 if descending else 0, buf.ptr(), self.m_tmp.ptr(),
                                                 self.m_work.ptr(), self.m_work.getSize(), n), "sortKeys")

    def sortPairs(self, device, keys, values, n, descending=False):
        """Sorts n typed keys and their values (any element type of 4, 8 or 16 bytes) in place, stably: equal keys keep their
        input order, descending too.  Key order as sortKeys."""
        if device is None:
            raise AdlHipError("sortPairs needs a device")
        kt = self._key_type(keys, "sortPairs")
        vb = values.dtype.itemsize
        if vb not in (4, 8, 16):
            raise AdlHipError("sortPairs: values %s unsupported (4, 8 or 16 bytes)" % values.dtype)
        n = int(n)
        tk = self._typed_scratch(device, kt, 1, vb, n)
        tmp_k = self.m_tmp.ptr() if tk else None
        tmp_v = ctypes.c_void_p(self.m_tmp.m_ptr + tk) if self.m_tmp.m_ptr else None
        check(_lib.load().adlhip_sort_pairs_typed(device._h, kt, 1 if descending else 0, keys.ptr(), values.ptr(), vb, tmp_k, tmp_v,
                                                  self.m_work.ptr(), self.m_work.getSize(), n), "sortPairs")

    def argsort(self, device, keys, n, descending=False, keysOut=None, indexOut=None):
        """Returns a Buffer(uint32) with the stable sorting permutation of the first n keys: out[j] = position in `keys` of the
        j-th element of the sorted order.  `keys` is left intact; keysOut (same dtype, not `keys`) receives the sorted keys.
        indexOut: a uint32 buffer of n elements to fill and return instead of a new one."""
        if device is None:
            raise AdlHipError("argsort needs a device")
        kt = self._key_type(keys, "argsort")
        if keysOut is not None and np.dtype(keysOut.dtype) != np.dtype(keys.dtype):
            raise AdlHipError("argsort: keysOut is %s, keys are %s" % (keysOut.dtype, keys.dtype))
        if indexOut is not None and (np.dtype(indexOut.dtype) != np.uint32 or indexOut.getSize() < int(n)):
            raise AdlHipError("argsort: indexOut must hold n uint32 elements")
        n = int(n)
        self._typed_scratch(device, kt, 2, 0, n)
        out = indexOut if indexOut is not None else Buffer(device, n, np.uint32)
        try:
            check(_lib.load().adlhip_argsort_typed(device._h, kt, 1 if descending else 0, keys.ptr(),
                                                   keysOut.ptr() if keysOut is not None else None, out.ptr(), self.m_work.ptr(),
                                                   self.m_work.getSize(), n), "argsort")
        except AdlHipError:
            if indexOut is None:
                out.release()
            raise
        return out

    def topk(self, device, keys, n, k, descending=False, keysOut=None, indexOut=None):
        """Returns a Buffer(uint32) with the first k entries of argsort(device, keys, n, descending): the positions of the k smallest
        (descending: largest) of the first n keys, sorted, ties by ascending position.  `keys` is left intact; keysOut (same dtype,
        k elements, not `keys`) receives the k keys.  indexOut: a uint32 buffer of k elements to fill and return instead of a new one."""
        if device is None:
            raise AdlHipError("topk needs a device")
        kt = self._key_type(keys, "topk")
        n, k = int(n), int(k)
        if k < 0 or k > n:
            raise AdlHipError("topk: k = %d outside [0, n = %d]" % (k, n))
        if keysOut is not None and (np.dtype(keysOut.dtype) != np.dtype(keys.dtype) or keysOut.getSize() < k):
            raise AdlHipError("topk: keysOut must hold k elements of %s" % keys.dtype)
        if indexOut is not None and (np.dtype(indexOut.dtype) != np.uint32 or indexOut.getSize() < k):
            raise AdlHipError("topk: indexOut must hold k uint32 elements")
        wb = ctypes.c_size_t()
        check(_lib.load().adlhip_topk_scratch_bytes(device._h, kt, n, k, ctypes.byref(wb)), "adlhip_topk_scratch_bytes")
        self._scratch(device, 0, wb.value)
        out = indexOut if indexOut is not None else Buffer(device, k, np.uint32)
        try:
            check(_lib.load().adlhip_topk_typed(device._h, kt, 1 if descending else 0, keys.ptr(), n, k,
                                                keysOut.ptr() if keysOut is not None else None, out.ptr(), self.m_work.ptr(),
                                                self.m_work.getSize()), "topk")
        except AdlHipError:
            if indexOut is None:
                out.release()
            raise
        return out

    def topkRows(self, device, keys, rows, cols, k, descending=False, keysOut=None, indexOut=None, rowStride=None):
        """Top-k along the rows of a rows x cols matrix (row r starts at element r * rowStride; default cols): returns a
        Buffer(uint32) of rows * k columns, row-major -- per row the first k entries of the row's own argsort, ties by ascending
        column.  `keys` is left intact; keysOut (same dtype, rows * k elements, not `keys`) receives the keys.  indexOut: a uint32
        buffer of rows * k elements to fill and return instead of a new one."""
        if device is None:
            raise AdlHipError("topkRows needs a device")
        kt = self._key_type(keys, "topkRows")
        rows, cols, k = int(rows), int(cols), int(k)
        stride = cols if rowStride is None else int(rowStride)
        if rows < 0 or cols < 0:
            raise AdlHipError("topkRows: rows = %d, cols = %d" % (rows, cols))
        if k < 0 or k > cols:
            raise AdlHipError("topkRows: k = %d outside [0, cols = %d]" % (k, cols))
        if stride < cols:
            raise AdlHipError("topkRows: rowStride = %d is below cols = %d" % (stride, cols))
        if rows and keys.getSize() < (rows - 1) * stride + cols:
            raise AdlHipError("topkRows: keys must hold (rows - 1) * rowStride + cols = %d elements" % ((rows - 1) * stride + cols))
        if keysOut is not None and (np.dtype(keysOut.dtype) != np.dtype(keys.dtype) or keysOut.getSize() < rows * k):
            raise AdlHipError("topkRows: keysOut must hold rows * k elements of %s" % keys.dtype)
        if indexOut is not None and (np.dtype(indexOut.dtype) != np.uint32 or indexOut.getSize() < rows * k):
            raise AdlHipError("topkRows: indexOut must hold rows * k uint32 elements")
        wb = ctypes.c_size_t()
        check(_lib.load().adlhip_topk_rows_scratch_bytes(device._h, kt, rows, cols, k, ctypes.byref(wb)), "adlhip_topk_rows_scratch_bytes")
        self._scratch(device, 0, wb.value)
        out = indexOut if indexOut is not None else Buffer(device, rows * k, np.uint32)
        try:
            check(_lib.load().adlhip_topk_rows_typed(device._h, kt, 1 if descending else 0, keys.ptr(), rows, cols, stride, k,
                                                     keysOut.ptr() if keysOut is not None else None, out.ptr(), self.m_work.ptr(),
                                                     self.m_work.getSize()), "topkRows")
        except AdlHipError:
            if indexOut is None:
                out.release()
            raise
        return out

    def sortRows(self, device, keys, rows, cols, descending=False, keysOut=None, indexOut=None, rowStride=None):
        """Sort and argsort along the rows of a rows x cols matrix (row r starts at element r * rowStride; default cols): returns a
        Buffer(uint32) of rows * cols columns, row-major -- per row the row's own stable argsort, ties by ascending column in both
        orders.  `keys` is left intact; keysOut (same dtype, rows * cols elements, not `keys`) receives the sorted rows.  indexOut: a
        uint32 buffer of rows * cols elements to fill and return instead of a new one.  Key order as sortKeys."""
        if device is None:
            raise AdlHipError("sortRows needs a device")
        kt = self._key_type(keys, "sortRows")
        rows, cols = int(rows), int(cols)
        stride = cols if rowStride is None else int(rowStride)
        if rows < 0 or cols < 0:
            raise AdlHipError("sortRows: rows = %d, cols = %d" % (rows, cols))
        if rows * cols >= 1 << 32:
            raise AdlHipError("sortRows: rows * cols = %d, fewer than 2^32 elements" % (rows * cols))
        if stride < cols:
            raise AdlHipError("sortRows: rowStride = %d is below cols = %d" % (stride, cols))
        if rows and cols and keys.getSize() < (rows - 1) * stride + cols:
            raise AdlHipError("sortRows: keys must hold (rows - 1) * rowStride + cols = %d elements" % ((rows - 1) * stride + cols))
        if keysOut is not None and (np.dtype(keysOut.dtype) != np.dtype(keys.dtype) or keysOut.getSize() < rows * cols):
            raise AdlHipError("sortRows: keysOut must hold rows * cols elements of %s" % keys.dtype)
        if indexOut is not None and (np.dtype(indexOut.dtype) != np.uint32 or indexOut.getSize() < rows * cols):
            raise AdlHipError("sortRows: indexOut must hold rows * cols uint32 elements")
        wb = ctypes.c_size_t()
        check(_lib.load().adlhip_sort_rows_scratch_bytes(device._h, kt, rows, cols, ctypes.byref(wb)), "adlhip_sort_rows_scratch_bytes")
        self._scratch(device, 0, wb.value)
        out = indexOut if indexOut is not None else Buffer(device, rows * cols, np.uint32)
        try:
            check(_lib.load().adlhip_sort_rows_typed(device._h, kt, 1 if descending else 0, keys.ptr(), rows, cols, stride,
                                                     keysOut.ptr() if keysOut is not None else None, out.ptr(), self.m_work.ptr(),
                                                     self.m_work.getSize()), "sortRows")
        except AdlHipError:
            if indexOut is None:
                out.release()
            raise
        return out

    def sortSegments(self, device, keys, offsets, numSegments, maxSegment=0, descending=False, keysOut=None, indexOut=None,
                     globalIndex=False, oversizedOut=None):
        """Sort and argsort within segments: segment s is elements [offsets[s], offsets[s + 1]) of `keys`, n = keys.getSize().
        Returns a Buffer(uint32) of n indices -- per segment the segment's own stable argsort, ties by ascending position in both
        orders; the position inside the segment, or in `keys` with globalIndex.  offsets: a uint32 buffer of numSegments + 1 ascending
        offsets, the first 0, the last n; empty segments may stand anywhere.  maxSegment: an upper bound on the longest segment (0:
        unknown); up to 4096 the segment kernel runs, otherwise the flat path.  A segment longer than a bound of 4096 or less comes
        back in input order and is counted in oversizedOut (a uint32 buffer of one element, always written when given).  `keys` is
        left intact; keysOut (same dtype, n elements, not `keys`) receives the sorted segments.  indexOut: a uint32 buffer of n
        elements to fill and return instead of a new one.  Key order as sortKeys."""
        if device is None:
            raise AdlHipError("sortSegments needs a device")
        kt = self._key_type(keys, "sortSegments")
        n, S, bound = int(keys.getSize()), int(numSegments), int(maxSegment)
        if S < 0 or bound < 0:
            raise AdlHipError("sortSegments: numSegments = %d, maxSegment = %d" % (S, bound))
        if n >= 1 << 32:
            raise AdlHipError("sortSegments: n = %d, fewer than 2^32 elements" % n)
        if np.dtype(offsets.dtype) != np.uint32 or offsets.getSize() < S + 1:
            raise AdlHipError("sortSegments: offsets must hold numSegments + 1 = %d uint32 elements" % (S + 1))
        if keysOut is not None and (np.dtype(keysOut.dtype) != np.dtype(keys.dtype) or keysOut.getSize() < n):
            raise AdlHipError("sortSegments: keysOut must hold n = %d elements of %s" % (n, keys.dtype))
        if indexOut is not None and (np.dtype(indexOut.dtype) != np.uint32 or indexOut.getSize() < n):
            raise AdlHipError("sortSegments: indexOut must hold n = %d uint32 elements" % n)
        if oversizedOut is not None and (np.dtype(oversizedOut.dtype) != np.uint32 or oversizedOut.getSize() < 1):
            raise AdlHipError("sortSegments: oversizedOut must hold one uint32 element")
        wb = ctypes.c_size_t()
        check(_lib.load().adlhip_sort_segments_scratch_bytes(device._h, kt, n, S, bound, ctypes.byref(wb)),
              "adlhip_sort_segments_scratch_bytes")
        self._scratch(device, 0, wb.value)
        out = indexOut if indexOut is not None else Buffer(device, n, np.uint32)
        try:
            check(_lib.load().adlhip_sort_segments_typed(device._h, kt, 1 if descending else 0, keys.ptr(), n, offsets.ptr(), S, bound,
                                                         1 if globalIndex else 0, keysOut.ptr() if keysOut is not None else None,
                                                         out.ptr(), oversizedOut.ptr() if oversizedOut is not None else None,
                                                         self.m_work.ptr(), self.m_work.getSize()), "sortSegments")
        except AdlHipError:
            if indexOut is None:
                out.release()
            raise
        return out

    # -- unique keys, run lengths, inverse indices (no reference counterpart; include/adlhip.h adlhip_unique_typed)
    @staticmethod
    def _runs_outputs(what, device, n, asked):
        """asked: [(name, value, elements)], value False / None (not asked), True (a new uint32 Buffer) or a uint32 Buffer of at least
        `elements` elements to fill.  Checks every value first -- nothing is allocated when one is refused -- then returns the Buffers
        (None where not asked) and the ones that were allocated here."""
        for name, v, elems in asked:
            if v is None or v is False or v is True:
                continue
            if not hasattr(v, "getSize") or np.dtype(v.dtype) != np.uint32 or v.getSize() < elems:
                raise AdlHipError("%s: %s must be True or a uint32 buffer of %d elements" % (what, name, elems))
        out, own = [], []
        for name, v, elems in asked:
            if v is True:
                v = Buffer(device, elems, np.uint32)
                own.append(v)
            out.append(v if v is not None and v is not False else None)
        return out, own

    def unique(self, device, keys, n, descending=False, counts=False, offsets=False, firstIndex=False, inverse=False,
               uniqueOut=None, countOut=None):
        """The distinct keys among the first n of `keys` in the order of sortKeys(descending) -> UniqueResult.  Keys are equal when
        their bits are: -0 and +0 are two keys, NaNs with different payloads too.  With R distinct keys (result.count, on the device):
        unique[r] the r-th key, counts[r] how often it occurs, offsets[r] where its run starts in the sorted order (offsets[R] = n),
        firstIndex[r] the lowest position in `keys` that holds it, inverse[i] the r of keys[i].  counts / offsets / firstIndex /
        inverse: True for a new uint32 Buffer, or a uint32 Buffer to fill (n elements; offsets n + 1).  uniqueOut (keys' dtype, n
        elements) and countOut (uint32, 1 element) likewise replace the Buffers allocated here.  `keys` is left intact.  Enqueues and
        returns; read result.count (toHost) to learn R."""
        if device is None:
            raise AdlHipError("unique needs a device")
        kt = self._key_type(keys, "unique")
        n = int(n)
        if n < 0 or keys.getSize() < n:
            raise AdlHipError("unique: n = %d outside [0, %d]" % (n, keys.getSize()))
        if uniqueOut is not None and (np.dtype(uniqueOut.dtype) != np.dtype(keys.dtype) or uniqueOut.getSize() < n):
            raise AdlHipError("unique: uniqueOut must hold n elements of %s" % keys.dtype)
        if countOut is not None and (np.dtype(countOut.dtype) != np.uint32 or countOut.getSize() < 1):
            raise AdlHipError("unique: countOut must hold one uint32 element")
        (c, o, f, i), own = self._runs_outputs("unique", device, n, [("counts", counts, n), ("offsets", offsets, n + 1),
                                                                     ("firstIndex", firstIndex, n), ("inverse", inverse, n)])
        try:
            lib = _lib.load()
            wb = ctypes.c_size_t()
            want_index = 1 if (f is not None or i is not None or device.getParam("unique.algo") == 1) else 0
            check(lib.adlhip_unique_scratch_bytes(device._h, kt, n, want_index, ctypes.byref(wb)), "adlhip_unique_scratch_bytes")
            self._scratch(device, 0, wb.value)
            if uniqueOut is None:
                uniqueOut = Buffer(device, n, keys.dtype)
                own.append(uniqueOut)
            if countOut is None:
                countOut = Buffer(device, 1, np.uint32)
                own.append(countOut)

            def p(b):
                return b.ptr() if b is not None else None
            check(lib.adlhip_unique_typed(device._h, kt, 1 if descending else 0, keys.ptr(), n, uniqueOut.ptr(), p(c), p(o), p(f), p(i),
                                          countOut.ptr(), self.m_work.ptr(), self.m_work.getSize()), "unique")
        except AdlHipError:
            for b in own:
                b.release()
            raise
        return UniqueResult(uniqueOut, c, o, f, i, countOut)

    def runLengthEncode(self, device, keys, n, counts=False, offsets=False, uniqueOut=None, countOut=None):
        """The runs (maximal stretches of adjacent keys with identical bits) of the first n of `keys`, which are already grouped; any
        element type of 4 or 8 bytes -> UniqueResult (firstIndex and inverse are None).  With R runs (result.count): unique[r] the
        key of run r, offsets[r] its first position (offsets[R] = n), counts[r] its length.  Buffers as in unique()."""
        if device is None:
            raise AdlHipError("runLengthEncode needs a device")
        kb = np.dtype(keys.dtype).itemsize
        if kb not in (4, 8):
            raise AdlHipError("runLengthEncode: unsupported key type %s (4 or 8 bytes)" % keys.dtype)
        n = int(n)
        if n < 0 or keys.getSize() < n:
            raise AdlHipError("runLengthEncode: n = %d outside [0, %d]" % (n, keys.getSize()))
        if uniqueOut is not None and (np.dtype(uniqueOut.dtype) != np.dtype(keys.dtype) or uniqueOut.getSize() < n):
            raise AdlHipError("runLengthEncode: uniqueOut must hold n elements of %s" % keys.dtype)
        if countOut is not None and (np.dtype(countOut.dtype) != np.uint32 or countOut.getSize() < 1):
            raise AdlHipError("runLengthEncode: countOut must hold one uint32 element")
        (c, o), own = self._runs_outputs("runLengthEncode", device, n, [("counts", counts, n), ("offsets", offsets, n + 1)])
        try:
            lib = _lib.load()
            wb = ctypes.c_size_t()
            check(lib.adlhip_run_length_encode_scratch_bytes(device._h, kb, n, ctypes.byref(wb)), "adlhip_run_length_encode_scratch_bytes")
            self._scratch(device, 0, wb.value)
            if uniqueOut is None:
                uniqueOut = Buffer(device, n, keys.dtype)
                own.append(uniqueOut)
            if countOut is None:
                countOut = Buffer(device, 1, np.uint32)
                own.append(countOut)
            check(lib.adlhip_run_length_encode(device._h, kb, keys.ptr(), n, uniqueOut.ptr(), c.ptr() if c is not None else None,
                                               o.ptr() if o is not None else None, countOut.ptr(), self.m_work.ptr(),
                                               self.m_work.getSize()), "runLengthEncode")
        except AdlHipError:
            for b in own:
                b.release()
            raise
        return UniqueResult(uniqueOut, c, o, None, None, countOut)

    # -- reduce values by key (no reference counterpart; include/adlhip.h adlhip_reduce_by_key_typed)
    def _reduce(self, what, device, by_key, keys, values, n, op, descending, counts, offsets, uniqueOut, reducedOut, countOut):
        if device is None:
            raise AdlHipError("%s needs a device" % what)
        if op not in REDUCE_OPS:
            raise AdlHipError("%s: op must be 'sum', 'min' or 'max', got %r" % (what, op))
        if by_key:
            kt = self._key_type(keys, what)
        elif np.dtype(keys.dtype).itemsize not in (4, 8):
            raise AdlHipError("%s: unsupported key type %s (4 or 8 bytes)" % (what, keys.dtype))
        vt = KEY_TYPES.get(np.dtype(values.dtype))
        if vt is None:
            raise AdlHipError("%s: unsupported value type %s (uint32, int32, float32, uint64, int64, float64)" % (what, values.dtype))
        n = int(n)
        if n < 0 or keys.getSize() < n or values.getSize() < n:
            raise AdlHipError("%s: n = %d outside [0, %d]" % (what, n, min(keys.getSize(), values.getSize())))
        if uniqueOut is not None and (np.dtype(uniqueOut.dtype) != np.dtype(keys.dtype) or uniqueOut.getSize() < n):
            raise AdlHipError("%s: uniqueOut must hold n elements of %s" % (what, keys.dtype))
        if reducedOut is not None and (np.dtype(reducedOut.dtype) != np.dtype(values.dtype) or reducedOut.getSize() < n):
            raise AdlHipError("%s: reducedOut must hold n elements of %s" % (what, values.dtype))
        if countOut is not None and (np.dtype(countOut.dtype) != np.uint32 or countOut.getSize() < 1):
            raise AdlHipError("%s: countOut must hold one uint32 element" % what)
        (c, o), own = self._runs_outputs(what, device, n, [("counts", counts, n), ("offsets", offsets, n + 1)])
        try:
            lib = _lib.load()
            wb = ctypes.c_size_t()
            if by_key:
                check(lib.adlhip_reduce_by_key_scratch_bytes(device._h, kt, vt, n, ctypes.byref(wb)), "adlhip_reduce_by_key_scratch_bytes")
            else:
                check(lib.adlhip_reduce_runs_scratch_bytes(device._h, np.dtype(keys.dtype).itemsize, vt, n, ctypes.byref(wb)),
                      "adlhip_reduce_runs_scratch_bytes")
            self._scratch(device, 0, wb.value)
            if uniqueOut is None:
                uniqueOut = Buffer(device, n, keys.dtype)
                own.append(uniqueOut)
            if reducedOut is None:
                reducedOut = Buffer(device, n, values.dtype)
                own.append(reducedOut)
            if countOut is None:
                countOut = Buffer(device, 1, np.uint32)
                own.append(countOut)

            def p(b):
                return b.ptr() if b is not None else None
            if by_key:
                check(lib.adlhip_reduce_by_key_typed(device._h, kt, 1 if descending else 0, keys.ptr(), vt, REDUCE_OPS[op], values.ptr(), n,
                                                     uniqueOut.ptr(), reducedOut.ptr(), p(c), p(o), countOut.ptr(), self.m_work.ptr(),
                                                     self.m_work.getSize()), what)
            else:
                check(lib.adlhip_reduce_runs(device._h, np.dtype(keys.dtype).itemsize, keys.ptr(), vt, REDUCE_OPS[op], values.ptr(), n,
                                             uniqueOut.ptr(), reducedOut.ptr(), p(c), p(o), countOut.ptr(), self.m_work.ptr(),
                                             self.m_work.getSize()), what)
        except AdlHipError:
            for b in own:
                b.release()
            raise
        return ReduceResult(uniqueOut, reducedOut, c, o, countOut)

    def reduceByKey(self, device, keys, values, n, op="sum", descending=False, counts=False, offsets=False, uniqueOut=None,
                    reducedOut=None, countOut=None):
        """op ("sum", "min", "max") over the values of every distinct key among the first n of `keys` -> ReduceResult.  The keys appear
        in the order of sortKeys(descending) and are equal when their bits are, as in unique(); reduced[r] belongs to unique[r].
        Values: uint32 / int32 / float32 / uint64 / int64 / float64, whatever the keys' width.  Integer sums wrap; float sums are IEEE
        adds in an unspecified but reproducible association; min / max follow the order of the typed sorts (floats: totalOrder, so
        -0 < +0 and NaNs are ordered, not propagated) whatever `descending` says.  counts / offsets / uniqueOut / countOut as in
        unique(), reducedOut (the values' dtype, n elements) likewise.  `keys` and `values` are left intact.  Enqueues and returns
        like unique(); read result.count (toHost) to learn R."""
        return self._reduce("reduceByKey", device, True, keys, values, n, op, descending, counts, offsets, uniqueOut, reducedOut, countOut)

    def reduceRuns(self, device, keys, values, n, op="sum", counts=False, offsets=False, uniqueOut=None, reducedOut=None, countOut=None):
        """reduceByKey for keys that are already grouped (any element type of 4 or 8 bytes): one result per run of adjacent keys with
        identical bits, the runs of runLengthEncode() -> ReduceResult."""
        return self._reduce("reduceRuns", device, False, keys, values, n, op, False, counts, offsets, uniqueOut, reducedOut, countOut)

    # -- typed scans, plain and by key (no reference counterpart; include/adlhip.h adlhip_scan_typed / adlhip_scan_by_key)
    def _scan(self, what, device, keys, dst, src, n, op, exclusive, init):
        if device is None:
            raise AdlHipError("%s needs a device" % what)
        if op not in REDUCE_OPS:
            raise AdlHipError("%s: op must be 'sum', 'min' or 'max', got %r" % (what, op))
        if keys is not None and np.dtype(keys.dtype).itemsize not in (4, 8):
            raise AdlHipError("%s: unsupported key type %s (4 or 8 bytes)" % (what, keys.dtype))
        vt = KEY_TYPES.get(np.dtype(src.dtype))
        if vt is None:
            raise AdlHipError("%s: unsupported value type %s (uint32, int32, float32, uint64, int64, float64)" % (what, src.dtype))
        if np.dtype(dst.dtype) != np.dtype(src.dtype):
            raise AdlHipError("%s: dst must have the values' type %s, got %s" % (what, src.dtype, dst.dtype))
        n = int(n)
        room = min(b.getSize() for b in (keys, dst, src) if b is not None)
        if n < 0 or room < n:
            raise AdlHipError("%s: n = %d outside [0, %d]" % (what, n, room))
        if init is not None and not exclusive:
            raise AdlHipError("%s: an inclusive scan takes no init" % what)
        hp = None
        if init is not None:
            pat = np.array(init, dtype=src.dtype).reshape(1)
            hp = pat.ctypes.data_as(ctypes.c_void_p)   # (read during the call)
        lib = _lib.load()
        wb = ctypes.c_size_t()
        if keys is None:
            check(lib.adlhip_scan_typed_scratch_bytes(device._h, vt, n, ctypes.byref(wb)), "adlhip_scan_typed_scratch_bytes")
        else:
            check(lib.adlhip_scan_by_key_scratch_bytes(device._h, np.dtype(keys.dtype).itemsize, vt, n, ctypes.byref(wb)),
                  "adlhip_scan_by_key_scratch_bytes")
        self._scratch(device, 0, wb.value)
        if keys is None:
            check(lib.adlhip_scan_typed(device._h, vt, REDUCE_OPS[op], 1 if exclusive else 0, hp, src.ptr(), dst.ptr(), n,
                                        self.m_work.ptr(), self.m_work.getSize()), what)
        else:
            check(lib.adlhip_scan_by_key(device._h, np.dtype(keys.dtype).itemsize, keys.ptr(), vt, REDUCE_OPS[op], 1 if exclusive else 0, hp,
                                         src.ptr(), dst.ptr(), n, self.m_work.ptr(), self.m_work.getSize()), what)

    def scanTyped(self, device, dst, src, n, op="sum", exclusive=False, init=None):
        """dst[i] = op ("sum", "min", "max") over src[0 .. i] (inclusive) or src[0 .. i - 1] (exclusive) for the first n elements;
        uint32 / int32 / float32 / uint64 / int64 / float64, dst of src's type.  dst may be src.  Integer sums wrap; float sums are
        IEEE adds in an unspecified but reproducible association; min / max follow the order of the typed sorts (floats: totalOrder,
        NaNs are ordered, not propagated).  Exclusive: dst[0] = init, dst[i] = op(init, inclusive[i - 1]); without an init dst[0] is
        the operator's identity pattern (0, the type's last / first pattern in that order) and dst[i] = inclusive[i - 1] bit for bit.
        An inclusive scan takes no init.  `src` is left intact unless it is dst.  Enqueues and returns."""
        self._scan("scanTyped", device, None, dst, src, n, op, exclusive, init)

    def scanByKey(self, device, keys, dst, src, n, op="sum", exclusive=False, init=None):
        """scanTyped within every run of adjacent keys with identical bits, the runs of runLengthEncode() (keys of any element type
        of 4 or 8 bytes, already grouped): the scan starts again at every run's first element, which gets init (exclusive) or its
        own bits (inclusive).  dst may be src, not keys."""
        self._scan("scanByKey", device, keys, dst, src, n, op, exclusive, init)

    # -- stream compaction (no reference counterpart; include/adlhip.h adlhip_compact_flagged / adlhip_compact_if_typed)
    def _compact(self, what, device, n, pred, arrays, indexOut, countOut, call):
        """arrays: [(name, input Buffer or None, output: None / False / True / Buffer)] -- an input's output defaults to a new Buffer of
        its type.  call(lib, pointers of the inputs, pointers of the outputs, index pointer, count pointer) runs the entry point."""
        if device is None:
            raise AdlHipError("%s needs a device" % what)
        n = int(n)
        room = min([pred.getSize()] + [b.getSize() for _, b, _ in arrays if b is not None])
        if n < 0 or room < n:
            raise AdlHipError("%s: n = %d outside [0, %d]" % (what, n, room))
        outs = []
        for name, b, o in arrays:
            if b is None:
                if o is not None and o is not False:
                    raise AdlHipError("%s: %sOut needs %s" % (what, name, name))
                outs.append(None)
                continue
            if np.dtype(b.dtype).itemsize not in (4, 8):
                raise AdlHipError("%s: unsupported %s type %s (4 or 8 bytes)" % (what, name, b.dtype))
            if o is None:
                o = True
            if o is not True and o is not False and (not hasattr(o, "getSize") or np.dtype(o.dtype) != np.dtype(b.dtype) or o.getSize() < n):
                raise AdlHipError("%s: %sOut must hold n elements of %s" % (what, name, b.dtype))
            outs.append(o)
        if countOut is not None and (np.dtype(countOut.dtype) != np.uint32 or countOut.getSize() < 1):
            raise AdlHipError("%s: countOut must hold one uint32 element" % what)
        if not any(o is not None and o is not False for o in outs) and (indexOut is None or indexOut is False):
            raise AdlHipError("%s: nothing asked (an array to compact, or indexOut)" % what)
        (idx,), own = self._runs_outputs(what, device, n, [("indexOut", indexOut, n)])
        try:
            lib = _lib.load()
            wb = ctypes.c_size_t()
            check(lib.adlhip_compact_scratch_bytes(device._h, n, ctypes.byref(wb)), "adlhip_compact_scratch_bytes")
            self._scratch(device, 0, wb.value)
            for k, (name, b, _) in enumerate(arrays):
                if outs[k] is True:
                    outs[k] = Buffer(device, n, b.dtype)
                    own.append(outs[k])
                elif outs[k] is False:
                    outs[k] = None
            if countOut is None:
                countOut = Buffer(device, 1, np.uint32)
                own.append(countOut)

            def p(b):
                return b.ptr() if b is not None else None
            check(call(lib, [p(b) for _, b, _ in arrays], [p(o) for o in outs], p(idx), countOut.ptr()), what)
        except AdlHipError:
            for b in own:
                b.release()
            raise
        return outs, idx, countOut

    def compactFlagged(self, device, flags, n, items=None, partition=False, itemsOut=None, indexOut=None, countOut=None):
        """The elements i < n whose flag byte flags[i] (a uint8 or bool Buffer) is non-zero, in input order -> CompactResult.  With S of
        them (result.count, on the device): items[0 .. S) the selected elements of `items` (any element type of 4 or 8 bytes; None:
        positions only), index[0 .. S) their positions.  partition=True: a stable partition -- the rejected elements follow in input
        order at [S, n); otherwise nothing at S and beyond is written.  itemsOut: a Buffer of the items' type to fill (n elements),
        False for none, default a new one; indexOut: True for a new uint32 Buffer, or one to fill; countOut (uint32, 1 element).
        The inputs are left intact.  Enqueues and returns; read result.count (toHost) to learn S."""
        what = "compactFlagged"
        if flags is not None and np.dtype(flags.dtype).itemsize != 1:
            raise AdlHipError("%s: flags must be one byte per element (uint8 or bool), got %s" % (what, flags.dtype))
        ib = np.dtype(items.dtype).itemsize if items is not None else 0

        def call(lib, ins, outs, idx, cnt):
            return lib.adlhip_compact_flagged(device._h, ib, ins[0], flags.ptr(), int(n), 1 if partition else 0, outs[0], idx, cnt,
                                              self.m_work.ptr(), self.m_work.getSize())
        if device is None:
            raise AdlHipError("%s needs a device" % what)
        outs, idx, cnt = self._compact(what, device, n, flags, [("items", items, itemsOut)], indexOut, countOut, call)
        return CompactResult(outs[0], None, idx, cnt)

    def compactIf(self, device, keys, n, cmp, threshold, values=None, partition=False, keysOut=None, valuesOut=None, indexOut=None,
                  countOut=None):
        """The keys i < n with keys[i] cmp threshold ("lt", "le", "gt", "ge", "eq", "ne") in the ascending order of sortKeys, in input
        order -> CompactResult (items = the keys).  Integers compare by value, floats by totalOrder (-NaN < -inf < ... < -0 < +0 < ...
        < +NaN: NaNs are ordered, -0 is below +0); eq / ne compare bits.  `values` (any element type of 4 or 8 bytes, whatever the
        keys' width) travel with their keys.  partition, keysOut / valuesOut (False: not written), indexOut and countOut as in
        compactFlagged.  The inputs are left intact.  Enqueues and returns; read result.count (toHost) to learn S."""
        what = "compactIf"
        if device is None:
            raise AdlHipError("%s needs a device" % what)
        kt = self._key_type(keys, what)
        if cmp not in CMP_OPS:
            raise AdlHipError("%s: cmp must be 'lt', 'le', 'gt', 'ge', 'eq' or 'ne', got %r" % (what, cmp))
        pat = np.array(threshold, dtype=keys.dtype).reshape(1)
        vb = np.dtype(values.dtype).itemsize if values is not None else 0

        def call(lib, ins, outs, idx, cnt):
            return lib.adlhip_compact_if_typed(device._h, kt, CMP_OPS[cmp], pat.ctypes.data_as(ctypes.c_void_p), ins[0], vb, ins[1], int(n),
                                               1 if partition else 0, outs[0], outs[1], idx, cnt, self.m_work.ptr(), self.m_work.getSize())
        outs, idx, cnt = self._compact(what, device, n, keys, [("keys", keys, keysOut), ("values", values, valuesOut)], indexOut, countOut,
                                       call)
        return CompactResult(outs[0], outs[1], idx, cnt)

    # -- histograms (no reference counterpart; include/adlhip.h adlhip_histogram_range_typed / adlhip_bincount_typed)
    def _histogram(self, what, device, keys, n, num_bins, by_edges, integers_only, countsOut, call):
        if device is None:
            raise AdlHipError("%s needs a device" % what)
        kt = self._key_type(keys, what)
        if integers_only and np.dtype(keys.dtype).kind == "f":
            raise AdlHipError("%s: integer keys only (uint32, int32, uint64, int64), got %s" % (what, keys.dtype))
        n, num_bins = int(n), int(num_bins)
        if n < 0 or keys.getSize() < n:
            raise AdlHipError("%s: n = %d outside [0, %d]" % (what, n, keys.getSize()))
        most = HISTOGRAM_MAX_RANGE_BINS if by_edges else (1 << 31) - 1
        if num_bins < 1 or num_bins > most:
            raise AdlHipError("%s: num_bins = %d outside [1, %d]" % (what, num_bins, most))
        if countsOut is not None and (np.dtype(countsOut.dtype) != np.uint32 or countsOut.getSize() < num_bins):
            raise AdlHipError("%s: countsOut must hold num_bins uint32 elements" % what)
        lib = _lib.load()
        wb = ctypes.c_size_t()
        check(lib.adlhip_histogram_scratch_bytes(device._h, kt, n, num_bins, 1 if by_edges else 0, ctypes.byref(wb)),
              "adlhip_histogram_scratch_bytes")
        self._scratch(device, 0, wb.value)
        own = countsOut is None
        if own:
            countsOut = Buffer(device, num_bins, np.uint32)
        try:
            check(call(lib, kt, n, num_bins, countsOut.ptr()), what)
        except AdlHipError:
            if own:
                countsOut.release()
            raise
        return countsOut

    def histogramRange(self, device, keys, n, edges, num_bins=None, include_upper=False, countsOut=None):
        """counts[b] = the keys i < n with edges[b] <= keys[i] < edges[b + 1], for the num_bins bins that the first num_bins + 1 elements
        of `edges` (a device Buffer of the keys' type; default: all of it) bound -> a uint32 Buffer of num_bins counters (countsOut, or
        a new one).  The edges are non-decreasing in the order of sortKeys -- integers by value, floats by totalOrder (-0 below +0,
        NaNs at the two ends) -- and both comparisons are made in that order, on bits: nothing is compared as a float.  Keys outside
        the edges are ignored; a key equal to repeated edges belongs to the last of them.  include_upper=True closes the last bin as
        numpy.histogram does: a key equal to the last edge counts in the last bin that is not empty by construction.  At most
        HISTOGRAM_MAX_RANGE_BINS bins.  The inputs are left intact.  Enqueues and returns."""
        what = "histogramRange"
        if edges is None or not hasattr(edges, "getSize"):
            raise AdlHipError("%s: edges must be a device Buffer of the keys' type" % what)
        if keys is not None and np.dtype(edges.dtype) != np.dtype(keys.dtype):
            raise AdlHipError("%s: edges are %s, keys %s" % (what, edges.dtype, keys.dtype))
        if num_bins is None:
            num_bins = edges.getSize() - 1
        if edges.getSize() < int(num_bins) + 1:
            raise AdlHipError("%s: %d bins need %d edges, got %d" % (what, num_bins, int(num_bins) + 1, edges.getSize()))

        def call(lib, kt, n_, bins, counts):
            return lib.adlhip_histogram_range_typed(device._h, kt, keys.ptr(), n_, edges.ptr(), bins, 1 if include_upper else 0, counts,
                                                    self.m_work.ptr(), self.m_work.getSize())
        return self._histogram(what, device, keys, n, num_bins, True, False, countsOut, call)

    def binCount(self, device, keys, n, num_bins, countsOut=None):
        """counts[v] = the keys i < n with value v, for 0 <= v < num_bins -> a uint32 Buffer of num_bins counters (countsOut, or a new
        one).  Integer keys only; negative keys and keys >= num_bins are ignored.  num_bins < 2^31: up to the LDS limit
        (device.getParam("debug.histogram_lds_bins"), 8192) one read of the keys, above it a sort of a copy of them.  The keys are
        left intact.  Enqueues and returns."""
        def call(lib, kt, n_, bins, counts):
            return lib.adlhip_bincount_typed(device._h, kt, keys.ptr(), n_, bins, counts, self.m_work.ptr(), self.m_work.getSize())
        return self._histogram("binCount", device, keys, n, num_bins, False, True, countsOut, call)

    # -- merge of sorted sequences (no reference counterpart; include/adlhip.h adlhip_merge_typed)
    def _merge(self, what, device, a, va, b, vb, out, vout, na, nb, descending, indexOut):
        if device is None:
            raise AdlHipError("%s needs a device" % what)
        if a is None or b is None:
            raise AdlHipError("%s: both inputs are required (an empty one with its count 0)" % what)
        kt = self._key_type(a, what)
        if np.dtype(b.dtype) != np.dtype(a.dtype):
            raise AdlHipError("%s: a is %s, b %s" % (what, a.dtype, b.dtype))
        na, nb = int(na), int(nb)
        for name, buf, n in (("na", a, na), ("nb", b, nb)):
            if n < 0 or buf.getSize() < n:
                raise AdlHipError("%s: %s = %d outside [0, %d]" % (what, name, n, buf.getSize()))
        n = na + nb
        if n >= 1 << 32:
            raise AdlHipError("%s: na + nb = %d; fewer than 2^32 elements" % (what, n))
        if out is not None and (not hasattr(out, "getSize") or np.dtype(out.dtype) != np.dtype(a.dtype) or out.getSize() < n):
            raise AdlHipError("%s: out must hold na + nb elements of %s" % (what, a.dtype))
        vbytes = 0
        if va is not None or vb is not None or vout is not None:
            if va is None or vb is None or vout is None:
                raise AdlHipError("%s: the values of a, of b and valuesOut go together" % what)
            vbytes = np.dtype(va.dtype).itemsize
            if vbytes not in (4, 8):
                raise AdlHipError("%s: unsupported values type %s (4 or 8 bytes)" % (what, va.dtype))
            if np.dtype(vb.dtype) != np.dtype(va.dtype) or np.dtype(vout.dtype) != np.dtype(va.dtype):
                raise AdlHipError("%s: the values are %s, %s and %s" % (what, va.dtype, vb.dtype, vout.dtype))
            if va.getSize() < na or vb.getSize() < nb or vout.getSize() < n:
                raise AdlHipError("%s: the values must hold na, nb and na + nb elements" % what)
        if out is None and vout is None and (indexOut is None or indexOut is False):
            raise AdlHipError("%s: nothing asked (out, valuesOut or indexOut)" % what)
        (idx,), own = self._runs_outputs(what, device, n, [("indexOut", indexOut, n)])
        try:
            lib = _lib.load()
            wb = ctypes.c_size_t()
            check(lib.adlhip_merge_scratch_bytes(device._h, kt, vbytes, na, nb, ctypes.byref(wb)), "adlhip_merge_scratch_bytes")
            self._scratch(device, 0, wb.value)

            def p(buf):
                return buf.ptr() if buf is not None else None
            check(lib.adlhip_merge_typed(device._h, kt, 1 if descending else 0, p(a), p(va), na, p(b), p(vb), nb, vbytes, p(out), p(vout),
                                         p(idx), self.m_work.ptr(), self.m_work.getSize()), what)
        except AdlHipError:
            for buf in own:
                buf.release()
            raise
        return idx

    def mergeKeys(self, device, a, b, out, na, nb, descending=False, indexOut=None):
        """The stable merge of the first na keys of `a` and the first nb keys of `b` -- Buffers of one key type (uint32, int32, float32,
        uint64, int64, float64), each sorted in the order of sortKeys(descending) -- into out[0 .. na + nb): what sortKeys gives for the
        concatenation, with one read and one write per element.  Where keys compare equal (same code: same bits) those of `a` come
        first.  indexOut: True for a new uint32 Buffer, or one to fill: the position in a || b (i for a[i], na + i for b[i]) of every
        output element; it is returned (None when not asked).  out may be None when only the positions are wanted.  The caller sizes
        the Buffers; the inputs are left intact and may be the same Buffer; out may be neither.  Inputs that are not sorted give an
        output in unspecified order, never an access outside the Buffers.  Enqueues and returns."""
        return self._merge("mergeKeys", device, a, None, b, None, out, None, na, nb, descending, indexOut)

    def mergePairs(self, device, keysA, valuesA, keysB, valuesB, keysOut, valuesOut, na, nb, descending=False, indexOut=None):
        """mergeKeys with a value per key (any element type of 4 or 8 bytes, one type for valuesA, valuesB and valuesOut, whatever the
        keys' width): valuesOut[j] is the value of the key keysOut[j].  keysOut may be None (values and / or positions only)."""
        if valuesA is None or valuesB is None or valuesOut is None:
            raise AdlHipError("mergePairs: valuesA, valuesB and valuesOut are required (mergeKeys merges keys alone)")
        return self._merge("mergePairs", device, keysA, valuesA, keysB, valuesB, keysOut, valuesOut, na, nb, descending, indexOut)

    # -- set operations on sorted sequences (no reference counterpart; include/adlhip.h adlhip_set_op_typed)
    def setOp(self, device, op, a, b, out, na, nb, descending=False, valuesA=None, valuesB=None, valuesOut=None, indexOut=None,
              countOut=None):
        """op ("intersection", "union", "difference", "symmetric_difference") of the first na keys of `a` and the first nb keys of `b`
        -- Buffers of one key type, each sorted in the order of sortKeys(descending) -- with thrust's multiset semantics: of a key
        that occurs m times in a and n times in b the result holds min(m, n) (the first of a's), max(m, n) (a's, then the last of
        b's), max(m - n, 0) (the last of a's) or |m - n| copies.  Keys are equal when their bits are.  -> SetOpResult: with S result
        elements (result.count, on the device) out[0 .. S) are the kept keys in the order of mergeKeys, valuesOut[0 .. S) the kept
        elements' own values (valuesA, valuesB and valuesOut go together: any element type of 4 or 8 bytes) and index[0 .. S) their
        positions in a || b (indexOut: True for a new uint32 Buffer, or one to fill).  out may be None when only values or positions
        are wanted.  Every output holds na elements for intersection and difference, na + nb for the other two; nothing at S and
        beyond is written.  The inputs are left intact and may be the same Buffer.  Inputs that are not sorted give an unspecified
        result, never an access outside the Buffers.  Enqueues and returns; read result.count (toHost) to learn S."""
        what = "setOp"
        if device is None:
            raise AdlHipError("%s needs a device" % what)
        if op not in SET_OPS:
            raise AdlHipError("%s: op must be 'intersection', 'union', 'difference' or 'symmetric_difference', got %r" % (what, op))
        if a is None or b is None:
            raise AdlHipError("%s: both inputs are required (an empty one with its count 0)" % what)
        kt = self._key_type(a, what)
        if np.dtype(b.dtype) != np.dtype(a.dtype):
            raise AdlHipError("%s: a is %s, b %s" % (what, a.dtype, b.dtype))
        na, nb = int(na), int(nb)
        for name, buf, n in (("na", a, na), ("nb", b, nb)):
            if n < 0 or buf.getSize() < n:
                raise AdlHipError("%s: %s = %d outside [0, %d]" % (what, name, n, buf.getSize()))
        if na + nb >= 1 << 32:
            raise AdlHipError("%s: na + nb = %d; fewer than 2^32 elements" % (what, na + nb))
        cap = na + nb if op in ("union", "symmetric_difference") else na
        if out is not None and (not hasattr(out, "getSize") or np.dtype(out.dtype) != np.dtype(a.dtype) or out.getSize() < cap):
            raise AdlHipError("%s: out must hold %d elements of %s" % (what, cap, a.dtype))
        vbytes = 0
        if valuesA is not None or valuesB is not None or valuesOut is not None:
            if valuesA is None or valuesB is None or valuesOut is None:
                raise AdlHipError("%s: valuesA, valuesB and valuesOut go together" % what)
            vbytes = np.dtype(valuesA.dtype).itemsize
            if vbytes not in (4, 8):
                raise AdlHipError("%s: unsupported values type %s (4 or 8 bytes)" % (what, valuesA.dtype))
            if np.dtype(valuesB.dtype) != np.dtype(valuesA.dtype) or np.dtype(valuesOut.dtype) != np.dtype(valuesA.dtype):
                raise AdlHipError("%s: the values are %s, %s and %s" % (what, valuesA.dtype, valuesB.dtype, valuesOut.dtype))
            if valuesA.getSize() < na or valuesB.getSize() < nb or valuesOut.getSize() < cap:
                raise AdlHipError("%s: the values must hold na, nb and %d elements" % (what, cap))
        if countOut is not None and (np.dtype(countOut.dtype) != np.uint32 or countOut.getSize() < 1):
            raise AdlHipError("%s: countOut must hold one uint32 element" % what)
        if out is None and valuesOut is None and (indexOut is None or indexOut is False):
            raise AdlHipError("%s: nothing asked (out, valuesOut or indexOut)" % what)
        (idx,), own = self._runs_outputs(what, device, max(cap, 1), [("indexOut", indexOut, cap)])
        try:
            lib = _lib.load()
            wb = ctypes.c_size_t()
            check(lib.adlhip_set_op_scratch_bytes(device._h, kt, vbytes, na, nb, ctypes.byref(wb)), "adlhip_set_op_scratch_bytes")
            self._scratch(device, 0, wb.value)
            if countOut is None:
                countOut = Buffer(device, 1, np.uint32)
                own.append(countOut)

            def p(buf):
                return buf.ptr() if buf is not None else None
            check(lib.adlhip_set_op_typed(device._h, kt, 1 if descending else 0, SET_OPS[op], p(a), p(valuesA), na, p(b), p(valuesB), nb, vbytes,
                                          p(out), p(valuesOut), p(idx), countOut.ptr(), self.m_work.ptr(), self.m_work.getSize()), what)
        except AdlHipError:
            for buf in own:
                buf.release()
            raise
        return SetOpResult(out, valuesOut, idx, countOut)

    # -- sorted search (no reference counterpart; include/adlhip.h adlhip_search_sorted_typed)
    def searchSorted(self, device, sortedKeys, needles, posOut, m, n, descending=False, right=False):
        """posOut[i], i < n = where needles[i] would be inserted among the first m keys of `sortedKeys` -- a Buffer of one of the six key
        types, sorted in the order of sortKeys(descending) -- to keep them sorted: the number of keys that come before the needle
        (right=True: before it or equal to it) in that order, always in [0, m].  numpy.searchsorted with side 'left' / 'right', in
        the order of the typed sorts: floats by totalOrder (-0 before +0, NaNs by sign at the two ends), equal means equal bits.
        `needles` is a Buffer of the same type, posOut a uint32 Buffer of n elements at least; the caller sizes them.  The inputs
        are left intact and may be the same Buffer; posOut may be neither.  A sequence that is not sorted gives unspecified
        positions in [0, m], never an access outside the Buffers.  Enqueues and returns."""
        what = "searchSorted"
        if device is None:
            raise AdlHipError("%s needs a device" % what)
        if sortedKeys is None or needles is None or posOut is None:
            raise AdlHipError("%s: sortedKeys, needles and posOut are required (an empty sequence with m = 0)" % what)
        kt = self._key_type(sortedKeys, what)
        if np.dtype(needles.dtype) != np.dtype(sortedKeys.dtype):
            raise AdlHipError("%s: sortedKeys is %s, needles %s" % (what, sortedKeys.dtype, needles.dtype))
        m, n = int(m), int(n)
        for name, buf, k in (("m", sortedKeys, m), ("n", needles, n)):
            if k < 0 or buf.getSize() < k:
                raise AdlHipError("%s: %s = %d outside [0, %d]" % (what, name, k, buf.getSize()))
            if k >= 1 << 32:
                raise AdlHipError("%s: %s = %d; fewer than 2^32 elements" % (what, name, k))
        if not hasattr(posOut, "getSize") or np.dtype(posOut.dtype) != np.uint32 or posOut.getSize() < n:
            raise AdlHipError("%s: posOut must be a uint32 buffer of %d elements" % (what, n))
        check(_lib.load().adlhip_search_sorted_typed(device._h, kt, 1 if descending else 0, 1 if right else 0, sortedKeys.ptr(), m,
                                                     needles.ptr(), n, posOut.ptr()), what)
        return posOut

    # -- join of sorted sequences and expansion of runs (no reference counterpart; include/adlhip.h adlhip_join_sorted_typed)
    @staticmethod
    def _count64(what, device, countOut, own):
        if countOut is None:
            countOut = Buffer(device, 1, np.uint64)
            own.append(countOut)
        return countOut

    def joinSorted(self, device, kind, a, b, na, nb, cap=0, indexA=None, indexB=None, countOut=None, descending=False):
        """The kind ("inner", "left", "semi", "anti") of join of the first na keys of `a` with the first nb keys of `b` -- Buffers of one
        key type, each sorted in the order of sortKeys(descending) -- as pairs of positions -> JoinResult.  a[i] with m equal keys in
        b, the first of them at lo, gives the rows (i, lo) .. (i, lo + m - 1) for "inner"; the same, or (i, JOIN_NONE) where m is 0, for
        "left"; (i, lo) once where m > 0 for "semi"; (i, JOIN_NONE) where m is 0 for "anti".  Rows are ordered by i, then by the
        position in b.  Keys are equal when their bits are.  result.count (one uint64, on the device; countOut to fill one) is T, the
        exact number of rows, never clamped; rows below min(T, cap) are written to indexA / indexB (True for a new uint32 Buffer of cap
        elements, or one to fill), nothing beyond.  cap = 0 without outputs only counts.  na + nb and na + cap are at most
        0xFFF00000.  The inputs are left intact and may be the same Buffer.  Inputs that are not sorted give unspecified rows, never
        an access outside the Buffers nor a position outside a and b.  Enqueues and returns; read result.count (toHost) to learn T."""
        what = "joinSorted"
        if device is None:
            raise AdlHipError("%s needs a device" % what)
        if kind not in JOIN_KINDS:
            raise AdlHipError("%s: kind must be 'inner', 'left', 'semi' or 'anti', got %r" % (what, kind))
        if a is None or b is None:
            raise AdlHipError("%s: both inputs are required (an empty one with its count 0)" % what)
        kt = self._key_type(a, what)
        if np.dtype(b.dtype) != np.dtype(a.dtype):
            raise AdlHipError("%s: a is %s, b %s" % (what, a.dtype, b.dtype))
        na, nb, cap = int(na), int(nb), int(cap)
        for name, buf, n in (("na", a, na), ("nb", b, nb)):
            if n < 0 or buf.getSize() < n:
                raise AdlHipError("%s: %s = %d outside [0, %d]" % (what, name, n, buf.getSize()))
        if na + nb > JOIN_MAX_ELEMS:
            raise AdlHipError("%s: na + nb = %d; at most %d elements" % (what, na + nb, JOIN_MAX_ELEMS))
        if cap < 0 or na + cap > JOIN_MAX_ELEMS:
            raise AdlHipError("%s: cap = %d outside [0, %d - na]" % (what, cap, JOIN_MAX_ELEMS))
        asked = [v for v in (indexA, indexB) if v is not None and v is not False]
        if cap == 0 and asked:
            raise AdlHipError("%s: cap is 0, so indexA and indexB must not be given" % what)
        if cap > 0 and not asked:
            raise AdlHipError("%s: nothing asked (indexA or indexB) with cap = %d" % (what, cap))
        if countOut is not None and (np.dtype(countOut.dtype) != np.uint64 or countOut.getSize() < 1):
            raise AdlHipError("%s: countOut must hold one uint64 element" % what)
        (ia, ib), own = self._runs_outputs(what, device, cap, [("indexA", indexA, cap), ("indexB", indexB, cap)])
        try:
            lib = _lib.load()
            wb = ctypes.c_size_t()
            check(lib.adlhip_join_scratch_bytes(device._h, kt, na, nb, cap, ctypes.byref(wb)), "adlhip_join_scratch_bytes")
            self._scratch(device, 0, wb.value)
            countOut = self._count64(what, device, countOut, own)

            def p(buf):
                return buf.ptr() if buf is not None else None
            check(lib.adlhip_join_sorted_typed(device._h, kt, 1 if descending else 0, JOIN_KINDS[kind], p(a), na, p(b), nb, cap, p(ia), p(ib),
                                               countOut.ptr(), self.m_work.ptr(), self.m_work.getSize()), what)
        except AdlHipError:
            for buf in own:
                buf.release()
            raise
        return JoinResult(ia, ib, countOut)

    def expandRuns(self, device, counts, numRuns, cap=0, values=None, runOut=None, rankOut=None, valuesOut=None, countOut=None):
        """Run-length decode, the inverse of runLengthEncode: counts[i] rows for every run i < numRuns (`counts`: a uint32 Buffer), in the
        order of the runs -> ExpandResult.  Row o of run i, whose rows start at start[i] = counts[0] + .. + counts[i - 1], gets
        run[o] = i, rank[o] = o - start[i] and values[o] = values[i] (`values` and valuesOut: Buffers of one element type of 4 or 8
        bytes).  result.count (one uint64, on the device; countOut to fill one) is T, the sum of the counts, never clamped; rows below
        min(T, cap) are written to runOut / rankOut (True for a new uint32 Buffer of cap elements, or one to fill) and valuesOut (a
        Buffer of cap elements), nothing beyond.  cap = 0 without outputs only counts.  numRuns + cap is at most 0xFFF00000.  The inputs
        are left intact.  Enqueues and returns; read result.count (toHost) to learn T."""
        what = "expandRuns"
        if device is None:
            raise AdlHipError("%s needs a device" % what)
        if counts is None or not hasattr(counts, "getSize") or np.dtype(counts.dtype) != np.uint32:
            raise AdlHipError("%s: counts must be a uint32 buffer" % what)
        n, cap = int(numRuns), int(cap)
        if n < 0 or counts.getSize() < n:
            raise AdlHipError("%s: numRuns = %d outside [0, %d]" % (what, n, counts.getSize()))
        if cap < 0 or n + cap > JOIN_MAX_ELEMS:
            raise AdlHipError("%s: cap = %d outside [0, %d - numRuns]" % (what, cap, JOIN_MAX_ELEMS))
        vbytes = 0
        if values is not None or valuesOut is not None:
            if values is None or valuesOut is None:
                raise AdlHipError("%s: values and valuesOut go together" % what)
            vbytes = np.dtype(values.dtype).itemsize
            if vbytes not in (4, 8):
                raise AdlHipError("%s: unsupported values type %s (4 or 8 bytes)" % (what, values.dtype))
            if np.dtype(valuesOut.dtype) != np.dtype(values.dtype):
                raise AdlHipError("%s: the values are %s and %s" % (what, values.dtype, valuesOut.dtype))
            if values.getSize() < n or valuesOut.getSize() < cap:
                raise AdlHipError("%s: the values must hold numRuns and %d elements" % (what, cap))
        asked = [v for v in (runOut, rankOut, valuesOut) if v is not None and v is not False]
        if cap == 0 and asked:
            raise AdlHipError("%s: cap is 0, so runOut, rankOut and valuesOut must not be given" % what)
        if cap > 0 and not asked:
            raise AdlHipError("%s: nothing asked (runOut, rankOut or valuesOut) with cap = %d" % (what, cap))
        if countOut is not None and (np.dtype(countOut.dtype) != np.uint64 or countOut.getSize() < 1):
            raise AdlHipError("%s: countOut must hold one uint64 element" % what)
        (run, rank), own = self._runs_outputs(what, device, cap, [("runOut", runOut, cap), ("rankOut", rankOut, cap)])
        try:
            lib = _lib.load()
            wb = ctypes.c_size_t()
            check(lib.adlhip_expand_scratch_bytes(device._h, n, cap, ctypes.byref(wb)), "adlhip_expand_scratch_bytes")
            self._scratch(device, 0, wb.value)
            countOut = self._count64(what, device, countOut, own)

            def p(buf):
                return buf.ptr() if buf is not None else None
            check(lib.adlhip_expand_runs(device._h, p(counts), n, vbytes, p(values) if valuesOut is not None else None, cap, p(run), p(rank),
                                         p(valuesOut), countOut.ptr(), self.m_work.ptr(), self.m_work.getSize()), what)
        except AdlHipError:
            for buf in own:
                buf.release()
            raise
        return ExpandResult(run, rank, valuesOut, countOut)

    def copy(self, device, dst, src, n):
        """Pprims::copy (Pprims.cpp:31-67, commented out in the reference): first n elements of src -> dst."""
        if device is None:
            raise AdlHipError("copy needs a device")
        assert dst.dtype == src.dtype and n <= dst.getSize() and n <= src.getSize()
        if n > 0:
            check(_lib.load().adlhip_memcpy_d2d(device._h, dst.ptr(), src.ptr(), int(n) * dst.dtype.itemsize), "copy")

    def fill(self, device, dst, value, n):
        """Pprims::fill (Pprims.cpp:69-120, commented out in the reference): n copies of one element.  `value`
        is anything numpy can turn into ONE element of dst.dtype (4-, 8- or 16-byte element types)."""
        if device is None:
            raise AdlHipError("fill needs a device")
        assert n <= dst.getSize()
        pat = np.array(value, dtype=dst.dtype).reshape(1)
        if pat.dtype.itemsize not in (4, 8, 16):
            raise AdlHipError("fill: element size %d (4, 8 or 16 bytes)" % pat.dtype.itemsize)
        if n > 0:
            check(_lib.load().adlhip_fill_pattern(device._h, dst.ptr(), pat.ctypes.data_as(ctypes.c_void_p),
                                                  pat.dtype.itemsize, int(n)), "fill")

    def scan(self, device, dst, src, n, sumOut=None):
        """Exclusive prefix sum.  sumOut: optional 1-element uint32 numpy array that receives the grand
        total once the caller has synchronised (Pprims.cpp:164-167 reads it back non-blocking too)."""
        if device is None:
            raise AdlHipError("scan needs a device")   # Pprims.cpp:124-127 ADLASSERT(0)
        lib = _lib.load()
        wb = ctypes.c_size_t()
        check(lib.adlhip_scan_scratch_bytes(device._h, int(n), ctypes.byref(wb)), "adlhip_scan_scratch_bytes")
        self._scratch(device, 0, wb.value)
        hp = None
        if sumOut is not None:
            assert sumOut.dtype == np.uint32 and sumOut.size >= 1
            self._sum_keep = sumOut
            hp = sumOut.ctypes.data_as(ctypes.c_void_p)
        check(lib.adlhip_exclusive_scan_u32(device._h, dst.ptr(), src.ptr(), self.m_work.ptr(), self.m_work.getSize(),
                                            int(n), hp), "scan")
