/*
 * adlhip.h -- C ABI of the MI355X (gfx950) HIP back-end that replaces the reference's OpenCL
 * back-end (the Adl/CL directory) and the device half of Tahoe::Pprims for the radix-sort / scan hot path.
 *
 * Plain C: opaque handle, raw device pointers, sizes.  No C++ or torch types cross this boundary.
 * Every function returns ADLHIP_SUCCESS (0) or ADLHIP_FAILURE (1) unless stated otherwise
 * (the reference defines the same two codes, Adl/Adl.h:22-23, but never returns them: its APIs are
 * void and fail through ADLASSERT, Tahoe/Math/Error.h:24-38).  Nothing throws across the boundary;
 * adlhip_last_error() returns the text of the calling thread's most recent failure.
 *
 * Threading: like the reference (one in-order command queue per device, Adl/CL/AdlCL.inl:303;
 * nothing re-entrant), calls on one adlhip_device must be serialised by the caller; distinct handles
 * may be driven from distinct threads.  All work is enqueued on the handle's one HIP stream and the
 * primitives return without synchronising, as the GPU branches of Pprims.cpp do.
 *
 * All citations are relative to the reference repository root.
 */
#ifndef ADLHIP_H
#define ADLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADLHIP_SUCCESS 0 /* Adl/Adl.h:22 ADL_SUCCESS */
#define ADLHIP_FAILURE 1 /* Adl/Adl.h:23 ADL_FAILURE */

typedef struct adlhip_device adlhip_device;

/* Replaces Device::getDeviceName/getDeviceVendor/getMemSize/getMaxAllocationSize and
 * DeviceUtils::getNCUs (Adl/CL/AdlCL.inl:704-759). */
typedef struct adlhip_info {
    int32_t compute_units;      /* CL_DEVICE_MAX_COMPUTE_UNITS analogue (AdlCL.inl:704-709) */
    int32_t wavefront_size;     /* 64 on gfx950 */
    int32_t lds_bytes_per_cu;   /* sharedMemPerMultiprocessor */
    int32_t clock_khz;
    uint64_t total_mem_bytes;
    uint64_t max_alloc_bytes;
    char name[128];
    char arch[64];              /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
    char vendor[32];
} adlhip_info;

/* ---- device lifetime ----------------------------------------------------------------------- */

/* DeviceUtils::getNDevices(TYPE_CL) -- Adl/Adl.inl:8-23.  Returns the count (0 if none / no driver). */
int adlhip_device_count(void);

/* DeviceUtils::allocate(TYPE_CL, Config{m_deviceIdx}) -- Adl/Adl.inl:73-98, DeviceCL::initialize
 * Adl/CL/AdlCL.inl:148-345.  device_idx beyond the last device is clamped to the last one
 * (AdlCL.inl:244).  Creates one in-order stream. */
int adlhip_device_create(int device_idx, adlhip_device** out);

/* Same, but enqueue on a caller-owned hipStream_t (e.g. torch's current stream) instead of creating
 * one.  No reference counterpart; used by the multi-GPU host code so sort and RCCL share a stream. */
int adlhip_device_create_on_stream(int device_idx, void* hip_stream, adlhip_device** out);

/* DeviceUtils::deallocate -- Adl/Adl.inl:100-105.  Like the reference (ADLASSERT(getUsedMemory()==0))
 * this FAILS, leaving the handle alive, while adlhip_used_bytes() != 0. */
int adlhip_device_destroy(adlhip_device* dev);

int adlhip_device_info(adlhip_device* dev, adlhip_info* out);

/* Device::getUsedMemory -- Adl/Adl.h:141; live bytes handed out by adlhip_malloc. */
uint64_t adlhip_used_bytes(adlhip_device* dev);

/* DeviceUtils::waitForCompletion(const Device*) -- Adl/Adl.inl:107-110 (clFinish, AdlCL.inl:567-570).
 * Also reports, as a failure, any device-side fault flag a kernel raised since the last sync. */
int adlhip_sync(adlhip_device* dev);

/* Stream-ordered fault check that never blocks, for callers that drain the stream by other means (a handle
 * made with adlhip_device_create_on_stream and synchronised through the stream's owner, e.g. torch): enqueues a
 * copy of the device's sticky fault word into pinned memory and reports -- as a failure, clearing the word -- what
 * the PREVIOUS such copy delivered once it has completed.  Call it once per batch: a look-back time-out or an
 * oversized segment of batch i surfaces at the check that follows the completion of batch i.  The live word the
 * waiters poll is cleared by the first kernel of every sort, so a failure never leaks into later sorts.
 * No reference counterpart (its errors are ADLASSERTs on the host, Tahoe/Math/Error.h:24-38). */
int adlhip_fault_check(adlhip_device* dev);

/* DeviceUtils::flush -- Adl/CL/AdlCL.inl:614-617.  HIP streams need no flush; kept for symmetry. */
int adlhip_flush(adlhip_device* dev);

/* The stream this handle enqueues on (hipStream_t as void*). */
void* adlhip_stream(adlhip_device* dev);

const char* adlhip_last_error(void);

/* ---- buffers: Buffer<T> alloc / copies / map -------------------------------------------------- */

/* Buffer<T>::allocate -> DeviceCL::allocate (Adl/CL/AdlCL.inl:356-420): device allocation, accounted
 * in the live-byte counter.  bytes == 0 yields *dptr == NULL and success. */
int adlhip_malloc(adlhip_device* dev, size_t bytes, void** dptr);
/* DeviceCL::deallocate (AdlCL.inl:422-439).  `bytes` must be the size given to adlhip_malloc. */
int adlhip_free(adlhip_device* dev, void* dptr, size_t bytes);

/* Buffer::write(host)/read(host)/write(Buffer) -- Adl/Adl.inl:273-303, AdlCL.inl:441-510.
 * Asynchronous and stream-ordered, like the non-blocking clEnqueue* calls they replace: the host
 * memory must stay valid until adlhip_sync().  Element offsets are folded into the pointers. */
int adlhip_memcpy_h2d(adlhip_device* dev, void* dst_dev, const void* src_host, size_t bytes);
int adlhip_memcpy_d2h(adlhip_device* dev, void* dst_host, const void* src_dev, size_t bytes);
int adlhip_memcpy_d2d(adlhip_device* dev, void* dst_dev, const void* src_dev, size_t bytes);

/* Buffer::clear / fill -- Adl/Adl.inl:305-315, AdlCL.inl:512-542 (byte-wise / 4-byte pattern). */
int adlhip_memset(adlhip_device* dev, void* dptr, int byte_value, size_t bytes);
int adlhip_fill_u32(adlhip_device* dev, void* dptr, uint32_t pattern, size_t count);
/* Pprims::fill(int | u32 | float4) -- Tahoe/ParallelPrimitives/Pprims.cpp:69-120 (FillIntKernel / FillU32Kernel /
 * FillF4Kernel, commented out in the reference): `count` copies of a 4-, 8- or 16-byte pattern read from host
 * memory at call time.  dptr must be aligned to pattern_bytes. */
int adlhip_fill_pattern(adlhip_device* dev, void* dptr, const void* pattern, size_t pattern_bytes, size_t count);

/* Buffer::getHostPtr / returnHostPtr -- Adl/Adl.inl:317-329, AdlCL.inl:544-565 (non-blocking
 * clEnqueueMapBuffer READ|WRITE / clEnqueueUnmapMemObject).  adlhip_map enqueues a device->pinned-host
 * copy and returns the host pointer; contents are valid after adlhip_sync().  adlhip_unmap enqueues the
 * host->device write-back and releases the staging memory once that copy has run; the device sees the
 * writes after adlhip_sync().  Exactly the call sequence of UnitTest/main.cpp:118-125.
 * adlhip_unmap: bytes = 0 writes back the whole mapping (Buffer::returnHostPtr carries no size). */
int adlhip_map(adlhip_device* dev, void* dptr, size_t bytes, void** hptr);
int adlhip_unmap(adlhip_device* dev, void* dptr, void* hptr, size_t bytes);

/* ---- the primitives: Tahoe::Pprims ----------------------------------------------------------- */

/* Element kinds the sort entry points handle. */
#define ADLHIP_ELEM_U32  0 /* Buffer<u32>   : Pprims::radixSort(..., Buffer<u32>&, ...)   Pprims.h:41 */
#define ADLHIP_ELEM_KV32 1 /* Buffer<uint2> : {x = key, y = value}                         Pprims.h:38 */
#define ADLHIP_ELEM_U64  2 /* 64-bit keys (BASELINE config #5; no reference API)                       */
#define ADLHIP_ELEM_SOA32 3 /* separate u32 key and u32 value arrays (*tmp_bytes is per array)           */

/* Scratch the caller must own, replacing Pprims' m_u32WorkBuffer[0] (ping-pong copy of the data,
 * Pprims.cpp:226-232, :332) and m_u32WorkBuffer[1] (histogram table, :229-230, :333-337).
 *   *tmp_bytes  : second data buffer, n elements
 *   *work_bytes : control scratch (digit tables / tile status words) and, for the sizes the large sort takes
 *                 ("sort.msd2": sorts of more than 1 Mi elements), its bucket and segment slabs -- about 1.5 x n elements
 *                 for whole u32 keys from 16 Mi keys up (their 16-bit second slab then lives in d_tmp; 64 Mi keys: 451 MB),
 *                 3 x n elements otherwise (64 Mi pairs: 1.7 GB; 256 Mi u64 keys: 6.1 GB).  The value
 *                 suffices for EVERY n' <= n with the current knobs (the need of a single n is not monotone:
 *                 smaller inputs use smaller tiles and so more status rows), so a caller may size its scratch
 *                 once for its largest batch; changing "sort.tile", "sort.digit_bits" or "sort.algo" later can
 *                 raise the requirement (the sort entry points re-check and fail loudly).
 * Data, tmp and work buffers of the sorts and partitions need 16-byte alignment and no more; a pointer that is not
 * 16-byte aligned is refused before anything is enqueued.  The work buffer's contents on entry are arbitrary.
 * n beyond 0xFFF00000 -- the kernels index elements with 32 bits and keep 2^20 of head-room below 2^32 -- is refused by the scratch
 * queries as it is by the sorts. */
int adlhip_radix_sort_scratch_bytes(adlhip_device* dev, int elem_kind, size_t n,
                                    size_t* tmp_bytes, size_t* work_bytes);

/* The same for a sort on `sort_bits` bits, at one of three levels (sizes: level 0 <= level 2 <= level 1):
 *   level 0: the minimum -- the reference's own contract (Pprims.cpp:332-337: the n-element partner array and a digit table of
 *            a few KiB).  Every sort entry point accepts a work buffer of this size; the sort then runs the per-digit
 *            three-kernel passes (64 Mi u32 keys: 75-81 instead of 206-215 Gkeys/s, profiles/r4_bench_n1.json).
 *   level 1: full speed -- what adlhip_radix_sort_scratch_bytes reports for whole keys.  A sort on fewer bits than the key has
 *            takes the stable form of the large sort, whose second slab cannot shrink to 16 bits per key, and so needs more.
 *   level 2: lean -- whole u32 / u64 keys keep the large sort (cursor form) with 12 % instead of 50 % of head-room in the
 *            first pass's bucket slabs: 64 Mi u32 keys 306 MB of work instead of 451, same speed on keys spread evenly over
 *            their range; keys whose density varies by more than ~10 % from one 256th of the range to the next go through
 *            the safety net inside the sort (correct, about 4 x slower; nothing is remembered between sorts).  Pairs, SoA and sorts
 *            on part of the key keep the stable form of the large sort with statistical head-room only (mean + 8 sd in the first
 *            pass's sub-slabs, + 7.5 sd in the segment slabs, instead of + 50 %): 64 Mi pairs 1.25 GB instead of 1.7.
 * With a work buffer between the levels, every path checks its own need and the sort takes the fastest one that fits. */
int adlhip_radix_sort_scratch_bytes_for(adlhip_device* dev, int elem_kind, size_t n, int sort_bits, int level,
                                        size_t* tmp_bytes, size_t* work_bytes);

/* Pprims::radixSort(const Device*, const Buffer<u32>& inout, int n, int sortBits=32)
 * -- Tahoe/ParallelPrimitives/Pprims.h:41, Pprims.cpp:304-406.
 * Sorts d_keys_inout[0..n) ascending by the low `sort_bits` bits of each key, stably with respect to
 * input order; the result is in d_keys_inout (odd pass counts are copied back, Pprims.cpp:400-403).
 * sort_bits: multiple of 4 in [4,32] (Pprims.cpp:330); anything else fails.  Unlike the reference
 * (n % 256 == 0, Pprims.cpp:327) any n >= 0 is accepted.  Enqueues and returns. */
int adlhip_radix_sort_u32(adlhip_device* dev, uint32_t* d_keys_inout, uint32_t* d_tmp,
                          void* d_work, size_t work_bytes, size_t n, int sort_bits);

/* Pprims::radixSort(const Device*, const Buffer<uint2>& inout, int n, int sortBits=32)
 * -- Pprims.h:38, Pprims.cpp:200-302.  Elements are 8-byte {u32 key (.x); u32 value (.y)} pairs
 * (Tahoe/Math/Math.h:175-188 == SortData, Tahoe/Algorithm/Sort/RadixSort.h:10-27); stable. */
int adlhip_radix_sort_kv32(adlhip_device* dev, void* d_pairs_inout, void* d_tmp,
                           void* d_work, size_t work_bytes, size_t n, int sort_bits);

/* Key-value sort on SEPARATE key and value arrays (structure of arrays): the layout of the reference's
 * never-launched SortAndScatterKernel(gSrc, gSrcVal, ...) (RadixSortKeyValueKernels.cl:354-509).
 * Same contract as adlhip_radix_sort_kv32: ascending by the low sort_bits key bits, stable; values follow
 * their keys.  d_tmp_keys / d_tmp_vals: n u32 each (adlhip_radix_sort_scratch_bytes with ADLHIP_ELEM_SOA32).
 * The histogram / count kernels read the key array only (half the bytes of the AoS layout). */
int adlhip_radix_sort_soa32(adlhip_device* dev, uint32_t* d_keys_inout, uint32_t* d_vals_inout,
                            uint32_t* d_tmp_keys, uint32_t* d_tmp_vals, void* d_work, size_t work_bytes,
                            size_t n, int sort_bits);

/* The same on keys of 4 or 8 bytes and values of 4, 8 or 16 bytes ("SoA key/value API ... and 64-bit values";
 * the reference's kernel, RadixSortKeyValueKernels.cl:354-509, takes `const u32* gSrc, const int* gSrcVal`).  Ascending by the
 * low sort_bits key bits (a multiple of 4 in [4, 8 * key_bytes]), stable, values follow their keys; n < 2^32.
 * (4, 4) is adlhip_radix_sort_soa32.  Every other width sorts {32 key bits, source index} pairs with the stable pair sort of
 * adlhip_radix_sort_kv32 -- once for u32 keys, twice (low dword, then high dword) for u64 keys on more than 32 bits -- and
 * fetches keys and values ONCE, at the end, from where the indices point; the value's width only costs in that gather.
 * d_tmp_keys: n keys (may be NULL for 4-byte keys), d_tmp_vals: n values; sizes and the work buffer's size from
 * adlhip_radix_sort_soa_scratch_bytes.  All buffers 16-byte aligned. */
int adlhip_radix_sort_soa_scratch_bytes(adlhip_device* dev, int key_bytes, int value_bytes, size_t n, int sort_bits,
                                        size_t* tmp_keys_bytes, size_t* tmp_vals_bytes, size_t* work_bytes);
int adlhip_radix_sort_soa(adlhip_device* dev, void* d_keys_inout, int key_bytes, void* d_vals_inout, int value_bytes,
                          void* d_tmp_keys, void* d_tmp_vals, void* d_work, size_t work_bytes, size_t n, int sort_bits);

/* 64-bit keys, ascending; sort_bits multiple of 4 in [4,64]. */
int adlhip_radix_sort_u64(adlhip_device* dev, uint64_t* d_keys_inout, uint64_t* d_tmp,
                          void* d_work, size_t work_bytes, size_t n, int sort_bits);

/* ---- typed keys, order, argsort (no reference counterpart) ----------------------------------- */

/* The sorts above order unsigned bit patterns, ascending -- all the reference has (Pprims.h:38-41).  These entry points sort signed
 * integers, IEEE-754 floats and descending orders with the same kernels, through an order-preserving bijection between a typed key
 * and an unsigned key of the same width (integer instructions only):
 *   unsigned: identity;  signed: the sign bit flipped;  float: bits ^ (sign set ? all ones : sign bit);  descending: the complement.
 * Floats sort in IEEE-754 totalOrder: -NaN < -inf < ... < -denormal < -0 < +0 < +denormal < ... < +inf < +NaN, NaNs of one sign by
 * payload.  So -0 sorts before +0, and NaNs whose sign bit is set come FIRST, not last (descending: the mirror image).  Every sort
 * below is stable: equal keys keep their input order, also descending (torch.sort(descending=True, stable=True) does the same).
 * Where keys are compared for EQUALITY (adlhip_run_length_encode, adlhip_unique_typed) it is equality of bits, consistent with that
 * order: -0 and +0 are two keys, NaNs with different payloads are different keys. */
#define ADLHIP_KEY_U32 0
#define ADLHIP_KEY_I32 1
#define ADLHIP_KEY_F32 2
#define ADLHIP_KEY_U64 3
#define ADLHIP_KEY_I64 4
#define ADLHIP_KEY_F64 5

#define ADLHIP_ORDER_ASCENDING  0
#define ADLHIP_ORDER_DESCENDING 1

/* The codec alone (no reference counterpart): d_dst[i] = enc(d_src[i]) for i < n, so that unsigned ascending order of the encoded keys
 * is the requested order of the typed ones; adlhip_key_decode is the exact inverse -- every bit pattern round-trips, NaN payloads and
 * -0 included.  d_dst may equal d_src; both 16-byte aligned.  One streaming sweep (read n keys, write n keys); U32 / U64 ascending is
 * the identity and copies (nothing at all when d_dst == d_src).  For callers that feed encoded keys to the unsigned entry points
 * themselves (partial-bit sorts, partitions, the sharded sort). */
int adlhip_key_encode(adlhip_device* dev, int key_type, int order, void* d_dst, const void* d_src, size_t n);
int adlhip_key_decode(adlhip_device* dev, int key_type, int order, void* d_dst, const void* d_src, size_t n);

/* Scratch of the three typed sorts below (no reference counterpart).  mode 0 = keys only (adlhip_sort_keys_typed: *tmp_keys_bytes is its
 * d_tmp), 1 = pairs (value_bytes: 4, 8 or 16; *tmp_keys_bytes is 0 for 4-byte keys, which need no partner array), 2 = argsort (no
 * partner arrays; value_bytes is ignored).  Unlike the unsigned sorts, the typed entry points REFUSE a work buffer below
 * *work_bytes instead of taking a slower path. */
int adlhip_sort_typed_scratch_bytes(adlhip_device* dev, int key_type, int mode, int value_bytes, size_t n,
                                    size_t* tmp_keys_bytes, size_t* tmp_vals_bytes, size_t* work_bytes);

/* Sorts n typed keys in place (no reference counterpart): encode in place -> adlhip_radix_sort_u32 / _u64 on whole keys -> decode in
 * place.  Cost: two streaming sweeps of n keys (read + write each) on top of the unsigned sort; U32 / U64 ascending launch no codec
 * kernel and cost what adlhip_radix_sort_u32 / _u64 cost.  NaN and -0 order: above.  d_tmp: n keys.  Enqueues and returns.
 * If the unsigned sort refuses after the encode has been enqueued (knobs changed since the scratch was sized: "sort.algo" = 0
 * with a work buffer that does not hold the one-sweep path), the decode is enqueued all the same: the call
 * fails with the sort's message and the keys are what they were, unsorted. */
int adlhip_sort_keys_typed(adlhip_device* dev, int key_type, int order, void* d_keys_inout, void* d_tmp,
                           void* d_work, size_t work_bytes, size_t n);

/* Sorts n typed keys and their values of 4, 8 or 16 bytes in place, stably (no reference counterpart; NaN and -0 order: above).
 * Like adlhip_radix_sort_soa with wide values it sorts {32 encoded key bits, source index} pairs -- once for 4-byte keys, twice for
 * 8-byte keys -- and fetches keys and values once, at the end; the codec sits inside the pack and gather kernels that path runs
 * anyway, so typed pairs cost NO sweep on top of the unsigned path.  (4-byte key, 4-byte value) takes this path too.
 * d_tmp_keys: n keys (may be NULL for 4-byte keys), d_tmp_vals: n values.  n < 2^32.  Enqueues and returns. */
int adlhip_sort_pairs_typed(adlhip_device* dev, int key_type, int order, void* d_keys_inout, void* d_vals_inout, int value_bytes,
                            void* d_tmp_keys, void* d_tmp_vals, void* d_work, size_t work_bytes, size_t n);

/* Argsort (no reference counterpart; NaN and -0 order: above): d_keys_in is left intact; d_index_out[j] = position in the input of the
 * j-th element of the sorted order (stable: equal keys appear with ascending positions, descending too); d_keys_out_or_null receives
 * the sorted keys when given (it must not be d_keys_in).  The same index sort as adlhip_sort_pairs_typed, written straight to the
 * caller's arrays: no codec sweep, no copy back.  n < 2^32.  Enqueues and returns. */
int adlhip_argsort_typed(adlhip_device* dev, int key_type, int order, const void* d_keys_in, void* d_keys_out_or_null,
                         uint32_t* d_index_out, void* d_work, size_t work_bytes, size_t n);

/* ---- top-k (no reference counterpart) --------------------------------------------------------- */

/* Work bytes of adlhip_topk_typed for (key_type, n, k); one size covers both of its paths.  With kb = bytes per key, every part
 * rounded up to 256 bytes:
 *   max( 82176 (selection state: ten 2048-bin histograms, ranks, cursors) + 4 k (result list)
 *          + max( 2 n (kb + 4)                                     two survivor lists of {code, position}
 *               , 4 k + kb k + max(W_u32(k), W_argsort(k)) ),      the finish, which runs when the lists are dead
 *        W_argsort(n) + n kb + 4 n )                               the full argsort and its full-length outputs
 * W_argsort = *work_bytes of adlhip_sort_typed_scratch_bytes (mode 2), W_u32 = *work_bytes of adlhip_radix_sort_scratch_bytes (u32 keys).
 * W_argsort(n) holds two arrays of n 8-byte pairs, so the first term exceeds the second only for small n (the fixed state) and for
 * 8-byte keys by less than the k-element finish. */
int adlhip_topk_scratch_bytes(adlhip_device* dev, int key_type, size_t n, size_t k, size_t* work_bytes);

/* The k first elements of the stable order, sorted (NaN and -0 order: above): exactly the first k entries of what
 * adlhip_argsort_typed(dev, key_type, order, ...) returns for the same input.  d_index_out[j] = position in the input of the j-th
 * element, d_keys_out[j] = its key, bit for bit; ADLHIP_ORDER_DESCENDING gives the k largest, largest first, ascending the k smallest.
 * Ties at the k-th key go to the lower input position in both orders, so the result is deterministic.
 * d_keys_in is never written.  At least one output must be given; each holds k elements, is 16-byte aligned (as are d_keys_in and
 * d_work) and must not overlap the input.  0 <= k <= n < 2^32; k == 0 succeeds and enqueues nothing.  k > n, a misaligned pointer, an
 * unknown key type or order, or work_bytes below adlhip_topk_scratch_bytes fail before anything is enqueued.
 * Enqueues and returns: nothing is copied to the host and nothing is remembered between calls.  Small k ("topk.algo"): radix select on
 * the composite (encoded key, position) in 11-bit digits, most significant first -- one histogram sweep of the keys, one filtering
 * sweep, then one launch per further digit on the keys that share the k-th key's leading digits; which bin holds the k-th key, how
 * many keys survive and whether selection is complete are decided on the device (launch grids depend on n alone; a level with
 * nothing to do leaves at once).  The k positions are then sorted, their keys gathered and the stable typed pair sort orders the k
 * (key, position) pairs.  Large k: the full argsort into d_work, its first k entries copied out.  All selection state lives in
 * d_work, whose contents on entry are arbitrary; the handle owns no word of it. */
int adlhip_topk_typed(adlhip_device* dev, int key_type, int order, const void* d_keys_in, size_t n, size_t k,
                      void* d_keys_out_or_null, uint32_t* d_index_out_or_null, void* d_work, size_t work_bytes);

/* Work bytes of adlhip_topk_rows_typed: one size for both of its paths -- what adlhip_topk_scratch_bytes(dev, key_type, cols, k) reports,
 * the need of the per-row loop; the rows share it.  The row kernel uses no global scratch and never touches d_work. */
int adlhip_topk_rows_scratch_bytes(adlhip_device* dev, int key_type, size_t rows, size_t cols, size_t k, size_t* work_bytes);

/* Top-k along the rows of a rows x cols matrix: for every row r < rows the output row is exactly the first k entries of
 * adlhip_argsort_typed applied to that row alone (same key order, NaN and -0 included; ties go to the lower column in both orders).
 * Row r of the input starts at element r * row_stride (row_stride in elements, >= cols); the outputs are dense rows x k, row-major:
 * d_index_out[r * k + j] = the COLUMN of the j-th element of row r, d_keys_out[r * k + j] = its key, bit for bit.
 * Only the base pointers (d_keys_in, the outputs, d_work) need 16-byte alignment: a row may start at any element, cols and row_stride
 * may be odd.  d_keys_in is never written; the elements between cols and row_stride are never read either.  At least one output must
 * be given and neither may overlap the input.  0 <= k <= cols < 2^32; k == 0 or rows == 0 succeeds and enqueues nothing.  k > cols,
 * row_stride < cols, a misaligned base pointer, both outputs NULL, an output overlapping the input, an unknown key type or order, or
 * work_bytes below adlhip_topk_rows_scratch_bytes fail before anything is enqueued.  Enqueues and returns; nothing data-dependent
 * reaches the host and nothing is remembered between calls (the handle owns no device word of it).
 * Two paths ("topk.rows_algo"), the same result bit for bit:
 *   the row kernel (k <= 2048): one workgroup of 256 threads per row, workgroups take rows in turns; everything lives in LDS (4096
 *     composites {encoded key, column} + a 2048-bin histogram).  cols <= 4096: the row is read once, sorted in LDS, its first k
 *     written.  Longer rows: radix select on the composite in the 11-bit digits of adlhip_topk_typed -- each level re-reads the row
 *     (from L2) and counts one digit -- until the certain items and the chosen bin together fit the 4096 slots, one collecting read,
 *     then the same sort.  No global scratch, no atomics to global memory, no workgroup depends on another.
 *   the per-row loop: `rows` runs of adlhip_topk_typed's own paths ("topk.algo" decides per row as there) on the shared d_work, in
 *     stream order.  Correct for every shape; rows * (a dozen launches or more). */
int adlhip_topk_rows_typed(adlhip_device* dev, int key_type, int order, const void* d_keys_in, size_t rows, size_t cols,
                           size_t row_stride, size_t k, void* d_keys_out_or_null, uint32_t* d_index_out_or_null,
                           void* d_work, size_t work_bytes);

/* ---- sort and argsort along rows (no reference counterpart) ----------------------------------- */

/* Work bytes of adlhip_sort_rows_typed for (key_type, rows, cols): the need of the path the knobs choose NOW ("sort.rows_algo").
 * The row kernel uses no global scratch: 0.  The flat path, with N = rows * cols and kb = bytes per key, every part rounded up to 256
 * bytes:  N kb (the rows packed densely; always counted, used when row_stride != cols) + 4 arrays of 4 N (positions, row ids and the
 * partner arrays of their sort) + max(W_argsort(N), W_soa32(N, bits of rows - 1)); rows == 1 needs W_argsort(cols) alone.
 * W_argsort = *work_bytes of adlhip_sort_typed_scratch_bytes (mode 2), W_soa32 = that of adlhip_radix_sort_soa_scratch_bytes (4, 4).
 * rows * cols >= 2^32 and, under "sort.rows_algo" = 1, cols > 4096 are refused here as they are by the sort. */
int adlhip_sort_rows_scratch_bytes(adlhip_device* dev, int key_type, size_t rows, size_t cols, size_t* work_bytes);

/* Sort and argsort along the rows of a rows x cols matrix -- torch.sort(t, dim=-1, stable=True), cub::DeviceSegmentedSort on equal
 * segments: for every row r < rows the output row is exactly what adlhip_argsort_typed(dev, key_type, order, ...) returns for that row
 * alone (same key order, NaN and -0 included; stable: equal keys appear by ascending column, in both orders).
 * Row r of the input starts at element r * row_stride (row_stride in elements, >= cols); the outputs are dense rows x cols, row-major:
 * d_index_out[r * cols + j] = the COLUMN of the j-th element of row r, d_keys_out[r * cols + j] = its key, bit for bit.
 * Only the base pointers (d_keys_in, the outputs, d_work) need 16-byte alignment: a row may start at any element, cols and row_stride
 * may be odd.  d_keys_in is never written; the elements between cols and row_stride are never read either.  At least one output must
 * be given and neither may overlap the input.  rows * cols < 2^32; rows == 0 or cols == 0 succeeds and enqueues nothing.  A NULL or
 * misaligned base pointer, both outputs NULL, an output overlapping the input, row_stride < cols, an unknown key type or order,
 * rows * cols >= 2^32, or work_bytes below adlhip_sort_rows_scratch_bytes fail before anything is enqueued.  Enqueues and returns;
 * nothing data-dependent reaches the host and nothing is remembered between calls (the handle owns no device word of it).
 * Two paths, chosen on the host from cols alone ("sort.rows_algo"), the same result bit for bit:
 *   the row kernel (cols <= 4096): a workgroup of 256 threads holds a tile of 4096 composites {encoded key, column} in LDS.  With P the
 *     power of two >= cols (at least 2) a tile takes G = 4096 / P rows side by side, each padded to P slots, and ONE bitonic network
 *     sorts all of them at once: it runs the merge phases up to length P only -- log2(P) (log2(P) + 1) / 2 stages -- with the compare
 *     direction taken from the index inside the row's block, so that every block comes out ascending.  Workgroups take tiles in turns.
 *     row_stride == cols: the G rows of a tile are one span, read in 16-byte loads; otherwise row by row.  Every key is read once,
 *     every output written once; no global scratch (d_work may be NULL when 0 bytes are reported), no atomics to global memory, no
 *     fence, no workgroup depends on another.
 *   the flat path (any cols): the rows are packed densely when row_stride != cols; adlhip_argsort_typed's sort of all N keys gives
 *     positions p in key order; a kernel writes their rows p / cols; adlhip_radix_sort_soa32 sorts (row, p) stably on the bits of
 *     rows - 1, which keeps every row's elements in key order and ties by ascending position; a last kernel writes the columns
 *     p - row * cols and gathers the keys from the input.  One row is the argsort itself, written straight to the outputs. */
int adlhip_sort_rows_typed(adlhip_device* dev, int key_type, int order, const void* d_keys_in, size_t rows, size_t cols,
                           size_t row_stride, void* d_keys_out_or_null, uint32_t* d_index_out_or_null,
                           void* d_work, size_t work_bytes);

/* ---- sort and argsort within variable-length segments (no reference counterpart) -------------- */

#define ADLHIP_SEGMENT_INDEX_LOCAL  0   /* position inside the segment (what sort_rows calls the column) */
#define ADLHIP_SEGMENT_INDEX_GLOBAL 1   /* position in d_keys_in */

/* Work bytes of adlhip_sort_segments_typed for (n, num_segments = S, max_segment): the need of the path the knobs choose NOW
 * ("sort.segments_algo"); key_type is checked and does not change the size.  Every part rounded up to 256 bytes:
 *   the segment kernel  4 arrays of 4 S (class numbers, segment ids and the partner arrays of their sort) + 256 (the class counts) +
 *                       W_soa32(S, 4)
 *   the flat path       4 arrays of 4 n (positions, segment ids and the partner arrays of their sort) + max(W_argsort(n),
 *                       W_soa32(n, bits of S - 1 rounded up to a multiple of 4)); S == 1 needs W_argsort(n) alone.
 * W_argsort = *work_bytes of adlhip_sort_typed_scratch_bytes (mode 2), W_soa32 = that of adlhip_radix_sort_soa_scratch_bytes (4, 4).
 * n == 0 or S == 0: 0.  n or S beyond what the flat sorts index (n >= 2^32 among them) and, under "sort.segments_algo" = 1,
 * max_segment == 0 or > 4096 are refused here as they are by the sort. */
int adlhip_sort_segments_scratch_bytes(adlhip_device* dev, int key_type, size_t n, size_t num_segments, size_t max_segment,
                                       size_t* work_bytes);

/* Sort and argsort within segments -- cub::DeviceSegmentedSort, the column indices of every CSR row, the members of every group, the
 * tokens of every sequence of a ragged batch: for every segment s < S = num_segments, with elements [off[s], off[s + 1]) of d_keys_in,
 * the same positions of the outputs hold exactly what adlhip_argsort_typed(dev, key_type, order, ...) returns for that segment alone
 * (keys bit for bit, totalOrder on NaN and -0; stable: equal keys appear by ascending position, in both orders).  d_index_out holds
 * the position inside the segment (ADLHIP_SEGMENT_INDEX_LOCAL) or that plus off[s] (ADLHIP_SEGMENT_INDEX_GLOBAL).
 * d_offsets: S + 1 ascending u32 element offsets in device memory, off[0] = 0, off[S] = n -- what adlhip_run_length_encode and
 * adlhip_unique_typed hand out.  Empty segments may stand anywhere, so S may exceed n.  n < 2^32 and S within what the flat sorts
 * index.  d_keys_in is never written.  At least one of the two outputs must be given; neither may overlap the input or d_offsets.
 * Only the base pointers (d_keys_in, d_offsets, the outputs, d_work) need 16-byte alignment, the count word 4-byte alignment.
 * n == 0 or S == 0 succeeds and enqueues nothing but, when the count word is given, one 4-byte clear of it.  A NULL or misaligned
 * pointer, an overlap, an unknown key type, order or index_base, n >= 2^32, or work_bytes below adlhip_sort_segments_scratch_bytes
 * fail before anything is enqueued.  Enqueues and returns; nothing data-dependent reaches the host, the launch grids depend on n, S
 * and max_segment alone, nothing is remembered between calls, all state lives in d_work (the handle owns no device word of it).
 * Offsets that break the requirements (not ascending, off[S] != n, ...) give an unspecified result but never an access outside the
 * arrays: every offset is clamped to [previous, n] wherever it is used and every segment id to [0, S - 1].
 * max_segment: the caller's upper bound on the longest segment, 0 = unknown.  The host picks the path from it alone
 * ("sort.segments_algo"), the same result bit for bit:
 *   the segment kernel (0 < max_segment <= 4096): a plan -- one thread per segment writes (class, id), class k = 1 .. 12 for the
 *     smallest power of two P = 2^k >= len (at least 2), 0 for an empty segment, 13 for len > 4096; adlhip_radix_sort_soa32 sorts
 *     the pairs stably on 4 bits; one workgroup finds the class counts in the sorted classes -- and then ONE launch of the row
 *     kernel's tile and network: a tile of class k holds 4096 / P listed segments side by side, each padded to P slots, and the
 *     bitonic network that stops at length P sorts all of them; workgroups take the tiles of all classes in turns.  Skewed lengths
 *     do not pad every segment to the longest.  Every key is read once, every output written once; no atomics to global memory, no
 *     fence, no workgroup depends on another.
 *     A segment longer than 4096 -- the bound was wrong -- is a defined result, not a fault: it is passed through in input order
 *     (keys copied, identity indices, local or global) and counted in *d_num_oversized_out.
 *   the flat path (any lengths): adlhip_argsort_typed's sort of all n keys gives positions p in key order; the segment of p is its
 *     upper bound in off[1 .. S] (the kernel of adlhip_search_sorted_typed, which steps over runs of empty segments);
 *     adlhip_radix_sort_soa32 sorts (segment, p) stably on the bits of S - 1; a last kernel writes p - off[segment] or p and gathers
 *     the keys.  S == 1 is the argsort itself, written straight to the outputs.
 * d_num_oversized_out, when given, is always written: the number of segments passed through, 0 on the flat path.  The handle's fault
 * word is not involved. */
int adlhip_sort_segments_typed(adlhip_device* dev, int key_type, int order, const void* d_keys_in, size_t n, const uint32_t* d_offsets,
                               size_t num_segments, size_t max_segment, int index_base, void* d_keys_out_or_null,
                               uint32_t* d_index_out_or_null, uint32_t* d_num_oversized_out_or_null, void* d_work, size_t work_bytes);

/* ---- unique keys, run lengths, inverse indices (no reference counterpart) --------------------- */

/* Key equality in this block is equality of BITS, consistent with the totalOrder above (NaN and -0 order): -0 and +0 are two keys, NaNs
 * with different payloads are different keys, NaNs with the same bits are one key.
 *
 * Contract common to adlhip_run_length_encode and adlhip_unique_typed: n < 2^32.  d_keys_in is never written.  d_unique_out and the count
 * word (d_num_runs_out / d_num_unique_out) are required, the other outputs optional.  d_unique_out, counts and first_index hold n
 * elements, offsets n + 1, inverse n; with R the number of runs, the elements at R and beyond (offsets: R + 1 and beyond) are NEVER
 * written.  d_keys_in, d_work and every output array are 16-byte aligned, the count word 4-byte aligned; no output (the count word
 * included) may overlap d_keys_in.  n == 0 enqueues one 4-byte clear of the count word and nothing else (only the count word is looked at).
 * A NULL required pointer, a misaligned pointer, an overlap, an unknown key_type, order or key_bytes, and a work buffer one byte short
 * (the message names the needed size) fail before anything is enqueued.  The calls enqueue and return: nothing data-dependent reaches
 * the host (R stays on the device; launch grids depend on n alone), nothing is remembered between calls, all state lives in d_work --
 * whose contents on entry are arbitrary -- and the handle owns no device word of it.  No kernel of the run stage waits on another
 * workgroup, so there is no new fault condition.
 *
 * Work bytes, every part rounded up to 256 bytes, with CUs = adlhip_info.compute_units and kb = bytes per key:
 *   W_runs(n)   = 16 CUs (one head count per workgroup of the largest grid, 4 workgroups per CU) + 4 (n + 1) (offsets, used when counts
 *                 are asked without offsets)
 *   adlhip_run_length_encode_scratch_bytes = W_runs(n)
 *   keys path   = W_runs(n) + n kb (the sorted keys) + n kb (the sort's partner array) + W_keys(n)
 *   index path  = W_runs(n) + n kb (the sorted keys) + 4 n (the argsort's index) + W_argsort(n)
 *   adlhip_unique_scratch_bytes = want_index ? max(keys path, index path) : keys path
 * W_keys / W_argsort = *work_bytes of adlhip_sort_typed_scratch_bytes, mode 0 / mode 2.  The value suffices for every n' <= n. */

/* Run-length encode of keys that are already grouped (no reference counterpart); key_bytes: 4 or 8.  A run is a maximal stretch of
 * adjacent keys with identical bits.  With R runs: d_unique_out[r] = the key of run r, d_offsets_out[r] = its first position and
 * d_offsets_out[R] = n, d_counts_out[r] = its length, *d_num_runs_out = R -- the contract of torch.unique_consecutive, and the
 * segment-start array adlhip_segment_sort takes.  Keys that are grouped but not sorted (A A B A) give one run per stretch (A B A).
 * Three or four launches: the workgroups count the run heads of their chunks (a head is position 0 or a key that differs from the one
 * in front of it), one workgroup scans the counts and writes R, the workgroups walk their chunks again and write the heads where their
 * ranks say, counts are the differences of the offsets. */
int adlhip_run_length_encode_scratch_bytes(adlhip_device* dev, int key_bytes, size_t n, size_t* work_bytes);
int adlhip_run_length_encode(adlhip_device* dev, int key_bytes, const void* d_keys_in, size_t n,
                             void* d_unique_out, uint32_t* d_counts_out_or_null, uint32_t* d_offsets_out_or_null,
                             uint32_t* d_num_runs_out, void* d_work, size_t work_bytes);

/* The distinct keys of d_keys_in in the order of adlhip_sort_keys_typed(key_type, order) (no reference counterpart).  With P the result
 * of adlhip_argsort_typed on the same input, S the sorted keys and off the run starts of S:
 *   d_unique_out[r] = S[off[r]], bit for bit;  d_offsets_out[r] = off[r], d_offsets_out[R] = n;  d_counts_out[r] = off[r + 1] - off[r];
 *   d_first_index_out[r] = P[off[r]] -- the argsort is stable, so this is the LOWEST input position that holds the key, in both orders;
 *   d_inverse_out[i] = the r for which d_keys_in[i] has the bits of d_unique_out[r];  *d_num_unique_out = R.
 * Two paths, the same common outputs bit for bit ("unique.algo"): the keys path, when neither first_index nor inverse is asked, copies
 * the keys into d_work, sorts them there with adlhip_sort_keys_typed and runs the run stage of adlhip_run_length_encode; the index path
 * runs adlhip_argsort_typed into d_work (S and P) and the run stage with P.  want_index of the scratch query: non-zero when
 * first_index or inverse will be asked or "unique.algo" = 1 is set.  As for the typed sorts, a sort that refuses after the copy has
 * been enqueued (knobs changed since the scratch was sized) fails the call with the sort's message. */
int adlhip_unique_scratch_bytes(adlhip_device* dev, int key_type, size_t n, int want_index, size_t* work_bytes);
int adlhip_unique_typed(adlhip_device* dev, int key_type, int order, const void* d_keys_in, size_t n,
                        void* d_unique_out, uint32_t* d_counts_out_or_null, uint32_t* d_offsets_out_or_null,
                        uint32_t* d_first_index_out_or_null, uint32_t* d_inverse_out_or_null,
                        uint32_t* d_num_unique_out, void* d_work, size_t work_bytes);

/* ---- reduce values by key: per-run and per-key sum, min, max (no reference counterpart) ------- */

/* The group-by step behind a sort: with the runs of adlhip_run_length_encode (grouped keys) or the groups of adlhip_unique_typed
 * (unsorted keys), d_reduced_out[r] = op over the values of run / group r -- thrust's reduce_by_key, or torch's
 * unique(return_inverse = True) followed by index_add_ / scatter_reduce_.  value_type is one of the six ADLHIP_KEY_* codes, used as a
 * VALUE type; the key width (4 or 8 bytes) and the value width are independent, every combination is served.
 *
 * op:
 *   ADLHIP_REDUCE_SUM, integer values: wrap-around in the value's width -- signed and unsigned of one width are the same arithmetic --;
 *     the result has the value's type.
 *   ADLHIP_REDUCE_SUM, float values: IEEE adds of the run's elements only, in an unspecified association.  DETERMINISTIC: the same
 *     input, device and knobs give the same bits on every call (no float atomics; the association depends on n and the launch grid
 *     alone).  No identity element stands in for "nothing yet": a run of one element returns that element's bits unchanged (-0,
 *     signalling NaNs and NaN payloads included), a run of -0 only sums to -0.
 *   ADLHIP_REDUCE_MIN / _MAX: taken in the ASCENDING order of the typed sorts -- integers by value, floats by IEEE totalOrder:
 *     -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN --, independent of the `order` argument, which orders the KEYS only.  The result
 *     is the bits of an element of the run, so it is bit-exact.  (torch's amin / amax propagate NaNs instead.)
 */
#define ADLHIP_REDUCE_SUM 0
#define ADLHIP_REDUCE_MIN 1
#define ADLHIP_REDUCE_MAX 2

/* Contract common to adlhip_reduce_runs and adlhip_reduce_by_key_typed, the same as the block above: n < 2^32.  d_keys_in and d_vals_in are
 * never written.  d_unique_out, d_reduced_out and the count word are required, counts and offsets optional.  unique, reduced and counts
 * hold n elements, offsets n + 1; with R the number of runs, the elements at R and beyond (offsets: R + 1 and beyond) are NEVER written.
 * Both inputs, d_work and every output array are 16-byte aligned, the count word 4-byte aligned; no output (the count word included)
 * may overlap d_keys_in or d_vals_in.  n == 0 enqueues one 4-byte clear of the count word and nothing else.  A NULL required pointer, a
 * misaligned pointer, an overlap, an unknown key_bytes, key_type, value_type, op or order, and a work buffer one byte short (the
 * message names the needed size) fail before anything is enqueued.  The calls enqueue and return: nothing data-dependent reaches the
 * host, nothing is remembered between calls, all state lives in d_work -- whose contents on entry are arbitrary -- and the handle owns
 * no device word of it.  No kernel of the reduce stage waits on another workgroup or uses an atomic to global memory.
 *
 * Work bytes, every part rounded up to 256 bytes, with CUs = adlhip_info.compute_units, kb / vb = bytes per key / value:
 *   W_reduce(n) = 16 CUs (one head count per workgroup of the largest grid, 4 workgroups per CU) + 16 CUs (one "chunk has a head" flag
 *                 each) + 32 CUs (one tail aggregate each, 8 bytes whatever vb) + 32 CUs (one carry each) + 4 (n + 1) (offsets, used
 *                 when counts are asked without offsets)
 *   adlhip_reduce_runs_scratch_bytes   = W_reduce(n)
 *   adlhip_reduce_by_key_scratch_bytes = W_reduce(n) + n kb (the sorted keys) + n vb (the values in sorted order) + W_argsort(n)
 * W_argsort = *work_bytes of adlhip_sort_typed_scratch_bytes, mode 2 (= mode 1).  The value suffices for every n' <= n. */

/* Keys that are already grouped (key_bytes: 4 or 8; runs are maximal stretches of identical key bits, grouped but unsorted keys A A B A
 * give three runs): unique, counts, offsets and *d_num_runs_out are exactly what adlhip_run_length_encode gives for the same keys, and
 * d_reduced_out[r] = op over d_vals_in[off[r] .. off[r + 1]).  Three or four launches over tiles of 2048 elements: the workgroups walk
 * their chunks and write head count, head flag and the aggregate behind their last head; one workgroup scans the counts (R) and, segmented
 * by the flags, the aggregates, which gives every chunk the part of its first run that lies in front of it; the workgroups walk their
 * chunks again with a segmented scan per tile -- heads write unique and offsets, run ends write reduced; counts are the differences of
 * the offsets. */
int adlhip_reduce_runs_scratch_bytes(adlhip_device* dev, int key_bytes, int value_type, size_t n, size_t* work_bytes);
int adlhip_reduce_runs(adlhip_device* dev, int key_bytes, const void* d_keys_in, int value_type, int op, const void* d_vals_in, size_t n,
                       void* d_unique_out, void* d_reduced_out, uint32_t* d_counts_out_or_null, uint32_t* d_offsets_out_or_null,
                       uint32_t* d_num_runs_out, void* d_work, size_t work_bytes);

/* Unsorted keys: the groups appear in the order of adlhip_sort_keys_typed(key_type, order), key equality by bits; unique, counts,
 * offsets and *d_num_unique_out are exactly what adlhip_unique_typed gives, and d_reduced_out[r] = op over the values whose key has the
 * bits of d_unique_out[r].  The stable typed pairs sort (what adlhip_sort_pairs_typed runs) reads the caller's arrays and gathers
 * sorted keys and values straight into d_work -- the in-place entry point's copy in and copy back are not needed --, then the reduce
 * stage runs there.  A sort that refuses (knobs changed since the scratch was sized) fails the call with the sort's message. */
int adlhip_reduce_by_key_scratch_bytes(adlhip_device* dev, int key_type, int value_type, size_t n, size_t* work_bytes);
int adlhip_reduce_by_key_typed(adlhip_device* dev, int key_type, int order, const void* d_keys_in, int value_type, int op,
                               const void* d_vals_in, size_t n, void* d_unique_out, void* d_reduced_out,
                               uint32_t* d_counts_out_or_null, uint32_t* d_offsets_out_or_null,
                               uint32_t* d_num_unique_out, void* d_work, size_t work_bytes);

/* ---- typed scans: prefix sum, min and max, plain and by key (no reference counterpart) --------- */

/* thrust's inclusive_scan / exclusive_scan and their _by_key forms; torch's cumsum / cummax / cummin (values only), which has no by-key
 * form.  value_type is one of the six ADLHIP_KEY_* codes, used as a VALUE type; op is ADLHIP_REDUCE_SUM / _MIN / _MAX with the
 * semantics of the reduce block above: integer sums wrap in the value's width; float sums are IEEE adds of the segment's elements only,
 * in an association that depends on n and the launch grid alone, so the same input, device and knobs give the same bits on every call;
 * min and max are taken in ascending totalOrder and return the bits of an element.  key_bytes is 4 or 8; a SEGMENT is a run of
 * identical key bits -- the runs of adlhip_run_length_encode, so grouped but unsorted keys A A B A give three segments.  The plain scan
 * is one segment.  A HEAD is the first element of a segment.
 *
 * Inclusive (exclusive == 0; h_init_or_null must be NULL, an init is refused): d_out[i] = op over the segment's elements up to and
 *   including i.  A segment's first element comes back bit for bit (-0, signalling NaNs and NaN payloads included): no identity element
 *   is ever combined with it.
 * Exclusive (exclusive == 1): with inc[] what the inclusive call writes for the same input, device and knobs,
 *   at a head      d_out[i] = init, bits unchanged; with h_init_or_null == NULL the operator's identity pattern: zero bits for sums, the
 *                  last pattern of the type in ascending order for MIN (+NaN with an all-ones payload for floats, the largest
 *                  integer), the first for MAX;
 *   elsewhere      d_out[i] = inc[i - 1] bit for bit (NULL init), or op(init, inc[i - 1]): ONE operation, init the left operand.
 *   h_init_or_null points to one value of the value type in HOST memory, read at call time, as adlhip_fill_pattern reads its pattern.
 *
 * Contract common to both entry points, as in the reduce block: n < 2^32.  The inputs are never written, except through d_out ==
 * d_vals_in.  d_out holds n elements.  d_keys_in, d_vals_in, d_out and d_work are 16-byte aligned.  d_out may BE d_vals_in (the scan
 * then runs in place and gives the bits of the out-of-place call); it must not overlap d_keys_in and must not partially overlap
 * d_vals_in.  n == 0 succeeds and enqueues nothing (NULL arrays are accepted then).  A NULL or misaligned pointer, a partial overlap,
 * an unknown key_bytes, value_type, op or exclusive, an init with an inclusive scan, and a work buffer one byte short (the message names
 * the needed size) fail before anything is enqueued.  The calls enqueue and return: nothing data-dependent reaches the host, nothing is
 * remembered between calls, all state lives in d_work -- whose contents on entry are arbitrary -- and the handle owns no device word
 * of it.  No kernel of the scan stage waits on another workgroup or uses an atomic to global memory.
 *
 * Work bytes, every part rounded up to 256 bytes, with CUs = adlhip_info.compute_units:
 *   W_scan = 16 CUs (one head count per workgroup of the largest grid, 4 workgroups per CU; written, not used) + 16 CUs (one "chunk has
 *            a head" flag each) + 32 CUs (one aggregate each, 8 bytes whatever the value width) + 32 CUs (one carry each) + 256 (one
 *            word the carry launch writes)
 *   adlhip_scan_typed_scratch_bytes = adlhip_scan_by_key_scratch_bytes = W_scan
 * Nothing is proportional to n: the value suffices for every n' <= n (and beyond).
 *
 * Three launches over tiles of 2048 elements, the reduce stage's structure: the workgroups walk their chunks and write head flag and
 * the aggregate behind their last head; one workgroup scans these, segmented by the flags, which gives every chunk the part of its
 * first segment that lies in front of it; the workgroups walk their chunks again with a segmented scan per tile and write every
 * element.  The values are read twice and written once, the keys read twice. */
int adlhip_scan_typed_scratch_bytes(adlhip_device* dev, int value_type, size_t n, size_t* work_bytes);
int adlhip_scan_typed(adlhip_device* dev, int value_type, int op, int exclusive, const void* h_init_or_null, const void* d_vals_in,
                      void* d_out, size_t n, void* d_work, size_t work_bytes);
int adlhip_scan_by_key_scratch_bytes(adlhip_device* dev, int key_bytes, int value_type, size_t n, size_t* work_bytes);
int adlhip_scan_by_key(adlhip_device* dev, int key_bytes, const void* d_keys_in, int value_type, int op, int exclusive,
                       const void* h_init_or_null, const void* d_vals_in, void* d_out, size_t n, void* d_work, size_t work_bytes);

/* ---- stream compaction: select and partition by flags or by a comparison (no reference counterpart) ---- */

/* The filter behind a sort or a scan: thrust's copy_if / remove_if / stable_partition, cub's DeviceSelect::Flagged / If and
 * DevicePartition, torch's masked_select, nonzero and t[t < x].
 *
 * Predicate.
 *   Flagged: element i is selected when d_flags_in[i] != 0.  Flags are one byte per element, the layout of a torch bool tensor; any
 *     non-zero byte selects.
 *   If: element i is selected when d_keys_in[i] cmp threshold, in the ASCENDING order of the typed sorts -- integers by value, floats by
 *     IEEE totalOrder: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.  EQ / NE are equality of bits, as everywhere else in this
 *     header (so -0 != +0, and a NaN equals the NaN with the same bits).  All six are unsigned comparisons of the code of the key with
 *     the code of the threshold, the code being what adlhip_key_encode(key_type, ADLHIP_ORDER_ASCENDING) gives.  h_threshold points to
 *     one key of key_type in HOST memory, read at call time, as h_init_or_null of the scans is.
 *
 * Result, with S the number of selected elements: *d_num_selected_out = S.  The selected elements appear in input order at [0, S) of
 * every output that is given; d_index_out receives their input positions (torch's nonzero, and the gather index for further columns).
 *   partition == 0: elements at S and beyond are NEVER written.
 *   partition == 1: a stable partition.  The rejected elements follow in input order at [S, n), and every output element is written.
 * item_bytes is 4 or 8; it may be 0, with d_items_in_or_null and d_items_out_or_null NULL, for positions only.  value_bytes is 0 (both
 * value pointers NULL), 4 or 8; the key width and the value width are independent.  With a non-zero width the input array is required,
 * the output array optional (an input without its output is not read).  At least one output array must be given.  Items, keys and
 * values are copied bit for bit.
 *
 * Contract, as in the unique and reduce blocks: n < 2^32.  The inputs are never written.  Every output array holds n elements.  Every
 * array and d_work are 16-byte aligned, the count word 4-byte aligned; no output (the count word included) may overlap an input.
 * n == 0 enqueues one 4-byte clear of the count word and nothing else.  A NULL required pointer (h_threshold included), a misaligned
 * pointer, an overlap, an unknown item_bytes, value_bytes, key_type, cmp or partition, no output at all, and a work buffer one byte
 * short (the message names the needed size) fail before anything is enqueued.  The calls enqueue and return: nothing data-dependent
 * reaches the host (S stays on the device; launch grids depend on n alone), nothing is remembered between calls, all state lives in
 * d_work -- whose contents on entry are arbitrary -- and the handle owns no device word of it.  No kernel waits on another workgroup
 * or uses an atomic to global memory.
 *
 * Work bytes, with CUs = adlhip_info.compute_units:
 *   adlhip_compact_scratch_bytes = 16 CUs rounded up to 256 (one count per workgroup of the largest grid, 4 workgroups per CU)
 * Nothing is proportional to n: the value suffices for every n.
 *
 * Three launches over tiles of 2048 elements: the workgroups count the selected elements of their chunks, one workgroup scans the
 * counts and writes S, the workgroups walk their chunks again, rank every element with a workgroup scan per tile, put the tile in rank
 * order in LDS and store it where the ranks say (a rejected element of a partition: S + its position - the selected elements in
 * front of it).  The predicate's input is read twice, everything else once. */
#define ADLHIP_CMP_LT 0
#define ADLHIP_CMP_LE 1
#define ADLHIP_CMP_GT 2
#define ADLHIP_CMP_GE 3
#define ADLHIP_CMP_EQ 4
#define ADLHIP_CMP_NE 5
int adlhip_compact_scratch_bytes(adlhip_device* dev, size_t n, size_t* work_bytes);
int adlhip_compact_flagged(adlhip_device* dev, int item_bytes, const void* d_items_in_or_null, const uint8_t* d_flags_in, size_t n,
                           int partition, void* d_items_out_or_null, uint32_t* d_index_out_or_null,
                           uint32_t* d_num_selected_out, void* d_work, size_t work_bytes);
int adlhip_compact_if_typed(adlhip_device* dev, int key_type, int cmp, const void* h_threshold, const void* d_keys_in,
                            int value_bytes, const void* d_vals_in_or_null, size_t n, int partition,
                            void* d_keys_out_or_null, void* d_vals_out_or_null, uint32_t* d_index_out_or_null,
                            uint32_t* d_num_selected_out, void* d_work, size_t work_bytes);

/* ---- histograms: bin counts by edges and bincount (no reference counterpart) ---- */

/* How many keys fall in each bin: cub's DeviceHistogram::HistogramRange, numpy.histogram with an array of edges, torch.histc and
 * torch.bincount.
 *
 * Range (adlhip_histogram_range_typed).  d_edges_in holds num_bins + 1 keys of key_type in DEVICE memory, non-decreasing in the
 *   ASCENDING order of the typed sorts -- integers by value, floats by IEEE totalOrder: -NaN < -inf < ... < -0 < +0 < ... < +inf <
 *   +NaN.  Bin b counts the keys with edge[b] <= key < edge[b + 1]; both are unsigned comparisons of the codes that
 *   adlhip_key_encode(key_type, ADLHIP_ORDER_ASCENDING) gives, exactly as adlhip_compact_if_typed compares: -0 is below +0, NaNs sit
 *   at the two ends and are counted only where the edges reach them, nothing is compared as a float and nothing is divided.  Keys
 *   outside the edges are ignored.  Repeated edges give empty bins; a key equal to a repeated edge belongs to the last of them.
 *   include_upper == 1 closes the last bin, as numpy does: a key whose bits equal edge[num_bins] counts in the last bin b with
 *   edge[b] < edge[num_bins] (in bin num_bins - 1 if all edges are equal).  1 <= num_bins <= ADLHIP_HISTOGRAM_MAX_RANGE_BINS: 8-byte
 *   edges and the counters together fit LDS several times over.  Edges that are not sorted give unspecified counts and no access
 *   outside the arrays: the search's result is always clamped to a bin or to "ignored".
 * Bincount (adlhip_bincount_typed).  Integer key types only (U32, I32, U64, I64).  counts[v] is the number of keys with value v for
 *   0 <= v < num_bins; negative keys and keys >= num_bins are ignored.  1 <= num_bins < 2^31.
 *
 * Contract, as in the neighbouring blocks: n < 2^32.  The inputs are never written.  Every one of the num_bins counters is written,
 * with zeros where nothing fell, and nothing beyond them.  Every array and d_work are 16-byte aligned; no output may overlap an
 * input.  n == 0 enqueues one clear of the counters and nothing else; d_keys_in, d_work and work_bytes are then not looked at (an empty
 * array has no address to check), as in the neighbouring blocks, while everything else is checked as for any n.  A NULL pointer, a misaligned pointer, an overlap, an unknown
 * key type (bincount: a float type), an out-of-range num_bins, an include_upper other than 0 or 1 and a work buffer one byte short
 * (the message names the needed size) fail before anything is enqueued.  The calls enqueue and return: nothing data-dependent
 * reaches the host, launch grids depend on n and num_bins alone, nothing is remembered between calls, all state lives in d_work --
 * whose contents on entry are arbitrary.  No kernel waits on another workgroup or uses an atomic to global memory.  Counts are
 * exact and identical from run to run.
 *
 * LDS path (range; bincount up to the limit "debug.histogram_lds_bins" reports, 8192 bins): two launches over tiles of
 * ADLHIP_HISTOGRAM_TILE elements.  The workgroups count the keys of their chunks with LDS atomics into private tables (range mode: a
 * branch-free binary search over the edges' codes in LDS) and store their tables as rows of d_work; a second launch sums the rows.
 * The keys are read once.  Sorted path (bincount above the limit): a copy of the keys in d_work is sorted as unsigned numbers by
 * what adlhip_sort_keys_typed runs, the counters are cleared, and two launches over the sorted keys turn the boundaries of the runs
 * into counts (run heads store -i, run ends add i + 1: one writer per word per launch).
 *
 * Work bytes (adlhip_histogram_scratch_bytes; by_edges: 1 for the range mode, 0 for bincount), with CUs = adlhip_info.compute_units:
 *   LDS path     G x num_bins x 4 rounded up to 256, G = 4 CUs x 2048 / num_bins kept within [2 CUs, 4 CUs]: one row per workgroup of
 *                the largest grid, which shrinks as the bins grow (at most 16 MiB at 256 CUs); nothing proportional to n
 *   sorted path  2 x (n keys rounded up to 256) + the work of the unsigned keys sort of n keys
 * The value holds for the knobs as they are when it is asked. */
#define ADLHIP_HISTOGRAM_MAX_RANGE_BINS 4096
#define ADLHIP_HISTOGRAM_TILE 2048
int adlhip_histogram_scratch_bytes(adlhip_device* dev, int key_type, size_t n, size_t num_bins, int by_edges, size_t* work_bytes);
int adlhip_histogram_range_typed(adlhip_device* dev, int key_type, const void* d_keys_in, size_t n, const void* d_edges_in,
                                 size_t num_bins, int include_upper, uint32_t* d_counts_out, void* d_work, size_t work_bytes);
int adlhip_bincount_typed(adlhip_device* dev, int key_type, const void* d_keys_in, size_t n, size_t num_bins, uint32_t* d_counts_out,
                          void* d_work, size_t work_bytes);

/* ---- merge of sorted sequences (no reference counterpart) ---- */

/* The stable merge of two sequences that are already sorted: thrust's merge / merge_by_key, cub's DeviceMerge, and what
 * torch.sort(torch.cat((a, b)), stable=True) gives for sorted a and b -- with one read of every input element and one write of every
 * output element instead of a sort of the concatenation.
 *
 * Order.  A (d_keys_a, na keys) and B (d_keys_b, nb keys) are each sorted in `order` in the order of the typed sorts: integers by value,
 *   floats by IEEE totalOrder (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN), descending the reverse.  Precisely: a sequence is
 *   sorted when the codes adlhip_key_encode(key_type, order) gives for its elements are non-decreasing as unsigned numbers.
 * Result.  The stable merge of the na + nb elements: the elements of one input keep their order, and where codes are equal every
 *   element of A comes before every element of B, in both orders.  This is, bit for bit, what the stable typed sort
 *   (adlhip_sort_pairs_typed, adlhip_argsort_typed) gives for the concatenation A || B.
 *     d_keys_out[j]   the j-th key, bit for bit (NaN payloads, -0)
 *     d_vals_out[j]   its value (value_bytes 4 or 8: d_vals_a, d_vals_b and d_vals_out are all given; value_bytes 0: all NULL)
 *     d_index_out[j]  its position in A || B: i for A[i], na + i for B[i]
 *   At least one output is given; each holds na + nb elements and every one of them is written.
 *
 * Contract.  na + nb <= 0xFFF00000, the limit of the sorts; either count may be 0 (the array of an empty input is not looked at).
 * The inputs are never written; A
 * and B may overlap or be the same array.  No output may overlap an input, another output or d_work.  The outputs and d_work are
 * 16-byte aligned.  The INPUTS need only the alignment of their element (4 or 8 bytes; values: value_bytes): a tile's share of A
 * and of B starts at an arbitrary element anyway, so a view that starts at any element of a larger array is merged where it lies.
 * na + nb == 0 succeeds and enqueues nothing.  A NULL required pointer, a misaligned pointer, an overlap, an unknown key_type, order
 * or value_bytes, value arrays that do not agree with value_bytes, no output at all, na + nb beyond the limit and a work buffer one byte
 * short (the message names the needed size and adlhip_merge_scratch_bytes) fail before anything is enqueued, each with a message
 * that names the argument.  The call enqueues and returns: nothing data-dependent reaches the host (launch grids depend on na + nb
 * alone), nothing is remembered between calls, all state lives in d_work -- whose contents on entry are arbitrary -- and the handle
 * owns no device word of it.  No kernel waits on another workgroup or uses an atomic to global memory.
 *
 * Inputs that are NOT sorted: the order of the output is unspecified (elements may even repeat or be missing), but the call
 * succeeds and terminates, every read stays inside [A, A + na) and [B, B + nb), and every write inside the na + nb elements of the
 * outputs (merge_kernels.hpp proves it: every search result lies in its search range whatever the comparisons answer, and a tile's
 * share of A is clamped to the tile).
 *
 * Work bytes:
 *   adlhip_merge_scratch_bytes = 4 x (tiles + 1) rounded up to 256, tiles = ceil((na + nb) / ADLHIP_MERGE_TILE): the number of
 *   elements of A in front of every tile boundary.  key_type and value_bytes are checked and do not change the value.
 *
 * Two launches over tiles of ADLHIP_MERGE_TILE output elements: one thread per tile boundary searches its diagonal of the merge
 * path; then the workgroups take tiles in turns -- the tile's share of A and B goes to LDS as codes, every thread finds the
 * diagonal of its 8 outputs there and merges them, the tile is put in output order in LDS and stored densely. */
#define ADLHIP_MERGE_TILE 2048
int adlhip_merge_scratch_bytes(adlhip_device* dev, int key_type, int value_bytes, size_t na, size_t nb, size_t* work_bytes);
int adlhip_merge_typed(adlhip_device* dev, int key_type, int order,
                       const void* d_keys_a, const void* d_vals_a_or_null, size_t na,
                       const void* d_keys_b, const void* d_vals_b_or_null, size_t nb,
                       int value_bytes, void* d_keys_out_or_null, void* d_vals_out_or_null, uint32_t* d_index_out_or_null,
                       void* d_work, size_t work_bytes);

/* ---- set operations on sorted sequences (no reference counterpart) ---- */

/* Intersection, union, difference and symmetric difference of two sequences that are already sorted: thrust's set_intersection /
 * set_union / set_difference / set_symmetric_difference and their _by_key forms, and -- for inputs without duplicates -- numpy's
 * intersect1d / union1d / setdiff1d / setxor1d, without merging, counting runs and compacting.
 *
 * Order.  A (d_keys_a, na keys) and B (d_keys_b, nb keys) are each sorted in `order` as adlhip_merge_typed asks: the codes
 *   adlhip_key_encode(key_type, order) gives for their elements are non-decreasing.  Keys are equal when their bits are: -0 is not
 *   +0, NaNs are equal by payload.
 * Result.  Duplicates are allowed, with thrust's multiset semantics.  For a key x that occurs m times in A and n times in B:
 *     op                                    copies of x     which elements
 *     ADLHIP_SETOP_INTERSECTION             min(m, n)       the first min(m, n) of A's
 *     ADLHIP_SETOP_UNION                    max(m, n)       all of A's, then the last max(n - m, 0) of B's
 *     ADLHIP_SETOP_DIFFERENCE               max(m - n, 0)   the last max(m - n, 0) of A's
 *     ADLHIP_SETOP_SYMMETRIC_DIFFERENCE     |m - n|         the last m - n of A's, or the last n - m of B's
 *   That is, with r an element's rank inside its own input's run of x: an element of A is kept by intersection when r < n, by
 *   difference and symmetric difference when r >= n, by union always; an element of B is kept by union and symmetric difference when
 *   r >= m, never otherwise.  The result is the kept elements in the order of the stable merge (ties: A before B): it is sorted in
 *   `order`, and it is exactly the subsequence these rules select of what adlhip_merge_typed returns for the same inputs.
 *     *d_num_out      S, the number of result elements; it stays on the device
 *     d_keys_out[j]   the j-th kept key, bit for bit, j < S
 *     d_vals_out[j]   the kept element's own value: A's for an element of A, B's for one of B (value_bytes 4 or 8: d_vals_a, d_vals_b
 *                     and d_vals_out are all given; value_bytes 0: all NULL)
 *     d_index_out[j]  its position in A || B: i for A[i], na + i for B[i]
 *   At least one output besides the count word is given.  Each given output holds cap elements: cap = na for intersection and
 *   difference, na + nb for union and symmetric difference.  Elements at S and beyond are never written.
 *
 * Contract.  That of adlhip_merge_typed: na + nb <= 0xFFF00000; either count may be 0 (the array of an empty input is not looked at).  The
 * inputs are never written, need only the alignment of their element and may overlap or be the same array.  No output, nor the count
 * word, nor d_work may overlap an input or one another.  The outputs and d_work are 16-byte aligned, the count word 4-byte aligned.
 * na + nb == 0 succeeds and enqueues only a clear of the count word (d_work may then be NULL).  A NULL required pointer, a misaligned
 * pointer, an overlap, an unknown key_type, order, op or value_bytes, value arrays that do not agree with value_bytes, no output at
 * all, na + nb beyond the limit and a work buffer one byte short (the message names the needed size and adlhip_set_op_scratch_bytes) fail
 * before anything is enqueued, each with a message that names the argument.  The call enqueues and returns: nothing data-dependent
 * reaches the host (launch grids depend on na + nb alone), nothing is remembered between calls, all state lives in d_work -- whose
 * contents on entry are arbitrary.  No kernel waits on another workgroup or uses an atomic to global memory.
 *
 * Inputs that are NOT sorted: the result is unspecified, but the call succeeds and terminates, every read stays inside
 * [A, A + na) and [B, B + nb), *d_num_out <= cap and no write lands at cap or beyond (setop_kernels.hpp proves the reads and clamps
 * the writes and the count).
 *
 * Work bytes:
 *   adlhip_set_op_scratch_bytes = (4 x 8 x CUs rounded up to 256) + (4 x (tiles + 1) rounded up to 256),
 *   tiles = ceil((na + nb) / ADLHIP_SETOP_TILE): the number of kept elements per workgroup, and the number of elements of A in front
 *   of every tile boundary.  key_type and value_bytes are checked and do not change the value.
 *
 * Four launches over tiles of ADLHIP_SETOP_TILE elements of the merged order: the merge's partition; a count -- every workgroup
 * merges its chunk of tiles in LDS as adlhip_merge_typed does and decides per element whether it is kept, by one look at the other
 * input at the element's rank in its run; a scan of the workgroups' counts, whose total is S; and an emit that repeats the walk,
 * ranks the kept elements of a tile with a workgroup scan, puts them in rank order in LDS and stores them densely. */
#define ADLHIP_SETOP_TILE 2048
#define ADLHIP_SETOP_INTERSECTION 0
#define ADLHIP_SETOP_UNION 1
#define ADLHIP_SETOP_DIFFERENCE 2
#define ADLHIP_SETOP_SYMMETRIC_DIFFERENCE 3
int adlhip_set_op_scratch_bytes(adlhip_device* dev, int key_type, int value_bytes, size_t na, size_t nb, size_t* work_bytes);
int adlhip_set_op_typed(adlhip_device* dev, int key_type, int order, int op,
                        const void* d_keys_a, const void* d_vals_a_or_null, size_t na,
                        const void* d_keys_b, const void* d_vals_b_or_null, size_t nb,
                        int value_bytes, void* d_keys_out_or_null, void* d_vals_out_or_null, uint32_t* d_index_out_or_null,
                        uint32_t* d_num_out, void* d_work, size_t work_bytes);

/* ---- sorted search (no reference counterpart) ---- */

/* The vectorised binary search: for every one of n needles its lower or upper bound in a sequence of m elements that is already
 * sorted.  thrust's lower_bound / upper_bound on vectors of values, numpy.searchsorted, torch.searchsorted and torch.bucketize.
 *
 * Order.  d_sorted (m keys) is sorted in `order` as adlhip_merge_typed asks.  Precisely, with c(x) = the code
 *   adlhip_key_encode(key_type, order) gives for x -- integers by value, floats by IEEE totalOrder on bits (-NaN < -inf < ... < -0 <
 *   +0 < ... < +inf < +NaN: -0 is below +0 and NaNs sit at the two ends), descending the complement -- the codes of its elements are
 *   non-decreasing as unsigned numbers.
 * Result.
 *     side ADLHIP_SEARCH_LEFT    d_pos_out[i] = the number of elements of d_sorted whose code is below c(d_needles[i])
 *     side ADLHIP_SEARCH_RIGHT   d_pos_out[i] = the number of elements whose code is below or equal to it
 *   always in [0, m]: where the needle would be inserted in front of (LEFT) or behind (RIGHT) its equals to keep the sequence sorted.
 *   All six key types and both orders.
 * Relation to the merge.  For sorted A and B, adlhip_merge_typed puts A[i] at i + LEFT_B(A[i]) and B[j] at j + RIGHT_A(B[j]), where
 *   LEFT_B / RIGHT_A are this search in B / in A: ties take A.
 *
 * Contract.  m < 2^32 and n < 2^32.  The inputs are never written; d_sorted and d_needles may overlap or be the same array.
 * d_pos_out overlaps no input.  d_needles and d_pos_out are 16-byte aligned.  d_sorted needs only the alignment of its element (4
 * or 8 bytes), because it is gathered, never streamed: a view that starts at any element of a larger array is searched where it
 * lies.  Every one of the n positions is written and nothing beyond them.  n == 0 succeeds and enqueues nothing.  m == 0 writes n
 * zeros, and d_sorted is then not looked at (it may be NULL).  A NULL pointer, a misaligned pointer, an overlap of d_pos_out with
 * an input, an unknown key_type, order or side, and m or n >= 2^32 fail before anything is enqueued, each with a message that
 * names the argument.  There is no work buffer: the call keeps no state, nothing is remembered between calls.  The call enqueues
 * and returns: nothing data-dependent reaches the host (the launch grid depends on n and m alone).  The kernel does not wait on
 * another workgroup and uses no atomic to global memory.
 *
 * A sequence that is NOT sorted: the positions are unspecified, but each lies in [0, m], the call succeeds and terminates, every
 * read stays inside [d_sorted, d_sorted + m) and the n needles, and every write inside the n positions (search_kernels.hpp proves
 * it: every probe index is clamped to the table or the sequence, whatever the comparisons answer, and a position only ever moves
 * to a count that is at most the length searched).
 *
 * One launch over tiles of ADLHIP_SEARCH_TILE needles, 8 consecutive needles per thread searched side by side.  Every workgroup
 * first puts a table of at most C = 4096 codes in LDS ("debug.search_lds_keys" reports C): for m <= C the whole sequence, and the
 * search ends there; for larger m the last element of every block of ceil(m / C) elements, and the search goes on inside the one
 * block the table points to with a branch-free search on global memory whose probe index is clamped to [0, m). */
#define ADLHIP_SEARCH_TILE 2048
#define ADLHIP_SEARCH_LEFT 0
#define ADLHIP_SEARCH_RIGHT 1
int adlhip_search_sorted_typed(adlhip_device* dev, int key_type, int order, int side,
                               const void* d_sorted, size_t m, const void* d_needles, size_t n,
                               uint32_t* d_pos_out);

/* ---- expansion of runs and join of sorted sequences (no reference counterpart) ---- */

/* adlhip_expand_runs: run-length decode, the inverse of adlhip_run_length_encode; torch.repeat_interleave; thrust's "expand".
 *
 * Result.  With start = the exclusive scan of the num_runs counts and T = their sum as a 64-bit number:
 *     *d_num_out      T.  It stays on the device and is never clamped, so the caller learns the capacity it needs
 *   and for every row o < min(T, cap), in whichever of the outputs is given:
 *     d_run_out[o]    the run i with start[i] <= o < start[i] + d_counts_in[i]
 *     d_rank_out[o]   o - start[i]
 *     d_vals_out[o]   d_vals_in[i] (value_bytes 4 or 8; value_bytes 0: both value pointers are NULL)
 *   Nothing is written at or beyond min(T, cap).  cap == 0 with no output is the counting call: only T is produced.
 *
 * Contract.  num_runs + cap <= 0xFFF00000.  The inputs are never written and need only the alignment of their element.  The outputs,
 * the count word and d_work overlap no input and not one another; the outputs and d_work are 16-byte aligned, the count word 8-byte
 * aligned.  num_runs == 0 enqueues only the clear of the count word (d_work may then be NULL).  A NULL required pointer, a
 * misaligned pointer, an overlap, an unknown value_bytes, value arrays that do not agree with value_bytes, outputs given with
 * cap == 0, cap > 0 with no output, sizes beyond the limit and a work buffer one byte short (the message names the needed size and
 * adlhip_expand_scratch_bytes) fail before anything is enqueued, each with a message that names the argument.  The call enqueues and
 * returns: nothing data-dependent reaches the host (launch grids depend on num_runs and cap alone), all state lives in d_work --
 * whose contents on entry are arbitrary.  No kernel waits on another workgroup or uses an atomic to global memory.
 *
 * Work bytes:
 *   adlhip_expand_scratch_bytes = (8 x 8 x CUs rounded up to 256) + (4 x num_runs rounded up to 256) + (4 x (tiles + 1) rounded up to 256),
 *   tiles = ceil((num_runs + cap) / ADLHIP_JOIN_TILE): the rows per workgroup, the start of every run (saturated at cap), and the
 *   number of runs in front of every tile boundary.
 *
 * Five launches (two for the counting call): the sums of the workgroups' chunks of counts; their scan, whose total is T; the starts;
 * and a merge path of the starts with the row numbers, cut into tiles of ADLHIP_JOIN_TILE runs plus rows -- a partition and a row
 * kernel that holds a tile's starts in LDS and stores its rows densely.  A tile is bounded whatever the counts: ten thousand zero
 * counts in a row and one count of a million cost what their number of items costs. */
#define ADLHIP_JOIN_TILE 2048
int adlhip_expand_scratch_bytes(adlhip_device* dev, size_t num_runs, size_t cap, size_t* work_bytes);
int adlhip_expand_runs(adlhip_device* dev, const uint32_t* d_counts_in, size_t num_runs,
                       int value_bytes, const void* d_vals_in_or_null, size_t cap,
                       uint32_t* d_run_out_or_null, uint32_t* d_rank_out_or_null, void* d_vals_out_or_null,
                       uint64_t* d_num_out, void* d_work, size_t work_bytes);

/* adlhip_join_sorted_typed: the join of two sequences that are already sorted, as pairs of positions: all m x n pairs of a key that
 * occurs m times in A and n times in B, where ADLHIP_SETOP_INTERSECTION keeps min(m, n) elements.
 *
 * Order.  A (d_keys_a, na keys) and B (d_keys_b, nb keys) are each sorted in `order` as adlhip_set_op_typed asks: the codes
 *   adlhip_key_encode(key_type, order) gives for their elements are non-decreasing.  Keys are equal when their bits are: -0 is not
 *   +0, NaNs are equal by payload.  All six key types and both orders.
 * Result.  For A[i] let lo_i be the number of codes of B below its code and m_i the number equal to it.  A[i] contributes
 *     kind                rows                   content
 *     ADLHIP_JOIN_INNER   m_i                    (i, lo_i + r), r = 0 .. m_i - 1
 *     ADLHIP_JOIN_LEFT    max(m_i, 1)            as INNER; where m_i == 0, the one row (i, ADLHIP_JOIN_NONE)
 *     ADLHIP_JOIN_SEMI    min(m_i, 1)            (i, lo_i)
 *     ADLHIP_JOIN_ANTI    m_i == 0 ? 1 : 0       (i, ADLHIP_JOIN_NONE)
 *   and the rows are ordered by i, then by the position in B: the result is fixed bit for bit.
 *     *d_num_out            T, the exact 64-bit number of rows.  It can reach na x nb; it stays on the device and is never clamped
 *     d_index_a_out[o]      the position in A of row o, o < min(T, cap)
 *     d_index_b_out[o]      its position in B, or ADLHIP_JOIN_NONE
 *   Rows below min(T, cap) are written to whichever of the two index outputs is given; nothing is written at or beyond that.
 *   cap == 0 with both outputs NULL is the counting call: it skips the expansion launches.
 *
 * Contract.  na + nb <= 0xFFF00000 and na + cap <= 0xFFF00000.  The inputs are never written, need only the alignment of their element
 * -- a view that starts at any element of a larger array is joined where it lies -- and may overlap or be the same array.  The
 * outputs, the count word and d_work overlap no input and not one another; the outputs and d_work are 16-byte aligned, the count
 * word 8-byte aligned.  na == 0 enqueues only the clear of the count word (d_work may then be NULL).  nb == 0 is legal (d_keys_b is
 * then not looked at): INNER and SEMI give 0 rows, LEFT and ANTI na rows.  A NULL required pointer, a misaligned pointer, an
 * overlap, an unknown key_type, order or kind, outputs given with cap == 0, cap > 0 with no output, sizes beyond the limits and a
 * work buffer one byte short (the message names the needed size and adlhip_join_scratch_bytes) fail before anything is enqueued, each
 * with a message that names the argument.  The call enqueues and returns: nothing data-dependent reaches the host (launch grids
 * depend on na, nb and cap alone), nothing is remembered between calls, all state lives in d_work -- whose contents on entry are
 * arbitrary.  No kernel waits on another workgroup or uses an atomic to global memory.
 *
 * Inputs that are NOT sorted: the rows and the count are unspecified, but the call succeeds and terminates, every read stays inside
 * [A, A + na) and [B, B + nb), every written index_a is below na, every written index_b is below nb or is ADLHIP_JOIN_NONE, and no
 * write lands at cap or beyond (join_kernels.hpp proves it: m_i is clamped to hi > lo ? hi - lo : 0, and the rows are expanded from
 * the library's own scan of the counts).
 *
 * Work bytes:
 *   adlhip_join_scratch_bytes = (8 x 8 x CUs rounded up to 256) + 2 x (4 x na rounded up to 256) + (4 x (tiles + 1) rounded up to 256),
 *   tiles = ceil((na + cap) / ADLHIP_JOIN_TILE): the rows per workgroup, lo_i and the start of the rows of every element of A (saturated at
 *   cap), and the number of elements of A in front of every tile boundary.  key_type and nb are checked and do not change the value.
 *
 * Five launches (two for the counting call).  The bounds: over tiles of ADLHIP_JOIN_TILE elements of A, every thread searches its 8
 * elements in B for both sides as adlhip_search_sorted_typed does, from one table of at most 16 KiB of codes in LDS (4096 4-byte or
 * 2048 8-byte codes, fewer where "debug.search_lds_keys" says so), and writes lo_i and the rows of A[i]; then the scan, the starts,
 * the partition and the row kernel of adlhip_expand_runs, which adds lo_i to the rank. */
#define ADLHIP_JOIN_INNER 0
#define ADLHIP_JOIN_LEFT  1
#define ADLHIP_JOIN_SEMI  2
#define ADLHIP_JOIN_ANTI  3
#define ADLHIP_JOIN_NONE  0xFFFFFFFFu
int adlhip_join_scratch_bytes(adlhip_device* dev, int key_type, size_t na, size_t nb, size_t cap, size_t* work_bytes);
int adlhip_join_sorted_typed(adlhip_device* dev, int key_type, int order, int kind,
                             const void* d_keys_a, size_t na, const void* d_keys_b, size_t nb, size_t cap,
                             uint32_t* d_index_a_out_or_null, uint32_t* d_index_b_out_or_null,
                             uint64_t* d_num_out, void* d_work, size_t work_bytes);

/* ---- segments finished in LDS (no reference counterpart) ------------------------------------- */

/* Sorts, stably and in place, every segment [d_seg_start[s], d_seg_start[s + 1]) of an array of u32 keys
 * (ADLHIP_ELEM_U32) or {key, value} pairs (ADLHIP_ELEM_KV32) by the low `low_bits` bits of its keys: one
 * workgroup per segment, the segment lives in LDS, one read and one write of global memory.  It is the
 * finishing pass of the hybrid sort ("sort.algo" = 2: two MSD passes of the kind
 * Tahoe/ClKernels/RadixSort32Kernels.cl:493-631 implements per digit, then this) and usable on its own.
 * d_seg_start: num_segments + 1 ascending element offsets in device memory.  max_segment: the caller's bound
 * on the largest segment (selects the LDS tile): at most 16384 keys / 8192 pairs for low_bits <= 24, half of
 * that up to 27 bits.  A segment that exceeds the tile is left unsorted and raises the device fault word
 * (reported by adlhip_sync / adlhip_fault_check). */
int adlhip_segment_sort(adlhip_device* dev, int elem_kind, void* d_data, const uint32_t* d_seg_start,
                        size_t num_segments, size_t max_segment, int low_bits);

/* Pprims::scan(const Device*, Buffer<int>& dst, const Buffer<int>& src, int n, u32* sumOut=0)
 * -- Pprims.h:35, Pprims.cpp:122-179.  Exclusive prefix sum, 32-bit wrap-around.  dst may equal src.
 * h_sum_or_null: when non-NULL the grand total is copied there (stream-ordered; valid after
 * adlhip_sync(), like the reference's non-blocking read at Pprims.cpp:164-167).  No n < 1,048,576
 * limit (the reference silently returns for numBlocks >= 4096, Pprims.cpp:134-138); n <= 0xFFF00000, the limit of the sorts,
 * beyond which both functions fail. */
int adlhip_scan_scratch_bytes(adlhip_device* dev, size_t n, size_t* work_bytes);
int adlhip_exclusive_scan_u32(adlhip_device* dev, uint32_t* d_dst, const uint32_t* d_src,
                              void* d_work, size_t work_bytes, size_t n, uint32_t* h_sum_or_null);

/* ---- multi-GPU helper: MSB-bucket partition (no reference counterpart) ----- */

/* Stable partition of n u32 keys into `num_buckets` (<= 256, power of two) contiguous segments by
 * their top log2(num_buckets) bits; d_counts_out[num_buckets] (u32) receives the segment sizes.
 * This is one radix pass on the most significant digit: the send side of the all-to-all exchange. */
int adlhip_partition_msb_u32(adlhip_device* dev, const uint32_t* d_keys_in, uint32_t* d_keys_out,
                             uint32_t* d_counts_out, void* d_work, size_t work_bytes,
                             size_t n, int num_buckets);
/* Same for n {u32 key, u32 value} pairs (the element of Pprims::radixSort(Buffer<uint2>), Pprims.h:38): partitioned by
 * the top bits of the KEY, stable, values travel with their keys. */
int adlhip_partition_msb_kv32(adlhip_device* dev, const void* d_pairs_in, void* d_pairs_out,
                              uint32_t* d_counts_out, void* d_work, size_t work_bytes,
                              size_t n, int num_buckets);

/* The same pass with the 256 top-byte totals handed out instead of folded: out = in, stably ordered by the key's
 * bits 24..31; d_totals256_out[b] (u32) = number of keys whose top byte is b.  The sharded sort all-reduces these
 * totals over the ranks and cuts the byte range into G contiguous pieces of near-equal population (balanced
 * splitters); any such cut yields G contiguous send segments of this output. */
int adlhip_partition_top_byte_u32(adlhip_device* dev, const uint32_t* d_keys_in, uint32_t* d_keys_out,
                                  uint32_t* d_totals256_out, void* d_work, size_t work_bytes, size_t n);
int adlhip_partition_top_byte_kv32(adlhip_device* dev, const void* d_pairs_in, void* d_pairs_out,
                                   uint32_t* d_totals256_out, void* d_work, size_t work_bytes, size_t n);

/* ---- sharded sort: ONE process, G devices (no reference counterpart) ------------------------
 *
 * The reference's API language is C++ (Tahoe/ParallelPrimitives/Pprims.h:35-41) and it drives one device
 * (Adl/Adl.h:90-94).  A group owns one adlhip_device per GPU and one RCCL communicator per device
 * (ncclCommInitAll; RCCL is loaded with dlopen on first use).  adlhip_sharded_sort_* sorts G shards that live
 * on the G devices into ONE global order: rank r ends up with a contiguous, ascending slice and the slices in
 * rank order are the sorted whole (pairs: stable in (source rank, position) order).  Steps: stable partition by
 * the top byte on every device (adlhip_partition_top_byte_*), ONE host synchronisation that brings the G x 256
 * totals to the host, balanced splitters (contiguous top-byte ranges of near-equal population; a rank's share
 * exceeds the mean by at most one byte value's population), one grouped ncclSend/ncclRecv exchange (every pair
 * of GPUs of a node has its own xGMI link), local sort.  The call returns with the exchange and the local sorts
 * ENQUEUED on the devices' streams: results are valid after adlhip_sync() on each device of the group.
 * Like every handle, a group must be driven by one host thread at a time. */
typedef struct adlhip_group adlhip_group;

/* device_indices: num_devices distinct HIP device indices, or NULL for 0 .. num_devices-1. */
int adlhip_group_create(const int* device_indices, int num_devices, adlhip_group** out);
/* Frees the group's scratch, communicators and device handles.  Fails (like adlhip_device_destroy,
 * Adl/Adl.inl:100-105) while the caller still holds memory allocated from one of its devices. */
int adlhip_group_destroy(adlhip_group* group);
int adlhip_group_size(adlhip_group* group);
/* The handle of rank `rank` (allocate the shards and outputs with it; NULL if out of range). */
adlhip_device* adlhip_group_device(adlhip_group* group, int rank);
/* Top-byte boundaries of the last sharded sort: bounds_out[G + 1], rank r owns top bytes [b[r], b[r+1]). */
int adlhip_group_last_bounds(adlhip_group* group, int* bounds_out);

/* d_shards_in[r]: n_in[r] keys on device r (left intact).  d_out[r]: room for out_capacity[r] keys on device r;
 * n_out[r] receives the size of rank r's slice.  If a slice does not fit, the call fails before anything is
 * exchanged and n_out holds the required sizes (1.25 x the mean + slack is enough unless one byte value dominates). */
int adlhip_sharded_sort_u32(adlhip_group* group, uint32_t* const* d_shards_in, const size_t* n_in,
                            uint32_t* const* d_out, const size_t* out_capacity, size_t* n_out);
/* Same for {u32 key, u32 value} pairs (8-byte elements, key in the low dword; Pprims.h:38). */
int adlhip_sharded_sort_kv32(adlhip_group* group, void* const* d_shards_in, const size_t* n_in,
                             void* const* d_out, const size_t* out_capacity, size_t* n_out);

/* ---- synthetic inputs: generated in place, reproducible by index ---------- */

/* key32(i) = hi32(splitmix64(seed*0x9E3779B97F4A7C15 + first_index + i)); key64 = the full 64 bits;
 * KV32 pair = {key32(i), value = (u32)(first_index + i)} (value = original index, as
 * UnitTest/main.cpp:152 does, so stability is checkable).  elem_kind: ADLHIP_ELEM_*. */
int adlhip_generate_keys(adlhip_device* dev, int elem_kind, void* dptr, size_t n, uint64_t seed,
                         uint64_t first_index);

/* ---- knobs ---------------------------------------------------------------------------------- */

/* Integer tunables, by name.  Unknown names fail.  Current names:
 *   "sort.algo"        -1 [default] = by size: n <= 16384 one workgroup does the whole sort in one launch;
 *                      n <= 2 Mi the mid-size sort ("sort.mid"), above it the large sort ("sort.msd2"); for what
 *                      those do not take (sort_bits < 16, a work buffer below level 1, sizes beyond their limits): below
 *                      24 MiB of data the three-kernel pass, from there on the one-sweep path
 *                      0 = onesweep (one sweep per digit, 16 decoupled look-back chains)
 *                      1 = three kernels per pass: count -> table scan -> sort+scatter (the
 *                          reference's pass structure, Pprims.cpp:357-398)
 *   "sort.digit_bits"  8 [default] or 4 (the reference's R32SORT_BITS_PER_PASS, Pprims.h:31)
 *   "sort.tile"        tile geometry variant (threads x elements per thread): -1 [default] = best known
 *                      per element size (512x32 for 4-byte, 1024x16 for 8-byte elements); 0 = 256x16,
 *                      1 = 512x16, 2 = 1024x16, 3 = 512x32
 *   "sort.rank"        1 [default when the device self-test passes] = in-tile ranking by lane-ordered
 *                      returning LDS atomics; 0 = ranking by 64-lane ballot match.  Mode 1 depends on a
 *                      hardware behaviour no ISA document promises (lanes of ONE returning DS atomic
 *                      instruction that hit the same address are served in ascending lane order); it is
 *                      checked at device creation and can be re-checked at any time
 *                      (adlhip_selftest_lds_order).  Mode 0 is the safe fallback: documented wave
 *                      intrinsics only.  Pairs (AoS and SoA) keep the stable large sort in mode 0 -- its passes, its
 *                      wave-per-segment finish and its safety net have ballot-ranked variants (up to 96 Mi pairs) --; keys
 *                      take the per-digit passes (~1.4 x the time).  Every LSD pass must be stable, so key-only
 *                      sorts depend on the ranking as much as key-value sorts do.
 *   "sort.lds_ordered" (read-only) result of that self-test
 *   "sort.mid"         1 [default] / 0: between 8 Ki and 2 Mi u32 keys (16 Ki and 1 Mi pairs), full 32-bit sorts take two
 *                      launches (u32 keys: MSD pass with bucket cursors, buckets finished in LDS) or three
 *                      (pairs; keys with a constant top byte: byte histograms, stable MSD pass, LDS finish)
 *                      instead of the per-digit passes.  Keys that do not fit the buckets are detected on the
 *                      device and sorted by a cooperative LSD sort inside the same launches (correct, slower);
 *                      the handle then steers later sorts of this size class by asynchronous hints (speed only;
 *                      results never depend on them).  2 / 3 force the two- / three-launch form (tests)
 *   "sort.msd2"        1 [default] / 0: sorts of 2 Mi .. 1088 Mi u32 keys, 100 K .. 260 Mi u64 keys and 1 Mi .. 260 Mi pairs on 16 or
 *                      more bits take two MSD passes into slabs of the work buffer plus one finish in LDS (six moves of
 *                      every element instead of nine); where the two digits sit is chosen on the device from a sample of
 *                      the keys (inside the low sort_bits bits).  Whole keys: runs are placed with atomic cursors (equal keys
 *                      are indistinguishable), from 192 Mi u32 / 48 Mi u64 keys the first (or both) passes by look-back;
 *                      pairs and sorts on part of the key: by look-back, stably.  The slabs give every bucket the same room:
 *                      keys whose density varies by more than ~45 % over their range, or that repeat a few values, do not fit.
 *                      That is detected on the device -- by the sort's first kernel when its 2048 sampled keys repeat
 *                      themselves (the passes then leave at once), else by the passes, which stop at their next tile -- and
 *                      the sort's own offsets kernel then sorts the untouched input: keys that take at most 256 values by
 *                      counting, pairs with such keys by one stable pass on the key's rank among them ("sort.dict"), anything
 *                      else by four (eight) LSD passes with grid-wide barriers between them (64 Mi u32 keys: 0.30-0.44 ms
 *                      and 1.0-1.1 ms instead of 0.32; 64 Mi pairs: 0.6-0.75 and 1.4-1.5 instead of 0.75;
 *                      profiles/r4_safety_net.txt).  Nothing is reported to the host and
 *                      nothing is remembered between sorts: a sort entry point never waits, and the first sort of an input
 *                      takes the time its hundredth does.  (Rounds 2-3 kept such keys off this path by a probe launch,
 *                      pinned-memory reports and a back-off counter in the handle; all of that is gone.)
 *                      2 forces the path from 1 Mi elements (tests), 3 / 4 / 5 force its stable / cursor / hybrid form
 *   "sort.binfinish"   1 [default]: whole u64 keys finish their segments by one counting pass on the top bits below the
 *                      digits + whole-key compares inside the bins (where a segment holds ~384 keys and more); 0: the
 *                      wave-per-segment LSD finish; 2: always, u32 keys too (tests, measurements)
 *   "sort.dict"        1 [default] / 0: the large sort's safety net first samples 16 Ki keys (if the sort's first kernel saw its
 *                      samples repeat often enough for that to be possible); if they take at most 256 distinct values
 *                      (whole-key sorts only) it sorts u32 / u64 keys by counting -- dictionary, one read, one write: equal
 *                      keys are interchangeable -- and {key, value} pairs by ONE stable pass on the key's rank in the
 *                      dictionary; u32 keys of up to 4096 values are counted with a larger dictionary (64 Ki samples); it
 *                      falls through to its LSD passes when a key misses the dictionary
 *   "topk.algo"        -1 [default] / 0 / 1: adlhip_topk_typed selects (radix select + a k-element finish) while k <= n / 8 and runs
 *                      the full argsort above; 0 always runs the argsort and copies its first k, 1 always selects (tests,
 *                      measurements).  The same result bit for bit either way
 *   "topk.rows_algo"   -1 [default] / 0 / 1: adlhip_topk_rows_typed runs its row kernel while k <= 2048 and cols <= 256 Ki and the
 *                      per-row loop otherwise; 0 always loops, 1 always runs the row kernel (k > 2048 is then refused).  The 256 Ki
 *                      is a PLACEHOLDER: where one workgroup per row starts to lose to the loop has not been measured
 *                      (tools/topk_rows_bench.py measures it).  The same result bit for bit either way
 *   "debug.topk_rows_grid" workgroups the row kernel is launched with at most (0 [default]: 4 per CU); tests set it to make few
 *                      workgroups take many rows in turns
 *   "sort.rows_algo"   -1 [default] / 0 / 1: adlhip_sort_rows_typed runs its row kernel while cols <= 4096 and the flat path above that;
 *                      0 always takes the flat path, 1 always the row kernel (cols > 4096 is then refused, by the scratch query
 *                      too).  Whether 4096 is where the default ought to switch is what tools/sort_rows_bench.py measures.  The
 *                      same result bit for bit either way
 *   "debug.sort_rows_grid" workgroups the row kernel of adlhip_sort_rows_typed is launched with at most (0 [default]: 4 per CU);
 *                      tests set it to make few workgroups take many tiles in turns.  The result does not depend on it
 *   "sort.segments_algo" -1 [default] / 0 / 1: adlhip_sort_segments_typed runs its segment kernel while 0 < max_segment <= 4096 and the
 *                      flat path otherwise; 0 always takes the flat path, 1 always the segment kernel (max_segment == 0 or > 4096 is
 *                      then refused, by the scratch query too).  tools/sort_segments_bench.py measures both per shape.  The same
 *                      result bit for bit either way
 *   "debug.sort_segments_grid" workgroups the segment kernel is launched with at most (0 [default]: 3 per CU for 4-byte keys, 2 for
 *                      8-byte keys, what its LDS admits); tests set it to make few workgroups walk tiles across class boundaries.
 *                      The result does not depend on it
 *   "unique.algo"      -1 [default] / 1: adlhip_unique_typed takes its keys path (copy, typed keys sort, run stage) unless first_index or
 *                      inverse is asked, which need the index path (argsort, run stage with the permutation); 1 always takes the index
 *                      path (tests, measurements; the work buffer must then have the want_index size).  The same unique, counts and
 *                      offsets bit for bit either way
 *   "debug.unique_grid" workgroups the run stage of adlhip_run_length_encode / adlhip_unique_typed is launched with at most (0 [default]:
 *                      4 per CU; larger values change nothing); tests set it to make few workgroups take many tiles
 *   "debug.reduce_grid" workgroups the reduce stage of adlhip_reduce_runs / adlhip_reduce_by_key_typed is launched with at most (0
 *                      [default]: 4 per CU; larger values change nothing); tests set it to make few workgroups take many tiles.  Float
 *                      sums may differ in the last bits between two values of it (another association), never between two calls
 *   "debug.scan_grid"  workgroups the scan stage of adlhip_scan_typed / adlhip_scan_by_key is launched with at most (0 [default]: 4 per
 *                      CU; larger values change nothing); tests set it to make few workgroups take many tiles.  Float sums may differ
 *                      in the last bits between two values of it (another association), never between two calls
 *   "debug.compact_grid" workgroups adlhip_compact_flagged / adlhip_compact_if_typed are launched with at most (0 [default]: 4 per
 *                      CU; larger values change nothing); tests set it to make few workgroups take many tiles
 *   "debug.histogram_grid" workgroups the count kernel of adlhip_histogram_range_typed / adlhip_bincount_typed is launched with at
 *                      most (0 [default]: the G of the histogram block; larger values change nothing); tests set it to make few
 *                      workgroups take many tiles
 *   "debug.merge_grid" workgroups the tile kernel of adlhip_merge_typed is launched with at most (0 [default]: 8 per CU; larger values
 *                      change nothing); tests set it to make few workgroups take many tiles in turns.  The result does not depend on it
 *   "debug.setop_grid" workgroups the count and emit kernels of adlhip_set_op_typed are launched with at most (0 [default]: 8 per CU;
 *                      larger values change nothing); tests set it to make few workgroups take many tiles.  The result does not depend on it
 *   "debug.search_grid" workgroups the kernel of adlhip_search_sorted_typed is launched with at most (0 [default]: 8 per CU, and never
 *                      more than tiles of needles; larger values change nothing); tests set it to make few workgroups take many
 *                      tiles.  The result does not depend on it
 *   "debug.join_grid"  workgroups the bounds, sum, starts and row kernels of adlhip_join_sorted_typed and adlhip_expand_runs are launched
 *                      with at most (0 [default]: 8 per CU; larger values change nothing); tests set it to make few workgroups take
 *                      many tiles.  The result does not depend on it
 *   "debug.search_lds_keys" the capacity C of the table adlhip_search_sorted_typed keeps in LDS, in codes (2 .. 4096, default 4096; 0
 *                      sets the default); tests lower it to reach the two-level path and long searches in global memory with a
 *                      short sequence.  adlhip_get_param reports the capacity in force.  The result does not depend on it
 *   "debug.histogram_lds_bins" the largest num_bins for which adlhip_bincount_typed takes the LDS path (1 .. 8192, default 8192; 0
 *                      sets the default); tests lower it to reach the sorted path with few keys.  adlhip_get_param reports the limit
 *   "debug.persist_grid" workgroups both persistent passes of the large keys-only sort (cursor form) are launched with, rounded up to
 *                      a multiple of 8 (0 [default]: two per CU; at most 4096); tests set it to give every workgroup many rounds of
 *                      tile tickets with small inputs: while it is set the passes draw their tickets at every size (at 0 only
 *                      sorts of six rounds of tiles and more do).  The result does not depend on it
 *   "sort.net_lookback" 1 [default] / 0: the LSD passes of the large sort's safety net on whole keys are look-back passes -- the
 *                      one-sweep path's histogram, tables and tile body, taken in turns by the net's resident workgroups, four
 *                      passes at a time (u64 keys: two rounds) -- instead of count -> scan -> scatter passes with per-workgroup
 *                      carries (which sorts on part of the key and SoA arrays always get); same result, ~25 % less time
 *   "partition.lookback" 1 [default] / 0: adlhip_partition_* on 24 MiB of data and more, with a work buffer of the sort's
 *                      full-speed size, is one look-back pass (histogram + chain kernel of the one-sweep path) instead of
 *                      count -> scan -> scatter; the same output bit for bit
 *   "stat.net_runs", "stat.net_counting" (read-only; reading waits for the stream) how often the large sort's safety net has run
 *                      on this handle, and how often it sorted by counting
 *   "debug.net_stamp0" .. "debug.net_stamp9" (read-only, diagnostic) when workgroup 0 of the handle's last safety net reached its
 *                      phase boundaries, 10-ns ticks (tools/net_phases.py)
 *   "debug.idle_dirty" (read-only, diagnostic; reading waits for the stream) how many of the handle-owned device words that have an
 *                      idle value -- cursors, flags, counters and sample words of the large sort, histograms and cursors of the
 *                      mid-size sort, the padding of the dictionary block, the fault words (adlhip.hip kIdleTable, DESIGN.md
 *                      "Idle state of a handle") -- do not hold it.  0 whenever the stream is drained, whatever ran before.  Copies
 *                      the areas to the host; launches nothing and changes nothing on the device
 *   "debug.idle_first" (read-only) the first such word as region << 24 | word (regions: 1 the large sort's words, 2 the mid-size
 *                      sort's, 3 the dictionary block, 4 the fault words); 0 when clean
 *   "debug.idle_poke"  (set-only; tests) region << 24 | word: flips bit 0 of that word in stream order -- the positive control of
 *                      "debug.idle_dirty"; a second poke undoes the first
 *   "debug.resident_wgs" workgroups the device certainly keeps resident at once (asked of the runtime at creation); the
 *                      paths whose safety nets hold a grid-wide barrier over 256 workgroups are taken only when it is
 *                      >= 256.  Setting it stands in for a small partition (tests); 0 = ask the device again
 *   "profile"          0/1: bracket every kernel launch with hipEvents (Device::toggleProfiling,
 *                          Adl/Adl.h:142, AdlKernelUtilsCL.inl:654-677) */
int adlhip_set_param(adlhip_device* dev, const char* name, int value);
int adlhip_get_param(adlhip_device* dev, const char* name, int* value);

/* ---- timing / profiling ----------------------------------------------------------------------- */

/* adl::Stopwatch (Adl/AdlStopwatch.h:60-83) on the handle's stream: start/split/stop map onto
 * hipEvent records; elapsed is device time between two recorded events. */
typedef struct adlhip_event adlhip_event;
int adlhip_event_create(adlhip_device* dev, adlhip_event** out);
int adlhip_event_record(adlhip_device* dev, adlhip_event* ev);
int adlhip_event_elapsed_ms(adlhip_device* dev, adlhip_event* start, adlhip_event* stop, float* ms);
int adlhip_event_destroy(adlhip_device* dev, adlhip_event* ev);
/* DeviceCL::waitForCompletion(const SyncObject*) / isComplete(const SyncObject*) -- Adl/CL/AdlCL.inl:572-612 (clWaitForEvents /
 * clGetEventInfo on the event a copy or launch was given): wait for / poll the point of the stream at which `ev` was last
 * recorded.  An event that was never recorded counts as complete. */
int adlhip_event_synchronize(adlhip_device* dev, adlhip_event* ev);
int adlhip_event_query(adlhip_device* dev, adlhip_event* ev, int* done_out);

/* Per-kernel launch timing collected while "profile" = 1 (replaces the per-launch CSV rows of
 * Adl/CL/AdlKernelUtilsCL.inl:664-677).  adlhip_profile_count synchronises the stream and folds the
 * pending event pairs; entry i is then readable with adlhip_profile_get. */
int adlhip_profile_reset(adlhip_device* dev);
int adlhip_profile_count(adlhip_device* dev);
int adlhip_profile_get(adlhip_device* dev, int i, char name_out[64], uint64_t* launches, double* total_ms);
/* Append the table as CSV rows "kernel",launches,total_ms,avg_ms to `path` (header written when the file is
 * new) -- the reference appends a row per launch to ProfileCL.<device>.<driver>.csv
 * (Adl/CL/AdlKernelUtilsCL.inl:664-677); here the rows are per kernel, folded since the last reset. */
int adlhip_profile_write_csv(adlhip_device* dev, const char* path);

/* ---- bandwidth probes (diagnostics for bench.py: empirical HBM ceilings) ---------------------- */
int adlhip_probe_copy(adlhip_device* dev, void* d_dst, const void* d_src, size_t bytes);
int adlhip_probe_read(adlhip_device* dev, const void* d_src, size_t bytes, void* d_sink8);
/* The same with cache-policy hints (hints bit 0 = non-temporal loads, bit 1 = non-temporal stores) and a choice of grid
 * (grid_per_cu workgroups of 256 threads per CU, 0 = 8): bench.py measures every variant on buffers that are cold in every
 * cache and reports the best one as the copy / read ceiling of the box. */
int adlhip_probe_copy_ex(adlhip_device* dev, void* d_dst, const void* d_src, size_t bytes, int hints, int grid_per_cu);
int adlhip_probe_read_ex(adlhip_device* dev, const void* d_src, size_t bytes, void* d_sink8, int hints, int grid_per_cu);

/* Re-runs the device self-test that "sort.rank" = 1 rests on (returning DS atomics of one wave instruction
 * resolve colliding lanes in ascending lane order; ranks are compared with ballot/mbcnt ranks) with `workgroups`
 * workgroups of 256 and of 1024 threads, and BLOCKS until the number of disagreements is in *mismatches
 * (0 = the property holds).  Device creation runs it once on an idle chip; stress tests call it on a second
 * handle while sorts run on the first.  No reference counterpart. */
int adlhip_selftest_lds_order(adlhip_device* dev, int workgroups, uint32_t* mismatches);

/* Self-test of the key probe's sampling (hybrid_kernels.hpp probe_sample_index): computes, on the device, the 16384 positions
 * the probe would read in an array of n elements (16384 <= n) and BLOCKS until *max_index holds the largest of them (must be
 * < n) and *out_of_cell the number of positions outside their 16384th of the array (must be 0).  A regression hook: a
 * compiler expansion of an integer remainder once sent 13 of the samples 64 MiB past a 7.7 Mi-key array.  No reference
 * counterpart. */
int adlhip_selftest_probe_positions(adlhip_device* dev, size_t n, uint32_t* max_index, uint32_t* out_of_cell);

const char* adlhip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ADLHIP_H */
