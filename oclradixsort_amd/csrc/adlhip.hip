// adlhip.hip -- the sorts of include/adlhip.h: the layouts, the path choice and the drivers of the per-digit, mid-size and large sorts,
// the scan, the partitions, and what a handle owns for them (sort_state_create, the idle table).  Replaces the GPU branches of
// Tahoe/ParallelPrimitives/Pprims.cpp (pass drivers).  The runtime under it -- handle, buffers, profiling, knobs -- is handle.hip.
// gfx950 only; kernels are compiled ahead of time into this shared object.
#include "adlhip_internal.hpp"
#include "large_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>

#include "radix_kernels.hpp"
#include "onesweep_kernels.hpp"
#include "hybrid_kernels.hpp"
#include "persist_kernels.hpp"
#include "finish16_kernels.hpp"
#include "soa_wide_kernels.hpp"

// The large sort's kernels and the per-digit passes' are instantiated in kernels_finish.hip / kernels_passes.hip / kernels_perdigit.hip (translation units of
// their own, compiled beside this one); here they are only declared.  The primitives on top of the sorts are a unit of their own too (primitives.hip).
// -DADLHIP_SINGLE_TU builds everything in this file, handle.hip and primitives.hip included at its end (what tools/gen_large_kernels.py reads the list from).
#ifndef ADLHIP_SINGLE_TU
#define X(...) extern template __global__ __VA_ARGS__;
#include "finish_kernels.inc"
#include "wavefinish_kernels.inc"
#include "passes_kernels.inc"
#include "perdigit_kernels.inc"
#undef X
#endif

using namespace adlhip_internal;

namespace {

// ---- sort configuration -------------------------------------------------------------------

// Tile geometry variants (threads per workgroup NT x elements per thread K), selectable at run time
// through "sort.tile".  The small digit table of the three-kernel pass is sized for the smallest tile (kMinTile);
// the status rows of the one-sweep pass are sized for the CURRENT knobs (a sort call re-checks the size, so changing the
// variant never invalidates a caller's work buffer.
struct TileVariant {
    int nt, k;
};
constexpr TileVariant kVariants[] = {{256, 16}, {512, 16}, {1024, 16}, {512, 32}};
constexpr int kNumVariants = (int)(sizeof(kVariants) / sizeof(kVariants[0]));
}  // namespace
int adlhip_internal::num_tile_variants() { return kNumVariants; }
namespace {
constexpr uint32_t kMinTile = 4096;
constexpr int kWgsPerCu = 8;   // three-kernel pass: workgroups per CU that each own a run of tiles

struct PassPlan {
    int start_bit;
    int nbits;
};

std::vector<PassPlan> plan_passes(int sort_bits, int digit_bits)
{
    std::vector<PassPlan> p;
    int sb = 0;
    while (sb < sort_bits) {
        const int nb = (digit_bits == 8 && sort_bits - sb >= 8) ? 8 : 4;
        p.push_back({sb, nb});
        sb += nb;
    }
    return p;
}

struct Geometry {
    uint32_t tile, num_tiles, tiles_per_wg, n_wgs;
};

Geometry geometry(const adlhip_device* d, size_t n, uint32_t tile)
{
    Geometry g;
    g.tile = tile;
    g.num_tiles = (uint32_t)((n + tile - 1) / tile);
    const uint32_t max_wgs = (uint32_t)d->prop.multiProcessorCount * kWgsPerCu;
    g.tiles_per_wg = (g.num_tiles + max_wgs - 1) / max_wgs;
    if (g.tiles_per_wg == 0) g.tiles_per_wg = 1;
    g.n_wgs = (g.num_tiles + g.tiles_per_wg - 1) / g.tiles_per_wg;
    return g;
}

// "sort.tile" = -1 (default): the measured best per element size on MI355X
//   4-byte elements: 512 x 32 (16 Ki keys, 73 KiB of LDS, two workgroups per CU)
//   8-byte elements: 1024 x 16 (16 Ki elements, 145 KiB of LDS, one workgroup per CU)
//   up to 8 MiB of data: 256 x 16 (4 Ki elements) so that there are enough tiles to occupy 256 CUs;
//   4-byte elements up to 24 MiB: 512 x 16
int effective_variant(const adlhip_device* d, size_t elem_bytes, size_t n)
{
    if (d->tile_variant >= 0) return d->tile_variant;
    if (n * elem_bytes <= (size_t(8) << 20)) return 0;
    // 4-byte keys between 8 and 24 MiB (three-kernel passes): 512 x 16 (8 Ki keys) -- 4Mi keys 75 vs 79 us with 512 x 32
    if (elem_bytes == 4 && n * elem_bytes < (size_t(24) << 20)) return 1;
    return elem_bytes == 4 ? 3 : 2;
}
uint32_t current_tile(const adlhip_device* d, size_t elem_bytes, size_t n)
{
    const TileVariant v = kVariants[effective_variant(d, elem_bytes, n)];
    return (uint32_t)(v.nt * v.k);
}

// work buffer layout (three-kernel pass): [table 256 x n_wgs u32][totals 256 u32]
size_t table_bytes(const adlhip_device* d, size_t n, uint32_t tile)
{
    return align_up((size_t)256 * geometry(d, n, tile).n_wgs * 4, 256);
}
size_t work_bytes_three_kernel(const adlhip_device* d, size_t n) { return table_bytes(d, n, kMinTile) + 256 * 4; }

// Kernels with more than 64 KiB of dynamic LDS need the limit raised once per function.
// Kernels that need more than 64 KiB of dynamic LDS must be told so once (per device).  Distinct handles may be driven
// from distinct host threads, so the bookkeeping is locked.
template <typename KernelT>
int ensure_lds(KernelT kernel, size_t bytes)
{
    if (bytes <= 64 * 1024) return ADLHIP_SUCCESS;
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, size_t> raised;   // (kernel, device) -> bytes
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    size_t& have = raised[std::make_pair((const void*)kernel, dev)];
    if (have >= bytes) return ADLHIP_SUCCESS;
    HIPCHK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    have = bytes;
    return ADLHIP_SUCCESS;
}

// ---- what a sort ping-pongs between ------------------------------------------------------------------
// AosBuf<E>: one array of E.  SoaBuf: u32 keys + u32 values in separate arrays (pairs travel through the
// kernels as u64 {key low, value high}; histogram / count kernels read the key array only).
template <typename E>
struct AosBuf {
    typedef adlhip::AosIO<E> IO;
    typedef E key_t;
    static constexpr size_t kElemBytes = sizeof(E);
    static constexpr bool kSoa = false;
    E* p;
    const key_t* keys() const { return p; }
    bool same(const AosBuf& o) const { return p == o.p; }
    static IO io(const AosBuf& src, const AosBuf& dst) { return IO{src.p, dst.p}; }
    int copy_from(const AosBuf& src, size_t n, hipStream_t st) const
    {
        HIPCHK(hipMemcpyAsync(p, src.p, n * sizeof(E), hipMemcpyDeviceToDevice, st));
        return ADLHIP_SUCCESS;
    }
    static const char* tag() { return sizeof(E) == 4 ? "_u32" : "_e64"; }
};
struct SoaBuf {
    typedef adlhip::SoaIO IO;
    typedef uint32_t key_t;
    static constexpr size_t kElemBytes = 8;
    static constexpr bool kSoa = true;
    uint32_t* k;
    uint32_t* v;
    const key_t* keys() const { return k; }
    bool same(const SoaBuf& o) const { return k == o.k; }
    static IO io(const SoaBuf& src, const SoaBuf& dst) { return IO{src.k, src.v, dst.k, dst.v}; }
    int copy_from(const SoaBuf& src, size_t n, hipStream_t st) const
    {
        HIPCHK(hipMemcpyAsync(k, src.k, n * 4, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(v, src.v, n * 4, hipMemcpyDeviceToDevice, st));
        return ADLHIP_SUCCESS;
    }
    static const char* tag() { return "_soa"; }
};

template <typename Buf, int NBITS>
const char* kernel_name(const char* stem)
{
    return intern(std::string(stem) + Buf::tag() + (NBITS == 8 ? "_8b" : "_4b"));
}

// tile variant: SoA pairs are instantiated for two geometries only (256x16 for small inputs, 1024x16 otherwise)
template <typename Buf>
int buf_variant(const adlhip_device* d, size_t n)
{
    const int v = effective_variant(d, Buf::kElemBytes, n);
    if (Buf::kSoa) return v == 0 ? 0 : 2;
    return v;
}
template <typename Buf>
uint32_t buf_tile(const adlhip_device* d, size_t n)
{
    const TileVariant v = kVariants[buf_variant<Buf>(d, n)];
    return (uint32_t)(v.nt * v.k);
}

#define ADLHIP_DISPATCH_TILE(FN, Buf, NBITS, ...)                                                     \
    if (Buf::kSoa) {                                                                                  \
        switch (buf_variant<Buf>(d, n) * 2 + (d->rank_mode ? 1 : 0)) {                                \
        case 0: return FN<Buf, NBITS, 256, 16, 0>(__VA_ARGS__);                                       \
        case 1: return FN<Buf, NBITS, 256, 16, 1>(__VA_ARGS__);                                       \
        case 4: return FN<Buf, NBITS, 1024, 16, 0>(__VA_ARGS__);                                      \
        default: return FN<Buf, NBITS, 1024, 16, 1>(__VA_ARGS__);                                     \
        }                                                                                             \
    }                                                                                                 \
    switch (buf_variant<Buf>(d, n) * 2 + (d->rank_mode ? 1 : 0)) {                                    \
    case 0: return FN<Buf, NBITS, 256, 16, 0>(__VA_ARGS__);                                           \
    case 1: return FN<Buf, NBITS, 256, 16, 1>(__VA_ARGS__);                                           \
    case 2: return FN<Buf, NBITS, 512, 16, 0>(__VA_ARGS__);                                           \
    case 3: return FN<Buf, NBITS, 512, 16, 1>(__VA_ARGS__);                                           \
    case 4: return FN<Buf, NBITS, 1024, 16, 0>(__VA_ARGS__);                                          \
    case 5: return FN<Buf, NBITS, 1024, 16, 1>(__VA_ARGS__);                                          \
    case 6: return FN<Buf, NBITS, 512, 32, 0>(__VA_ARGS__);                                           \
    case 7: return FN<Buf, NBITS, 512, 32, 1>(__VA_ARGS__);                                           \
    default: return fail("bad tile variant %d", d->tile_variant);                                     \
    }

// ---- three-kernel pass: count -> table scan -> sort+scatter --------------------------------------

template <typename Buf, int NBITS, int NT, int K, int RANK>
int launch_scatter(adlhip_device* d, const Buf& src, const Buf& dst, const uint32_t* table, const uint32_t* totals,
                   size_t n, const Geometry& g, int start_bit)
{
    if (Buf::kSoa && !((NT == 256 && K == 16) || (NT == 1024 && K == 16))) return fail("internal: SoA tile");
    typedef typename Buf::IO IO;
    using C = adlhip::TileCfg<typename IO::elem_t, NBITS, NT, K>;
    auto kern = adlhip::radix_scatter_kernel<IO, NBITS, NT, K, RANK>;
    if (ensure_lds(kern, C::LDS_BYTES)) return ADLHIP_FAILURE;
    const IO io = Buf::io(src, dst);
    return launch(d, kernel_name<Buf, NBITS>("scatter"), [&] {
        hipLaunchKernelGGL(kern, dim3(g.n_wgs), dim3(NT), C::LDS_BYTES, d->stream, io, table, totals, (uint32_t)n,
                           (int)g.n_wgs, start_bit, g.tiles_per_wg, g.num_tiles);
    });
}

template <typename Buf, int NBITS>
int dispatch_scatter(adlhip_device* d, const Buf& src, const Buf& dst, const uint32_t* table, const uint32_t* totals,
                     size_t n, const Geometry& g, int start_bit)
{
    ADLHIP_DISPATCH_TILE(launch_scatter, Buf, NBITS, d, src, dst, table, totals, n, g, start_bit)
}

// three-kernel pass with at most this many workgroups: the count kernel leaves its raw counts workgroup-major and the
// scatter kernel sums its column itself (16 or 64 independent coalesced loads per thread), so the table-scan launch is
// dropped -- 12 -> 8 dependent launches per 32-bit sort.  Same-session A/B (a limit of 0 / 16 / 64 workgroups):
// 32 Ki keys 35.8 -> 26.5 us; 64 Ki + 1 .. 128 Ki keys 38.3 -> 36.0 / 37.2 -> 34.5 us; 200000 .. 256 Ki keys level.
constexpr uint32_t kScanInScatterMaxWgs = 64;

template <typename Buf, int NBITS>
int three_kernel_pass(adlhip_device* d, const Buf& src, const Buf& dst, void* work, size_t n, int start_bit,
                      bool need_totals = false)
{
    typedef typename Buf::key_t key_t;
    constexpr int kCountNT = 256;
    const Geometry g = geometry(d, n, buf_tile<Buf>(d, n));
    uint32_t* table = reinterpret_cast<uint32_t*>(work);
    uint32_t* totals = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(work) + table_bytes(d, n, kMinTile));
    const uint32_t elems_per_wg = g.tiles_per_wg * g.tile;
    const bool fused = !need_totals && g.n_wgs <= kScanInScatterMaxWgs;
    int rc = launch(d, kernel_name<Buf, NBITS>("count"), [&] {
        hipLaunchKernelGGL((adlhip::radix_count_kernel<key_t, NBITS, kCountNT>), dim3(g.n_wgs), dim3(kCountNT), 0, d->stream,
                           src.keys(), table, (uint32_t)n, (int)g.n_wgs, start_bit, elems_per_wg, fused ? 1 : 0);
    });
    if (rc) return rc;
    if (fused) return dispatch_scatter<Buf, NBITS>(d, src, dst, table, nullptr, n, g, start_bit);
    rc = launch(d, "scan_table", [&] {
        hipLaunchKernelGGL((adlhip::radix_scan_table_kernel<256>), dim3(1 << NBITS), dim3(256), 0, d->stream, table,
                           totals, (int)g.n_wgs);
    });
    if (rc) return rc;
    return dispatch_scatter<Buf, NBITS>(d, src, dst, table, totals, n, g, start_bit);
}

// ---- onesweep --------------------------------------------------------------------------------

// work buffer layout (onesweep):
//   [ctrl   : per pass 16 chain tickets, one 128-byte line each (2 KiB); 16 passes = 32 KiB]
//   [tables : 16 x PassTable]
//   [joint  : joint histograms of all passes (<= 16 passes x 16 chains x 256 bins)]
//   [partial: hist_wgs x total_bins u32]
//   [status : passes x status_rows x 256 u32]
struct OnesweepLayout {
    size_t off_ctrl, off_tables, off_joint, off_part, off_status, total;
    uint32_t hist_wgs;
};

constexpr uint32_t kMaxJointBins = 8u * 16u * 256u;   // 64-bit keys, eight 8-bit passes (16 x 4-bit passes need less)

uint32_t hist_wgs_for(const adlhip_device* d, size_t n)
{
    const uint32_t cap = (uint32_t)d->prop.multiProcessorCount;   // one 1024-thread workgroup per CU (2 or 4 measured slower)
    uint32_t w = (uint32_t)((n + adlhip::kHistChunk - 1) / adlhip::kHistChunk);
    if (w > cap) w = cap;
    return w ? w : 1;
}

// status rows of one pass: one per tile; every chain may add one partial tile
size_t status_rows(size_t n, uint32_t tile) { return (n + tile - 1) / tile + adlhip::kChains + 1; }

// most passes a sort of `key_bits`-bit keys can need with the current digit width (8,8,8,4 style plans included)
int max_passes_for(const adlhip_device* d, int key_bits)
{
    return d->digit_bits == 8 ? (key_bits + 7) / 8 : key_bits / 4;
}

OnesweepLayout onesweep_layout(const adlhip_device* d, size_t n, int max_passes, uint32_t tile)
{
    OnesweepLayout L;
    L.hist_wgs = hist_wgs_for(d, n);
    L.off_ctrl = 0;
    L.off_tables = (size_t)adlhip::kTicketVecs * 16;
    L.off_joint = L.off_tables + sizeof(adlhip::PassTable) * adlhip::kMaxPasses;
    L.off_part = align_up(L.off_joint + (size_t)kMaxJointBins * 4, 256);
    L.off_status = align_up(L.off_part + (size_t)L.hist_wgs * kMaxJointBins * 4, 256);
    L.total = L.off_status + (size_t)max_passes * status_rows(n, tile) * 256 * 4;
    return L;
}

template <typename Buf, int NBITS, int NT, int K, int RANK>
int launch_onesweep(adlhip_device* d, const Buf& src, const Buf& dst, const adlhip::PassTable* table, uint32_t* status,
                    uint32_t* tickets, size_t n, int start_bit, const uint32_t* dyn_start_bit = nullptr)
{
    if (Buf::kSoa && !((NT == 256 && K == 16) || (NT == 1024 && K == 16))) return fail("internal: SoA tile");
    typedef typename Buf::IO IO;
    using C = adlhip::TileCfg<typename IO::elem_t, NBITS, NT, K>;
    auto kern = adlhip::onesweep_chain_kernel<IO, NBITS, NT, K, RANK>;
    if (ensure_lds(kern, C::LDS_BYTES)) return ADLHIP_FAILURE;
    const size_t rows = status_rows(n, (uint32_t)C::TILE);
    const uint32_t grid = (uint32_t)((n + C::TILE - 1) / C::TILE) + adlhip::kChains;   // upper bound on the tile count
    const uint32_t status_bytes = (uint32_t)(rows * C::BINS * 4u);
    const IO io = Buf::io(src, dst);
    return launch(d, kernel_name<Buf, NBITS>("onesweep"), [&] {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), C::LDS_BYTES, d->stream, io, table, status, status_bytes, tickets,
                           d->d_fault, (uint32_t)n, start_bit, dyn_start_bit);
    });
}

template <typename Buf, int NBITS>
int dispatch_onesweep(adlhip_device* d, const Buf& src, const Buf& dst, const adlhip::PassTable* table, uint32_t* status,
                      uint32_t* tickets, size_t n, int start_bit)
{
    ADLHIP_DISPATCH_TILE(launch_onesweep, Buf, NBITS, d, src, dst, table, status, tickets, n, start_bit)
}

// copy_back = false / totals_at != nullptr: the one-pass partition (partition_top_byte): the result stays in `tmp`, and the digit
// totals of pass 0 (its joint histogram folded over the 16 chains) are left in the work buffer at *totals_at
template <typename Buf>
int onesweep_sort(adlhip_device* d, Buf data, Buf tmp, void* work, size_t n, const std::vector<PassPlan>& plan, bool copy_back = true,
                  uint32_t** totals_at = nullptr)
{
    typedef typename Buf::key_t key_t;
    const int P = (int)plan.size();
    const uint32_t tile = buf_tile<Buf>(d, n);
    const OnesweepLayout L = onesweep_layout(d, n, max_passes_for(d, Buf::kElemBytes == 4 ? 32 : 64), tile);
    char* wb = reinterpret_cast<char*>(work);
    uint32_t* ctrl = reinterpret_cast<uint32_t*>(wb + L.off_ctrl);
    adlhip::PassTable* tables = reinterpret_cast<adlhip::PassTable*>(wb + L.off_tables);
    uint32_t* joint = reinterpret_cast<uint32_t*>(wb + L.off_joint);
    uint32_t* part = reinterpret_cast<uint32_t*>(wb + L.off_part);
    uint32_t* status = reinterpret_cast<uint32_t*>(wb + L.off_status);
    const size_t rows = status_rows(n, tile);

    // the tickets and every status word of the passes we run (status is contiguous) are zeroed by the histogram kernel
    const size_t status_vecs = (size_t)P * rows * 256 * 4 / 16;

    adlhip::PassDesc desc;
    desc.num_passes = P;
    uint32_t total_bins = 0;
    for (int i = 0; i < P; ++i) {
        desc.start_bit[i] = (uint8_t)plan[i].start_bit;
        desc.nbits[i] = (uint8_t)plan[i].nbits;
        total_bins += adlhip::joint_bins(plan[i].nbits);
    }
    if (total_bins > kMaxJointBins) return fail("internal: joint histogram of %u bins exceeds %u", total_bins, kMaxJointBins);
    // histogram workgroups nest inside the 16 input slices that are pass 0's chains
    const uint32_t per_wg = (uint32_t)align_up((n + L.hist_wgs - 1) / L.hist_wgs, 1024);
    const uint32_t wgs = (uint32_t)((n + per_wg - 1) / per_wg);
    const uint32_t wgs_per_slice = (wgs + adlhip::kChains - 1) / adlhip::kChains;
    const uint32_t slice0 = per_wg * wgs_per_slice;
    const size_t hist_lds = (size_t)total_bins * 4;
    int rc = ADLHIP_FAILURE;
    const key_t* hist_src = data.keys();
    auto run_hist = [&](auto kern) -> int {
        if (ensure_lds(kern, hist_lds)) return ADLHIP_FAILURE;
        return launch(d, sizeof(key_t) == 4 ? "os_hist_u32" : "os_hist_e64", [&] {
            hipLaunchKernelGGL(kern, dim3(wgs), dim3(adlhip::kHistNT), hist_lds, d->stream, hist_src, part, (uint32_t)n, per_wg,
                               slice0, desc, total_bins, reinterpret_cast<adlhip::u32x4*>(ctrl),
                               reinterpret_cast<adlhip::u32x4*>(status), status_vecs, d->d_fault);
        });
    };
    switch (P) {   // pass count is a template parameter of the histogram kernel (descriptors stay in SGPRs)
#define ADLHIP_HIST_CASE(N) case N: rc = run_hist(adlhip::onesweep_hist_kernel<key_t, N>); break;
        ADLHIP_HIST_CASE(1) ADLHIP_HIST_CASE(2) ADLHIP_HIST_CASE(3) ADLHIP_HIST_CASE(4) ADLHIP_HIST_CASE(5)
        ADLHIP_HIST_CASE(6) ADLHIP_HIST_CASE(7) ADLHIP_HIST_CASE(8) ADLHIP_HIST_CASE(9) ADLHIP_HIST_CASE(10)
        ADLHIP_HIST_CASE(11) ADLHIP_HIST_CASE(12) ADLHIP_HIST_CASE(13) ADLHIP_HIST_CASE(14) ADLHIP_HIST_CASE(15)
        ADLHIP_HIST_CASE(16)
#undef ADLHIP_HIST_CASE
        default: return fail("internal: %d passes", P);
    }
    if (rc) return rc;
    rc = launch(d, "os_hist_reduce", [&] {
        hipLaunchKernelGGL(adlhip::onesweep_hist_reduce_kernel, dim3((total_bins + 255) / 256), dim3(1024), 0, d->stream,
                           part, joint, wgs, total_bins);
    });
    if (rc) return rc;
    rc = launch(d, "os_tables", [&] {
        hipLaunchKernelGGL(adlhip::onesweep_tables_kernel, dim3(P), dim3(256), 0, d->stream, joint, tables, desc, tile);
    });
    if (rc) return rc;

    Buf src = data;
    Buf dst = tmp;
    for (int i = 0; i < P; ++i) {
        uint32_t* st = status + (size_t)i * rows * 256;
        uint32_t* tk = ctrl + i * adlhip::kChains * adlhip::kTicketStride;
        rc = (plan[i].nbits == 8) ? dispatch_onesweep<Buf, 8>(d, src, dst, tables + i, st, tk, n, plan[i].start_bit)
                                  : dispatch_onesweep<Buf, 4>(d, src, dst, tables + i, st, tk, n, plan[i].start_bit);
        if (rc) return rc;
        std::swap(src, dst);
    }
    if (totals_at) {   // `part` is free once the reduce kernel has run
        rc = launch(d, "os_fold_totals", [&] {
            hipLaunchKernelGGL(adlhip::fold_joint_kernel, dim3(1), dim3(256), 0, d->stream, (const uint32_t*)joint, part);
        });
        if (rc) return rc;
        *totals_at = part;
    }
    if (copy_back && !src.same(data)) return data.copy_from(src, n, d->stream);
    return ADLHIP_SUCCESS;
}

template <typename Buf>
int three_kernel_sort(adlhip_device* d, Buf data, Buf tmp, void* work, size_t n, const std::vector<PassPlan>& plan)
{
    Buf src = data;
    Buf dst = tmp;
    for (const PassPlan& p : plan) {
        int rc = (p.nbits == 8) ? three_kernel_pass<Buf, 8>(d, src, dst, work, n, p.start_bit)
                                : three_kernel_pass<Buf, 4>(d, src, dst, work, n, p.start_bit);
        if (rc) return rc;
        std::swap(src, dst);   // Pprims.cpp:397
    }
    // odd number of passes: result sits in the scratch buffer -> copy back (Pprims.cpp:400-403)
    if (!src.same(data)) return data.copy_from(src, n, d->stream);
    return ADLHIP_SUCCESS;
}

// ---- small inputs: the whole sort in one workgroup ---------------------------------------------------
// (kSmallMax: large_plan.hpp, where the large sort starts from it)

template <typename E, int NT, int K, int RANK>
int launch_small(adlhip_device* d, E* data, size_t n, const adlhip::SmallPlan& sp)
{
    auto kern = adlhip::small_sort_kernel<E, NT, K, RANK>;
    const size_t lds = sizeof(E) * NT * K + (size_t)(NT / 64) * 256 * 4 + 128;
    if (ensure_lds(kern, lds)) return ADLHIP_FAILURE;
    return launch(d, sizeof(E) == 4 ? "small_sort_u32" : "small_sort_e64", [&] {
        hipLaunchKernelGGL(kern, dim3(1), dim3(NT), lds, d->stream, data, (uint32_t)n, sp);
    });
}

template <typename E>
int small_sort(adlhip_device* d, E* data, size_t n, const std::vector<PassPlan>& plan)
{
    adlhip::SmallPlan sp;
    sp.num_passes = (int)plan.size();
    for (size_t i = 0; i < plan.size(); ++i) {
        sp.start_bit[i] = (uint8_t)plan[i].start_bit;
        sp.nbits[i] = (uint8_t)plan[i].nbits;
    }
    if (n <= 4096) return d->rank_mode ? launch_small<E, 256, 16, 1>(d, data, n, sp) : launch_small<E, 256, 16, 0>(d, data, n, sp);
    return d->rank_mode ? launch_small<E, 1024, 16, 1>(d, data, n, sp) : launch_small<E, 1024, 16, 0>(d, data, n, sp);
}

// ---- segments finished in LDS (adlhip_segment_sort; pass 3 of the mid-size sort) -----------------------------------
template <typename E, int NT, int K, int LBITS>
int launch_segment_sort(adlhip_device* d, const E* in, E* out, const uint32_t* seg_start, size_t num_segments, int low_bits,
                        const uint32_t* dyn, const adlhip::MidCoop& coop = adlhip::MidCoop{nullptr, nullptr, nullptr, 0u},
                        const adlhip::SegSlab& slab = adlhip::SegSlab{nullptr, 0u, nullptr, nullptr})
{
    auto kern = adlhip::segment_sort_kernel<E, NT, K, LBITS>;
    const size_t own = sizeof(E) * NT * K + (size_t)(NT / 64) * (1u << LBITS) * 6 + 64;
    const size_t lds = std::max(own, (size_t)adlhip::TileCfg<E, 8, NT, K>::LDS_BYTES);   // the through-memory path's carve
    if (ensure_lds(kern, lds)) return ADLHIP_FAILURE;
    // as many workgroups as are resident at once (LDS- or wave-limited), each loops over segments
    const size_t per_cu = std::max<size_t>(1, std::min<size_t>((size_t)160 * 1024 / lds, (size_t)32 / (NT / 64)));
    // slab form (slab.state != nullptr): exactly one workgroup per bucket -- the kernel reads its bucket's count and offset once;
    // workgroups that are not resident yet simply follow (mid_eligible keeps the form off devices that hold fewer than 256)
    const uint32_t grid = slab.state ? (uint32_t)num_segments
                                     : (uint32_t)std::min<size_t>(num_segments, per_cu * (size_t)d->prop.multiProcessorCount);
    return launch(d, sizeof(E) == 4 ? "segment_sort_u32" : "segment_sort_e64", [&] {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds, d->stream, in, out, seg_start, (uint32_t)num_segments, (uint32_t)low_bits,
                           dyn, d->d_fault, coop, slab);
    });
}

template <typename E, int K, typename S = E, bool SOA = false, int RANK = 1>
int launch_wave_segment_sort(adlhip_device* d, const E* in, E* out, const uint32_t* seg_start, size_t num_segments, int low_bits,
                             const uint32_t* seg_cnt = nullptr, uint32_t in_stride = 0, const uint32_t* gate = nullptr,
                             const uint32_t* dyn_low_bits = nullptr, uint32_t* out_vals = nullptr, const uint32_t* list = nullptr,
                             const uint32_t* list_cnt = nullptr, uint32_t seg_shift = 8)
{
    // a wave's LDS: its tile + 256 counters; waves per workgroup so that a workgroup takes at most ~48 KiB (three per CU)
    constexpr size_t per_wave = sizeof(E) * 64 * K + 256 * 4;
    constexpr int WAVES = per_wave <= 6144 ? 8   /* eight waves with the 7 KiB of the 1536-element tile measured slower */ : per_wave <= 12288 ? 4 : per_wave <= 24576 ? 2 : 1;
    constexpr int STEP = K <= 40 ? 2 : 4;        // row-count bodies: every 2 rows, every 4 for the largest tile
    constexpr int RMIN = K <= 24 ? 2 : K / 2;    // the tiles beyond 24 rows exist for segments that need them
    const size_t lds = (size_t)WAVES * per_wave;
    if (list) {
        if constexpr (!SOA) {
            auto kern = adlhip::wave_segment_sort_kernel<E, K, WAVES, STEP, RMIN, S, SOA, true>;
            if (ensure_lds(kern, lds)) return ADLHIP_FAILURE;
            // list form (the segments the binning finish handed over -- usually none): a small grid that takes them in turns
            const size_t slots = std::min<size_t>(num_segments, (size_t)4 * d->prop.multiProcessorCount);
            const uint32_t grid = (uint32_t)((slots + WAVES - 1) / WAVES);
            return launch(d, sizeof(E) == 4 ? "segment_sort_listed_u32" : "segment_sort_listed_e64", [&] {
                hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * WAVES), lds, d->stream, in, out, seg_start, (uint32_t)num_segments,
                                   (uint32_t)low_bits, d->d_fault, seg_cnt, in_stride, gate, dyn_low_bits, out_vals, list, list_cnt, seg_shift);
            });
        } else {
            return fail("internal: no list form for SoA");
        }
    }
    auto kern = adlhip::wave_segment_sort_kernel<E, K, WAVES, STEP, RMIN, S, SOA, false, RANK>;
    if (ensure_lds(kern, lds)) return ADLHIP_FAILURE;
    const uint32_t grid = (uint32_t)((num_segments + WAVES - 1) / WAVES);
    return launch(d, sizeof(E) == 4 ? "segment_sort_wave_u32" : "segment_sort_wave_e64", [&] {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * WAVES), lds, d->stream, in, out, seg_start, (uint32_t)num_segments,
                           (uint32_t)low_bits, d->d_fault, seg_cnt, in_stride, gate, dyn_low_bits, out_vals, list, list_cnt, seg_shift);
    });
}

// the binning finish of the large keys-only sort (hybrid_kernels.hpp bin_segment_sort_kernel): one workgroup per segment slab
template <typename E, typename S, int NT, int K, int BITS>
int launch_bin_segment_sort(adlhip_device* d, const S* in, E* out, const uint32_t* seg_off, const uint32_t* seg_cnt, uint32_t in_stride,
                            uint32_t* mode, uint32_t* hard_list, uint32_t seg_shift = 8)
{
    auto kern = adlhip::bin_segment_sort_kernel<E, S, NT, K, BITS>;
    const size_t lds = align_up(sizeof(S) * NT * K, 16) + ((size_t)(1 << BITS) / 2) * 4 + (2 * NT / 64 + 4) * 4;
    if (ensure_lds(kern, lds)) return ADLHIP_FAILURE;
    // one workgroup per segment.  (The kernel can loop -- a grid of resident workgroups that take segments in turns and request the
    // next one's keys early -- but measured slower: 256 Mi u64 keys 1.02 vs 0.89 ms, 64 Mi 0.33 vs 0.26; a workgroup that leaves
    // hands its LDS to the next one while its stores drain.)
    const uint32_t grid = 256u << seg_shift;
    return launch(d, sizeof(E) == 4 ? "segment_sort_bin_u32" : "segment_sort_bin_u64", [&] {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds, d->stream, in, out, seg_off, seg_cnt, in_stride, grid, (const uint32_t*)mode,
                           mode + adlhip::kDynHardCnt, hard_list, d->d_fault, seg_shift);
    });
}

// the workgroup-per-segment finish of the large sort beyond 280 Mi u32 keys (hybrid_kernels.hpp wg_segment_sort_kernel)
template <typename E, typename S, int NT, int K>
int launch_wg_segment_sort(adlhip_device* d, const S* in, E* out, const uint32_t* seg_off, const uint32_t* seg_cnt, uint32_t in_stride,
                           const uint32_t* mode, size_t slots)
{
    auto kern = adlhip::wg_segment_sort_kernel<E, S, NT, K>;
    const size_t lds = sizeof(S) * NT * K + (size_t)(NT / 64) * 256 * 6;
    if (ensure_lds(kern, lds)) return ADLHIP_FAILURE;
    return launch(d, "segment_sort_wg_u32", [&] {
        hipLaunchKernelGGL(kern, dim3((uint32_t)slots), dim3(NT), lds, d->stream, in, out, seg_off, seg_cnt, in_stride, mode,
                           mode + adlhip::kDynLowBits, d->d_fault);
    });
}

// largest segment the finishing kernel takes for this element size and number of low bits
size_t segment_capacity(size_t elem_bytes, int low_bits)
{
    if (elem_bytes == 4) return low_bits <= 24 ? 16384 : 8192;
    return low_bits <= 24 ? 8192 : 4096;
}

template <typename E>
int segment_sort(adlhip_device* d, const E* in, E* out, const uint32_t* seg_start, size_t num_segments, size_t max_segment,
                 int low_bits, const uint32_t* dyn)
{
    // small segments, at most 16 bits: one wave per segment
    if (low_bits <= 16 && dyn == nullptr && max_segment <= 1280)
        return launch_wave_segment_sort<E, 20>(d, in, out, seg_start, num_segments, low_bits);
    // tile by the caller's bound on the segment size; the digit width of the local passes by what fits beside the tile
    if (sizeof(E) == 4) {
        if (max_segment <= 4096) return launch_segment_sort<E, 256, 16, 9>(d, in, out, seg_start, num_segments, low_bits, dyn);
        if (max_segment <= 8192) return launch_segment_sort<E, 512, 16, 9>(d, in, out, seg_start, num_segments, low_bits, dyn);
        if (max_segment <= 16384 && low_bits <= 24) return launch_segment_sort<E, 512, 32, 8>(d, in, out, seg_start, num_segments, low_bits, dyn);
    } else {
        if (max_segment <= 4096) return launch_segment_sort<E, 256, 16, 9>(d, in, out, seg_start, num_segments, low_bits, dyn);
        if (max_segment <= 8192 && low_bits <= 24) return launch_segment_sort<E, 512, 16, 8>(d, in, out, seg_start, num_segments, low_bits, dyn);
    }
    return fail("segment sort: segments of up to %zu elements with %d key bits exceed the LDS tile (%zu)", max_segment, low_bits,
                segment_capacity(sizeof(E), low_bits));
}

// ---- mid-size sort: byte histograms + tables -> one MSD pass -> buckets finished in LDS (hybrid_kernels.hpp) ----------
// u32 keys take the two-launch mid-size sort from here -- below the one-workgroup sort's limit kSmallMax: 10000 keys 16.5 -> 15.6 us,
// 12288 17.9 -> 15.5, 16384 19.3 -> 15.4; from 4096 it loses (6000 keys 13.6 -> 15.1).  profiles/r3_small_mid_ab.txt
constexpr size_t kMidMinU32 = 8192;
constexpr size_t kMidMaxU32 = size_t(2) << 20;
constexpr size_t kMidMaxE64 = size_t(1) << 20;
constexpr uint32_t kMidTile = 4096;   // pass 2 runs on 256 x 16 tiles

struct MidLayout {
    size_t off_tickets, off_table, off_seg, off_dyn, off_status, off_coop, off_slab, total;
    uint32_t wgs, rows, coop_wgs, stride;
};

MidLayout mid_layout(size_t n)
{
    MidLayout L;
    L.wgs = (uint32_t)((n + adlhip::kMidChunk - 1) / adlhip::kMidChunk);
    L.rows = (uint32_t)((n + kMidTile - 1) / kMidTile) + adlhip::kChains + 1;
    L.off_tickets = 0;
    L.off_table = (size_t)adlhip::kChains * adlhip::kTicketStride * 4;
    L.off_seg = L.off_table + sizeof(adlhip::PassTable);
    L.off_dyn = align_up(L.off_seg + 257 * 4, 16);
    L.off_status = align_up(L.off_dyn + sizeof(adlhip::MidDyn), 256);
    // cooperative LSD kernel (safety net for skewed keys): bucket-major table [256][wgs] + 256 totals
    L.coop_wgs = 256;   // = the grid of pass 3 (one workgroup per bucket)
    L.off_coop = align_up(L.off_status + (size_t)L.rows * 256 * 4, 256);
    // keys-only form: 256 bucket slabs of `stride` elements (= the LDS tile of pass 2: at least twice the mean bucket)
    L.stride = n <= (size_t(512) << 10) ? 4096u : (n <= (size_t(1) << 20) ? 8192u : 16384u);
    L.off_slab = align_up(L.off_coop + (size_t)256 * L.coop_wgs * 4 + 256 * 4, 256);
    L.total = L.off_slab + (size_t)256 * L.stride * 4;
    return L;
}

bool mid_eligible(const adlhip_device* d, size_t elem_bytes, size_t n, int sort_bits, int max_bits)
{
    if (d->resident_wgs < 256) return false;   // the finish's one workgroup per bucket doubles as a 256-workgroup cooperative sort
    return d->sort_algo < 0 && d->mid_path && max_bits == 32 && sort_bits == 32 && d->rank_mode == 1 && d->digit_bits == 8 &&
           d->tile_variant < 0 && n > (elem_bytes == 4 ? kMidMinU32 : kSmallMax) && n <= (elem_bytes == 4 ? kMidMaxU32 : kMidMaxE64);
}

// Which form an eligible sort takes: 2 = two launches (u32 keys only), 3 = three launches, 0 = the per-digit passes.
// Both mid-size forms fall back to a cooperative LSD sort when the keys do not fit their buckets -- correct, but 3-5x the cost
// of the per-digit passes (profiles/r2_mid_size_distributions_every_sort_through_mid_path.txt) -- and report what happened into
// pinned memory (hybrid_kernels.hpp: mid_prep_kernel, SegSlab::host_mode).  The host reads the latest reports WITHOUT
// synchronising (they may be a sort or two old) and steers by them:
//   two-launch form overflowed, top byte constant  -> this handle's next 64 eligible sorts take the three-launch form
//                                                     (it picks the byte that varies); 512, 4096 after repeats
//   two-launch form overflowed, several buckets    -> ... and the next 32 (256, 2048, 4096) take the per-digit passes
//   three-launch form fell back                    -> the next 32 (256, ...) take the per-digit passes
// A success resets the respective count.  Only speed depends on any of this; "sort.mid" = 2 / 3 force a form, 0 = off.
int choose_mid_form(adlhip_device* d, bool keys_only)
{
    if (d->mid_path == 2) return keys_only ? 2 : 3;
    if (d->mid_path == 3) return 3;
    if (keys_only) {
        if (d->mid2_skip > 0) {
            --d->mid2_skip;
        } else {
            const uint32_t report = d->h_fault[10];
            d->h_fault[10] = 0u;
            if (report >= 2u) {
                d->mid2_skip = d->mid2_backoff;
                d->mid2_backoff = std::min(d->mid2_backoff * 8, 4096);
                if (report == 2u) {
                    d->mid_skip = std::max(d->mid_skip, d->mid_backoff);
                    d->mid_backoff = std::min(d->mid_backoff * 8, 4096);
                }
            } else {
                if (report == 1u) d->mid2_backoff = 64;
                return 2;
            }
        }
    }
    if (d->mid_skip > 0) {
        --d->mid_skip;
        return 0;
    }
    const uint32_t report = d->h_fault[9];
    d->h_fault[9] = 0u;
    if (report == 2u) {
        d->mid_skip = d->mid_backoff;
        d->mid_backoff = std::min(d->mid_backoff * 8, 4096);
        return 0;
    }
    if (report == 1u) d->mid_backoff = 32;
    return 3;
}

template <typename E>
int mid_sort(adlhip_device* d, E* data, E* tmp, void* work, size_t n)
{
    const MidLayout L = mid_layout(n);
    char* wb = reinterpret_cast<char*>(work);
    uint32_t* tickets = reinterpret_cast<uint32_t*>(wb + L.off_tickets);
    adlhip::PassTable* table = reinterpret_cast<adlhip::PassTable*>(wb + L.off_table);
    uint32_t* seg_start = reinterpret_cast<uint32_t*>(wb + L.off_seg);
    adlhip::MidDyn* dyn = reinterpret_cast<adlhip::MidDyn*>(wb + L.off_dyn);
    uint32_t* status = reinterpret_cast<uint32_t*>(wb + L.off_status);
    const uint32_t status_vecs = (uint32_t)((size_t)L.rows * 256 * 4 / 16);
    // buckets average n / 256 elements; the LDS tile of pass 3 holds at least twice that, and an input whose largest
    // bucket still does not fit goes to the cooperative LSD kernel instead (decided on the device by mid_prep_kernel)
    const size_t cap = std::min(std::max<size_t>(4096, 2 * ((n + 255) / 256)), segment_capacity(sizeof(E), 24));
    int rc = launch(d, sizeof(E) == 4 ? "mid_prep_u32" : "mid_prep_e64", [&] {
        hipLaunchKernelGGL((adlhip::mid_prep_kernel<E>), dim3(L.wgs), dim3(adlhip::kMidPrepNT), 0, d->stream, (const E*)data, (uint32_t)n,
                           kMidTile, d->d_mid_hist, table, seg_start, dyn, reinterpret_cast<adlhip::u32x4*>(tickets),
                           reinterpret_cast<adlhip::u32x4*>(status), status_vecs, d->d_fault + 12, d->d_fault, (uint32_t)cap,
                           d->h_fault + 9);
    });
    if (rc) return rc;
    rc = launch_onesweep<AosBuf<E>, 8, 256, 16, 1>(d, AosBuf<E>{data}, AosBuf<E>{tmp}, table, status, tickets, n, 24, &dyn->start_bit);
    if (rc) return rc;
    // pass 3: 8-bit local digits (the bytes below the MSD byte); its workgroups double as the cooperative LSD sort that takes
    // over when mid_prep_kernel found a bucket beyond `cap` (the grid is 256 workgroups either way)
    uint32_t* ctable = reinterpret_cast<uint32_t*>(wb + L.off_coop);
    const adlhip::MidCoop coop{ctable, ctable + (size_t)256 * 256, d->d_fault + 13, (uint32_t)n};
    const uint32_t* dd = &dyn->start_bit;
    if (sizeof(E) == 4) {
        if (cap <= 4096) return launch_segment_sort<E, 256, 16, 8>(d, tmp, data, seg_start, 256, 24, dd, coop);
        if (cap <= 8192) return launch_segment_sort<E, 512, 16, 8>(d, tmp, data, seg_start, 256, 24, dd, coop);
        return launch_segment_sort<E, 512, 32, 8>(d, tmp, data, seg_start, 256, 24, dd, coop);
    }
    if (cap <= 4096) return launch_segment_sort<E, 256, 16, 8>(d, tmp, data, seg_start, 256, 24, dd, coop);
    return launch_segment_sort<E, 512, 16, 8>(d, tmp, data, seg_start, 256, 24, dd, coop);
}

// Keys-only form (u32 keys: the pass on the top byte need not be stable, hybrid_kernels.hpp msd_bucket_scatter_kernel):
// TWO launches.  Its buckets are fixed to the top byte, so keys that share it (anything below 2^24) or are otherwise skewed
// overflow a slab; pass 2 then runs the cooperative LSD sort (correct, slow) and reports it (choose_mid_form).
int mid_sort_keys(adlhip_device* d, uint32_t* data, uint32_t* tmp, void* work, size_t n)
{
    typedef uint32_t E;
    const MidLayout L = mid_layout(n);
    char* wb = reinterpret_cast<char*>(work);
    E* slab = reinterpret_cast<E*>(wb + L.off_slab);
    uint32_t* state = d->d_mid_hist + 16 * 1024;
    using CA = adlhip::TileCfg<E, 8, 256, 16>;
    auto ka = adlhip::msd_bucket_scatter_kernel<E, 256, 16, 0>;
    if (ensure_lds(ka, CA::LDS_BYTES)) return ADLHIP_FAILURE;
    const uint32_t tiles = (uint32_t)((n + kMidTile - 1) / kMidTile);
    adlhip::BucketPass<E> pa;
    pa.src = data; pa.dst = slab; pa.cursors = state; pa.cursor_shift = 5; pa.src_count_shift = 0; pa.flag = state + 8192;
    pa.src_counts = nullptr; pa.n = (uint32_t)n; pa.src_stride = 0; pa.tiles_per_bucket = 1; pa.dst_stride = L.stride;
    pa.dst_total = 256u * L.stride; pa.start_bit = 24; pa.zero_me = state + 8194;
    pa.sample = nullptr; pa.which_digit = 0; pa.dst16 = 0;
    pa.place = nullptr; pa.status_a = nullptr; pa.pieces = 0; pa.rows_per_chain_a = 0; pa.slice = 0; pa.seg_shift = 8;
    pa.tickets = nullptr;
    int rc = launch(d, "mid_bucket_scatter_u32", [&] {
        hipLaunchKernelGGL(ka, dim3(tiles), dim3(256), CA::LDS_BYTES, d->stream, pa);
    });
    if (rc) return rc;
    uint32_t* ctable = reinterpret_cast<uint32_t*>(wb + L.off_coop);
    const adlhip::MidCoop coop{ctable, ctable + (size_t)256 * 256, state + 8194, (uint32_t)n};
    const adlhip::SegSlab sl{state, L.stride, d->h_fault + 10, tmp};
    if (L.stride <= 4096) return launch_segment_sort<E, 256, 16, 8>(d, slab, data, nullptr, 256, 24, nullptr, coop, sl);
    if (L.stride <= 8192) return launch_segment_sort<E, 512, 16, 8>(d, slab, data, nullptr, 256, 24, nullptr, coop, sl);
    return launch_segment_sort<E, 512, 32, 8>(d, slab, data, nullptr, 256, 24, nullptr, coop, sl);
}

// ---- large sort: two MSD passes into slabs + LDS finish ("sort.msd2") -----------------------------------------------------
// Its limits, slab and tile sizes, layouts, forms and the plan of one sort call are large_plan.hpp; here are its launches.
static_assert(kLargeTicketStride == adlhip::kTicketStride, "large_plan.hpp sizes the stable form's ticket area for the kernels' counter stride");
uint32_t net_wgs(const adlhip_device* d) { return d->resident_wgs >= (int)kNetWgsMax ? kNetWgsMax : 256u; }
// two handle-owned counters: nets run, and of those, sorted by counting (net_sort; "stat.net_runs" / "stat.net_counting")
// d_msd2: 256 first-pass cursors (one line each) + 65536 second-pass cursors + 64 words (flag, done, barrier, sample words, the
// first kernel's repeat count and arrival word, net counters)
constexpr size_t kMsd2Words = 8192 + 65536 + 64;
// Behind them, in the same allocation: the persistent passes' nine tile-ticket counters, one 128-byte line each (flag[64 + 32 i];
// hybrid_kernels.hpp kTileTicketWord0).  Reset on entry by msd2_sample_kernel, read by nothing else, and NOT part of the idle
// table's region: tests/test_gpu_call_sequences.py pins that region's size (no word flag[64] to poke).
constexpr size_t kMsd2TicketWords = (size_t)adlhip::kTileTicketCounters * adlhip::kTileTicketStride;

// ---- what the handle-owned device words hold between sorts ("debug.idle_dirty"; DESIGN.md "Idle state of a handle") ----
// Every word of d_msd2, d_mid_hist, d_dict and d_fault[0..15] is one of three kinds:
//   kIdleValue     holds `value` whenever the stream is drained: whoever changes it puts it back before its sort ends, on every exit
//   kResetOnEntry  any value: the named kernel writes it before anything of the same sort reads it
//   kFreeRunning   counters and time stamps that only ever move on
// The ranges tile each region completely (idle_table_tiles, checked at compile time).  Words no kernel touches are kIdleValue 0:
// the areas are zeroed with the handle, so a stray store into them shows.
enum IdleRegion { kRegionMsd2 = 1, kRegionMidHist = 2, kRegionDict = 3, kRegionFault = 4, kIdleRegions = 4 };
enum IdleKind { kIdleValue, kResetOnEntry, kFreeRunning };
constexpr uint32_t kMsd2CursorsB = 8192;                           // second-pass cursors = d_msd2 + kMsd2CursorsB (65536, packed)
constexpr uint32_t kMsd2Flag = kMsd2CursorsB + 65536;              // flag = d_msd2 + kMsd2Flag
constexpr uint32_t kMsd2SampleAnd = kMsd2Flag + 10, kMsd2SampleAndWords = 2;   // flag[10..11]: all ones when idle (sort_state_create)
constexpr uint32_t kMsd2NetStats = kMsd2Flag + 16;                 // flag[16..17] the net's counters, flag[20..29] its time stamps
uint32_t* net_stats(const adlhip_device* d) { return d->d_msd2 + kMsd2NetStats; }
constexpr uint32_t kMidHistWords = 16 * 1024 + 8192 + 64;
constexpr uint32_t kMidState = 16 * 1024;                          // SegSlab::state = d_mid_hist + kMidState
constexpr uint32_t kDictSmallWords = (uint32_t)(sizeof(adlhip::DictBlock) / 4);
constexpr uint32_t kDictWords = (uint32_t)((sizeof(adlhip::DictBlock) + sizeof(adlhip::BigDictBlock)) / 4);
constexpr uint32_t kFaultWords = 16;
static_assert(adlhip::kSampleRepeatsWord == 12 && adlhip::kSampleArriveWord == 13 && adlhip::kSampleThresholdWord == 14, "the idle table below");
static_assert((sizeof(adlhip::DictBlock) + sizeof(adlhip::BigDictBlock)) % 4 == 0, "d_dict is allocated and checked in words");
static_assert(kMsd2Words == kMsd2Flag + adlhip::kTileTicketWord0, "the idle table's region ends where the ticket counters start");
static_assert(adlhip::kTileTicketWord0 == 64 && adlhip::kTileTicketStride == 32, "the ticket counters start behind the flag's 64 words, one 128-byte line each");
struct IdleRange {
    int region;
    uint32_t first, count;
    IdleKind kind;
    uint32_t value;      // kIdleValue only
    const char* what;    // the word's role; who restores it (kIdleValue) or who writes it first (kResetOnEntry)
};
constexpr IdleRange kIdleTable[] = {
    // d_msd2: the large sort
    {kRegionMsd2, 0, 8192, kIdleValue, 0u, "first-pass cursors [32 * b]: last workgroup of msd2_offsets_kernel"},
    {kRegionMsd2, 8192, 65536, kIdleValue, 0u, "second-pass cursors (cursor and hybrid forms): msd2_offsets_kernel / msd2s_offsets_kernel, each its own bucket's"},
    {kRegionMsd2, kMsd2Flag + 0, 1, kIdleValue, 0u, "flag[0] overflow flag: last workgroup of msd2_offsets_kernel / msd2s_offsets_kernel"},
    {kRegionMsd2, kMsd2Flag + 1, 1, kIdleValue, 0u, "flag[1] done counter: last workgroup of msd2_offsets_kernel / msd2s_offsets_kernel"},
    {kRegionMsd2, kMsd2Flag + 2, 1, kResetOnEntry, 0u, "flag[2] the net's grid-barrier counter: msd2_sample_kernel / msd2s_prep_kernel"},
    {kRegionMsd2, kMsd2Flag + 3, 5, kIdleValue, 0u, "flag[3..7] unused"},
    {kRegionMsd2, kMsd2Flag + 8, 2, kIdleValue, 0u, "flag[8..9] sample OR words: last workgroup of msd2_offsets_kernel / last arrival of msd2s_prep_kernel"},
    {kRegionMsd2, kMsd2SampleAnd, kMsd2SampleAndWords, kIdleValue, ~0u, "flag[10..11] sample AND words: last workgroup of msd2_offsets_kernel / last arrival of msd2s_prep_kernel"},
    {kRegionMsd2, kMsd2Flag + 12, 1, kIdleValue, 0u, "flag[12] sample repeats: last workgroup of msd2_offsets_kernel / msd2s_offsets_kernel"},
    {kRegionMsd2, kMsd2Flag + 13, 1, kIdleValue, 0u, "flag[13] arrivals: last arrival of msd2s_prep_kernel"},
    {kRegionMsd2, kMsd2Flag + 14, 1, kResetOnEntry, 0u, "flag[14] repeat threshold: msd2_sample_kernel / msd2s_prep_kernel"},
    {kRegionMsd2, kMsd2Flag + 15, 1, kIdleValue, 0u, "flag[15] unused"},
    {kRegionMsd2, kMsd2NetStats, 2, kFreeRunning, 0u, "flag[16..17] nets run / sorted by counting (stat.net_runs, stat.net_counting)"},
    {kRegionMsd2, kMsd2Flag + 18, 2, kIdleValue, 0u, "flag[18..19] unused"},
    {kRegionMsd2, kMsd2NetStats + 4, 10, kFreeRunning, 0u, "flag[20..29] the last net's time stamps (debug.net_stamp0..9)"},
    {kRegionMsd2, kMsd2Flag + 30, 34, kIdleValue, 0u, "flag[30..63] unused"},
    // d_mid_hist: the mid-size sort
    {kRegionMidHist, 0, 16 * 1024, kIdleValue, 0u, "slice histograms [16][4][256]: last workgroup of mid_prep_kernel"},
    {kRegionMidHist, kMidState, 8192, kIdleValue, 0u, "two-launch form's bucket cursors [32 * b]: last reader in segment_sort_kernel"},
    {kRegionMidHist, kMidState + 8192, 2, kIdleValue, 0u, "two-launch form's overflow word and reader counter: last reader in segment_sort_kernel"},
    {kRegionMidHist, kMidState + 8194, 1, kResetOnEntry, 0u, "two-launch form's grid-barrier counter: msd_bucket_scatter_kernel (zero_me)"},
    {kRegionMidHist, kMidState + 8195, 61, kIdleValue, 0u, "unused"},
    // d_dict: the net's dictionaries, rebuilt by every net that reads them
    {kRegionDict, 0, 2, kResetOnEntry, 0u, "n_values, miss: dict_sample_build / dict_sample_build_pair_keys (workgroup 0 of the net, before its first barrier)"},
    {kRegionDict, 2, 2, kIdleValue, 0u, "pad"},
    {kRegionDict, 4, kDictSmallWords - 4, kResetOnEntry, 0u, "value, slots, count[]: dict_sample_build / dict_sample_build_pair_keys"},
    {kRegionDict, kDictSmallWords + 0, 2, kResetOnEntry, 0u, "large dictionary's n_values, miss: big_dict_build"},
    {kRegionDict, kDictSmallWords + 2, 2, kIdleValue, 0u, "pad"},
    {kRegionDict, kDictSmallWords + 4, kDictWords - kDictSmallWords - 4, kResetOnEntry, 0u, "large dictionary's value, slots: big_dict_build; count[]: big_dict_sample"},
    // d_fault
    {kRegionFault, 0, 1, kResetOnEntry, 0u, "live fault word: the first kernel of every sort whose kernels wait on one another"},
    {kRegionFault, 1, 1, kIdleValue, 0u, "sticky fault word: zero once the host has collected the report (report_fault)"},
    {kRegionFault, 2, 6, kIdleValue, 0u, "unused"},
    {kRegionFault, 8, 1, kResetOnEntry, 0u, "self-test result: run_lds_order_selftest's own memset"},
    {kRegionFault, 9, 3, kIdleValue, 0u, "unused (h_fault[9], h_fault[10] are the mid-size forms' pinned reports)"},
    {kRegionFault, 12, 1, kIdleValue, 0u, "mid_prep_kernel's arrival counter: its last workgroup"},
    {kRegionFault, 13, 1, kResetOnEntry, 0u, "three-launch form's grid-barrier counter: last workgroup of mid_prep_kernel"},
    {kRegionFault, 14, 2, kIdleValue, 0u, "unused"},
};
constexpr uint32_t idle_region_words(int region)
{
    return region == kRegionMsd2 ? (uint32_t)kMsd2Words : region == kRegionMidHist ? kMidHistWords : region == kRegionDict ? kDictWords
         : region == kRegionFault ? kFaultWords : 0u;
}
constexpr bool idle_table_tiles()
{
    int region = 0;
    uint32_t next = 0;
    for (const IdleRange& r : kIdleTable) {
        if (r.region != region) {
            if (region && next != idle_region_words(region)) return false;
            if (r.region != region + 1) return false;
            region = r.region;
            next = 0;
        }
        if (r.first != next || r.count == 0) return false;
        next += r.count;
    }
    return region == kIdleRegions && next == idle_region_words(region);
}
static_assert(idle_table_tiles(), "kIdleTable must classify every handle-owned word exactly once, regions in order");
uint32_t* idle_region_base(const adlhip_device* d, int region)
{
    return region == kRegionMsd2 ? d->d_msd2 : region == kRegionMidHist ? d->d_mid_hist
         : region == kRegionDict ? reinterpret_cast<uint32_t*>(d->d_dict) : region == kRegionFault ? d->d_fault : nullptr;
}

// "debug.idle_dirty" / "debug.idle_first": drain the stream, copy the four areas to the host, compare the kIdleValue words.  Launches
// nothing and writes nothing on the device.
int idle_check(adlhip_device* d, uint32_t* dirty, uint32_t* first)
{
    if (bind(d)) return ADLHIP_FAILURE;
    HIPCHK(hipStreamSynchronize(d->stream));
    std::vector<uint32_t> host;
    *dirty = *first = 0u;
    for (int region = 1; region <= kIdleRegions; ++region) {
        host.resize(idle_region_words(region));
        HIPCHK(hipMemcpyAsync(host.data(), idle_region_base(d, region), host.size() * 4, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        for (const IdleRange& r : kIdleTable) {
            if (r.region != region || r.kind != kIdleValue) continue;
            for (uint32_t w = r.first; w < r.first + r.count; ++w)
                if (host[w] != r.value && (*dirty)++ == 0u) *first = ((uint32_t)region << 24) | w;
        }
    }
    return ADLHIP_SUCCESS;
}

__global__ void idle_poke_kernel(uint32_t* word) { *word ^= 1u; }

// Repeats the sort's first kernel must count among its samples (hybrid_kernels.hpp sample_accumulate: 16 waves, each comparing
// its own 128 samples) to call the keys too repetitive for the slabs: D distinct values, each with n / D copies, repeat
// 16 (128 - D (1 - e^(-128/D))) times; taken at D = n / 3072 (twice what a segment slab of ~1500 holds), with 20 % off for the
// sample's noise, never below 4 (keys without repeats show none: 3e-5 expected for random 32-bit keys).  At 64 Mi keys: 4, which
// 4096 values exceed eight times over and 30 000 values (2000 copies each: no fit either) reach every other time.
uint32_t sample_dup_threshold(size_t n)
{
    const double S = 128.0, D = std::max(1.0, (double)n / 3072.0);
    return (uint32_t)std::max(4.0, 0.8 * 16.0 * (S - D * (1.0 - std::exp(-S / D))));
}

// Scratch of the net's look-back passes (hybrid_kernels.hpp coop_onesweep_sort), carved out of `region` -- the first slab area, whose
// contents are void when the net runs.  tables == nullptr when it does not fit (small inputs) or the tile status words' 30-bit
// counts would not do (n >= 2^30): the net then runs its count-scan-scatter passes.
adlhip::OsNet net_onesweep_args(const adlhip_device* d, char* region, size_t region_bytes, size_t n, int passes, uint32_t tile)
{
    adlhip::OsNet os{};
    if (!region || n >= (size_t(1) << 30) || n < (size_t(1) << 16) || !d->net_lookback) return os;
    const uint32_t total_bins = (uint32_t)passes * ((uint32_t)adlhip::kChains << 8);
    uint32_t hw = (uint32_t)std::min<size_t>(net_wgs(d), (n + adlhip::kHistChunk - 1) / adlhip::kHistChunk);
    const uint32_t per_wg = (uint32_t)align_up((n + hw - 1) / hw, 1024);
    const uint32_t wgs = (uint32_t)((n + per_wg - 1) / per_wg);
    const uint32_t wgs_per_slice = (wgs + adlhip::kChains - 1) / adlhip::kChains;
    const size_t rows = status_rows(n, tile);
    const size_t off_tables = align_up((size_t)adlhip::kTicketVecs * 16, 256);
    const size_t off_joint = align_up(off_tables + sizeof(adlhip::PassTable) * adlhip::kMaxPasses, 256);
    const size_t off_part = align_up(off_joint + (size_t)total_bins * 4, 256);
    const size_t off_status = align_up(off_part + (size_t)wgs * total_bins * 4, 256);
    const size_t total = off_status + (size_t)passes * rows * 256 * 4;
    if (total > region_bytes || (size_t)passes * rows * 256 * 4 >= (size_t(1) << 31)) return os;
    os.ctrl = reinterpret_cast<adlhip::u32x4*>(region);
    os.tables = reinterpret_cast<adlhip::PassTable*>(region + off_tables);
    os.joint = reinterpret_cast<uint32_t*>(region + off_joint);
    os.part = reinterpret_cast<uint32_t*>(region + off_part);
    os.status = reinterpret_cast<uint32_t*>(region + off_status);
    os.rows = (uint32_t)rows;
    os.hist_wgs = wgs;
    os.per_wg = per_wg;
    os.slice0 = per_wg * wgs_per_slice;
    return os;
}

template <typename E, typename S, bool SOA = false>
int launch_large_finish(adlhip_device* d, const E* slab_b, E* out, uint32_t* out_vals, uint32_t* seg_off, uint32_t* seg_cnt, uint32_t stride_b,
                        uint32_t tier_b, uint32_t* mode, uint32_t* hard, int low_bits_max, bool bin, uint32_t seg_shift = 8);

template <typename E>
int msd2_sort(adlhip_device* d, E* data, E* tmp, void* work, size_t n, const LargePlan& plan)
{
    if (plan.form != kLargeCursor) return fail("internal: the cursor form was handed another form's plan");
    constexpr int K = sizeof(E) == 4 ? 32 : 16;
    constexpr int KEY_BITS = 8 * (int)sizeof(E);
    constexpr bool k32 = sizeof(E) == 4;   // profile names are kept by pointer: literals only
    // d_msd2 (allocated at device creation): cursors of both passes + flag + done counter + sample words, idle values between sorts
    uint32_t* cur_a = d->d_msd2;            // 256 cursors, one 128-byte line each
    uint32_t* cur_b = d->d_msd2 + kMsd2CursorsB;   // 65536 cursors, packed (16 atomics each per sort)
    uint32_t* flag = d->d_msd2 + kMsd2Flag;
    uint32_t* done = flag + 1;
    uint32_t* sample = flag + 8;            // or lo, or hi, and lo, and hi (hybrid_kernels.hpp msd2_placement)
    const LargeLayout& L = plan.L;
    char* wb = reinterpret_cast<char*>(work);
    uint32_t* mode = reinterpret_cast<uint32_t*>(wb + L.off_mode);
    uint32_t* seg_cnt = reinterpret_cast<uint32_t*>(wb + L.off_cnt);
    uint32_t* seg_off = reinterpret_cast<uint32_t*>(wb + L.off_off);
    E* slab_a = reinterpret_cast<E*>(wb + L.off_slab_a);
    E* slab_b = L.slab_b_in_tmp ? tmp : reinterpret_cast<E*>(wb + L.off_slab_b);
    using CT = adlhip::TileCfg<E, 8, 512, K>;
    auto kern = adlhip::msd_bucket_scatter_kernel<E, 512, K, 1>;
    auto kern2 = adlhip::msd_bucket_scatter_kernel<E, 512, K, 2>;
    if (ensure_lds(kern, CT::LDS_BYTES) || ensure_lds(kern2, CT::LDS_BYTES)) return ADLHIP_FAILURE;
    // where the two digits sit is chosen on the device from a sample of the keys (hybrid_kernels.hpp msd2_sample_kernel).  (Folding
    // the sample into pass 1 -- every workgroup ORs and ANDs the same 1024 keys -- saves this launch and costs more than it saves:
    // 1024 strided keys are 1024 cache lines, twice a tile's own; pass 1 at 64 Mi keys 0.150 -> 0.166 ms, nothing gained at 4 Mi.)
    int rc = launch(d, "msd2_sample", [&] {
        hipLaunchKernelGGL(adlhip::msd2_sample_kernel<E>, dim3(adlhip::kSampleWGs), dim3(64), 0, d->stream, (const E*)data, (uint32_t)n,
                           sample, flag + 2, d->d_fault, flag, sample_dup_threshold(n));
    });
    if (rc) return rc;
    adlhip::BucketPass<E> pa;   // pass 1: the input, first digit -> 256 bucket slabs
    pa.src = data; pa.dst = slab_a; pa.cursors = cur_a; pa.cursor_shift = 5; pa.src_count_shift = 0; pa.flag = flag;
    pa.src_counts = nullptr; pa.n = (uint32_t)n;
    pa.src_stride = 0; pa.tiles_per_bucket = 1; pa.dst_stride = L.stride_a; pa.dst_total = 256u * L.stride_a; pa.start_bit = KEY_BITS - 8;
    pa.zero_me = nullptr; pa.sample = sample; pa.which_digit = 1; pa.dst16 = 0;
    pa.place = nullptr; pa.status_a = nullptr; pa.pieces = 0; pa.rows_per_chain_a = 0; pa.slice = 0; pa.seg_shift = 8;
    pa.tickets = flag + adlhip::kTileTicketWord0;   // zeroed by the sample kernel above
    const uint32_t tiles_a = (uint32_t)((n + CT::TILE - 1) / CT::TILE);
    // round 4: the same pass as a persistent kernel -- 2 workgroups per CU take the tiles in turns, the next tile's keys are in
    // flight (non-temporal 16-byte buffer loads) while the current one is ranked, and no wait ever covers a tile's stores
    // (persist_kernels.hpp).  Buffer addressing: the slabs must lie within 4 GiB of their base.
    const bool slab16 = plan.slab16;
    const bool persist = d->persist && (size_t)256 * L.stride_a * sizeof(E) < (size_t(1) << 32) - (1u << 20) &&
                         (size_t)L.slots * L.stride_b * (slab16 ? 2 : sizeof(E)) < (size_t(1) << 32) - (1u << 20);
    using PC = adlhip::PersistCfg<E, 512, K>;
    // a multiple of 8: workgroup % 8 = XCD ("debug.persist_grid": tests reach many rounds per workgroup with small inputs)
    const uint32_t pgrid = (uint32_t)((d->persist_grid ? d->persist_grid : 2 * d->prop.multiProcessorCount) + 7) / 8 * 8;
    // Tile tickets are drawn (the kernels' DYN = true) from six rounds of tiles up: all workgroups draw first at the same moment, 512
    // deep on pass 1's counter, about 3.5 us that fewer rounds do not win back (pass 1 + pass 2, drawing from the third round on at
    // every size, against static tickets: 24 Mi keys + 4 us, 32 Mi + 1, 40 Mi 0, 48 Mi - 6, 64 Mi - 8; profiles/tile_tickets_ab.txt).
    // Below, the static kernels of before.  One decision for both passes: pass 2 has the tiles of pass 1 plus at most one per bucket.
    // With "debug.persist_grid" set the tickets are drawn at every size: that is what tests set it for.
    constexpr uint32_t kDynamicRounds = 6;
    const bool draw = d->persist_grid != 0 || tiles_a >= kDynamicRounds * pgrid;
    if (persist) {
        auto pk = adlhip::msd_scatter_persist_kernel<E, 512, K, 1, 4, false, 2, 0, false>;
        auto pkd = adlhip::msd_scatter_persist_kernel<E, 512, K, 1, 4, false, 2, 0, true>;
        if (ensure_lds(pk, PC::LDS_BYTES) || ensure_lds(pkd, PC::LDS_BYTES)) return ADLHIP_FAILURE;
        rc = launch(d, k32 ? "msd2_pass1_u32" : "msd2_pass1_u64",
                    [&] { hipLaunchKernelGGL(draw ? pkd : pk, dim3(pgrid), dim3(512), PC::LDS_BYTES, d->stream, pa); });
    } else {
        rc = launch(d, k32 ? "msd2_pass1_u32" : "msd2_pass1_u64", [&] { hipLaunchKernelGGL(kern, dim3(tiles_a), dim3(512), CT::LDS_BYTES, d->stream, pa); });
    }
    if (rc) return rc;
    adlhip::BucketPass<E> pb = pa;   // pass 2: every bucket, second digit -> 65536 segment slabs
    pb.src = slab_a; pb.dst = slab_b; pb.cursors = cur_b; pb.cursor_shift = 0; pb.src_count_shift = 5; pb.flag = flag;
    pb.src_counts = cur_a; pb.n = (uint32_t)n;
    pb.src_stride = L.stride_a; pb.tiles_per_bucket = L.tiles_per_bucket; pb.dst_stride = L.stride_b;
    pb.dst_total = L.slots * L.stride_b; pb.start_bit = KEY_BITS - 16; pb.zero_me = nullptr;
    pb.sample = sample; pb.which_digit = 2; pb.seg_shift = L.seg_shift;
    pb.dst16 = slab16 ? 1 : 0;   // u32 keys: the second slab holds the low 16 bits only
    if (persist) {
        auto pk16 = adlhip::msd_scatter_persist_kernel<E, 512, K, 2, 4, true, 2, 0, false>;
        auto pkE = adlhip::msd_scatter_persist_kernel<E, 512, K, 2, 4, false, 2, 0, false>;
        auto pk16d = adlhip::msd_scatter_persist_kernel<E, 512, K, 2, 4, true, 2, 0, true>;
        auto pkEd = adlhip::msd_scatter_persist_kernel<E, 512, K, 2, 4, false, 2, 0, true>;
        if (ensure_lds(pk16, PC::LDS_BYTES) || ensure_lds(pkE, PC::LDS_BYTES) || ensure_lds(pk16d, PC::LDS_BYTES) ||
            ensure_lds(pkEd, PC::LDS_BYTES))
            return ADLHIP_FAILURE;
        rc = launch(d, k32 ? "msd2_pass2_u32" : "msd2_pass2_u64", [&] {
            if (slab16) hipLaunchKernelGGL(draw ? pk16d : pk16, dim3(pgrid), dim3(512), PC::LDS_BYTES, d->stream, pb);
            else hipLaunchKernelGGL(draw ? pkEd : pkE, dim3(pgrid), dim3(512), PC::LDS_BYTES, d->stream, pb);
        });
    } else {
        rc = launch(d, k32 ? "msd2_pass2_u32" : "msd2_pass2_u64", [&] {
            hipLaunchKernelGGL(kern2, dim3(256 * L.tiles_per_bucket), dim3(512), CT::LDS_BYTES, d->stream, pb);
        });
    }
    if (rc) return rc;
    // segment sizes and offsets -- and, when a run did not fit its slab, the safety net: the same 256 resident workgroups sort
    // the untouched input with the cooperative LSD sort (hybrid_kernels.hpp coop_lsd_sort); the finish then returns at once
    uint32_t* bar = done + 1;
    uint32_t* ctable = reinterpret_cast<uint32_t*>(wb + L.off_coop);
    using CC = adlhip::TileCfg<E, 8, 512, K>;   // the net's tile: the one-sweep pass's own (16 Ki keys / 8 Ki 8-byte elements)
    auto ko = adlhip::msd2_offsets_kernel<E, 512, K>;
    if (ensure_lds(ko, CC::LDS_BYTES)) return ADLHIP_FAILURE;
    rc = launch(d, "msd2_offsets", [&] {
        hipLaunchKernelGGL(ko, dim3(net_wgs(d)), dim3(512), CC::LDS_BYTES, d->stream, cur_a, cur_b, flag, done, bar,
                           seg_cnt, seg_off, mode, (uint32_t)n, sample, data, tmp, ctable, d->d_fault, KEY_BITS,
                           8u - L.seg_shift, d->dict_path ? d->d_dict : nullptr, net_stats(d),
                           net_onesweep_args(d, wb + L.off_slab_a, (size_t)256 * L.stride_a * sizeof(E), n, 4, CC::TILE));
    });
    if (rc) return rc;
    // the finish sorts the bits below the second digit (the offsets kernel has published how many)
    using S = typename std::conditional<sizeof(E) == 4, uint16_t, E>::type;   // what pass 2 wrote (w = 8)
    uint32_t* hard = reinterpret_cast<uint32_t*>(wb + L.off_hard);
    const int low_max = KEY_BITS - 8 - (int)L.seg_shift;
    if (sizeof(E) == 4 && !slab16)
        return launch_large_finish<E, E>(d, slab_b, data, nullptr, seg_off, seg_cnt, L.stride_b, L.tier_b, mode, hard, low_max, plan.bin, L.seg_shift);
    return launch_large_finish<E, S>(d, slab_b, data, nullptr, seg_off, seg_cnt, L.stride_b, L.tier_b, mode, hard, low_max, plan.bin, L.seg_shift);
}

// The finish of either large sort: the binning finish (whole u64 keys from ~24 Mi up: one counting pass + compares, then the
// LSD finish's list form for what it handed over) or the wave-per-segment LSD finish.  S = what the second slab holds.
template <typename E, typename S, bool SOA>
int launch_large_finish(adlhip_device* d, const E* slab_b, E* out, uint32_t* out_vals, uint32_t* seg_off, uint32_t* seg_cnt, uint32_t stride_b,
                        uint32_t tier_b, uint32_t* mode, uint32_t* hard, int low_bits_max, bool bin, uint32_t seg_shift)
{
    // tier_b = the tile that holds a segment (msd2_tier_b); stride_b <= tier_b = the spacing of the segment slabs;
    // 256 << seg_shift slots (hybrid_kernels.hpp slot_to_segment)
    const uint32_t* lowb = mode + adlhip::kDynLowBits;
    const size_t slots = (size_t)256 << seg_shift;
    // segments beyond a wave's tile: whole u32 keys above 280 Mi keys (16-bit second slab, 65536 segments).  The 5120-key tier
    // (about 140 Mi ... 288 Mi keys) goes the same way: four waves with 20 rows per thread beat the one wave that holds 80
    // (256 Mi keys: finish 0.64 -> 0.48 ms, 144 Mi: 0.80 -> 0.35); below, the wave per segment stays ahead (64 Mi keys: 0.125 vs
    // 0.129 ms, 128 Mi: 0.218 vs 0.235).  Workgroup sizes by measurement (profiles/r3_wg_finish.txt): 5120 keys 256 x 20 | 512 x 10
    // = 0.478 | 0.606 ms at 256 Mi keys; 8192: 256 x 32 | 512 x 16 = 0.672 | 0.731 at 384 Mi; 12288: 512 x 24 | 256 x 48 = 1.047 |
    // 1.089 at 512 Mi; 16384 keys with 1024 x 16 took 2.37 ms against 1.63 with 512 x 32 at 768 Mi
    constexpr bool wg_kind = !SOA && sizeof(E) == 4 && sizeof(S) == 2;
    // round 4: 16-bit keys stay 16 bits wide in the finish (finish16_kernels.hpp): tiles of 1280 / 1536 / 2560 keys, one wave each
    if constexpr (wg_kind) {
        if (d->persist && !bin && seg_shift == 8 && tier_b <= 2560 && (stride_b & 1u) == 0u) {
            const uint16_t* sb = reinterpret_cast<const uint16_t*>(slab_b);
#define ADLHIP_F16(R2_, WAVES_)                                                                                                      \
    {                                                                                                                                \
        auto kf = adlhip::wave_finish16_kernel<R2_, WAVES_>;                                                                         \
        const size_t lds = (size_t)WAVES_ * adlhip::Finish16Cfg<R2_>::PER_WAVE;                                                      \
        if (ensure_lds(kf, lds)) return ADLHIP_FAILURE;                                                                              \
        return launch(d, "segment_sort_wave_u32", [&] {                                                                              \
            hipLaunchKernelGGL(kf, dim3((uint32_t)((slots + WAVES_ - 1) / WAVES_)), dim3(64 * WAVES_), lds, d->stream, sb, out, seg_off,       \
                               seg_cnt, stride_b, mode, lowb, (uint32_t)slots, d->d_fault);                                          \
        });                                                                                                                          \
    }
            if (tier_b <= 1280) ADLHIP_F16(10, 4)
            if (tier_b <= 1536) ADLHIP_F16(12, 4)
            ADLHIP_F16(20, 4)
#undef ADLHIP_F16
        }
    }
    if (tier_b > 5120 || (wg_kind && tier_b >= 3072 && seg_shift == 8)) {
        if constexpr (wg_kind) {
            const S* sb = reinterpret_cast<const S*>(slab_b);
            if (seg_shift != 8) return fail("internal: the workgroup-per-segment finish takes 65536 segments");
#define ADLHIP_WG(NT_, K_) return launch_wg_segment_sort<E, S, NT_, K_>(d, sb, out, seg_off, seg_cnt, stride_b, mode, slots)
            switch (tier_b) {
            case 3072: ADLHIP_WG(256, 12);
            case 4096: ADLHIP_WG(256, 16);
            case 5120: ADLHIP_WG(256, 20);
            case 8192: ADLHIP_WG(256, 32);
            case 12288: ADLHIP_WG(512, 24);
            case 16384: ADLHIP_WG(512, 32);
            default: ADLHIP_WG(512, 40);
            }
#undef ADLHIP_WG
        } else {
            return fail("internal: no finish for segments of %u elements of this kind", tier_b);
        }
    }
    if constexpr (!SOA) {
        if (bin) {
            const S* sb = reinterpret_cast<const S*>(slab_b);
            int rc;
            if (tier_b <= kMsd2Stride0) rc = launch_bin_segment_sort<E, S, 256, 6, 11>(d, sb, out, seg_off, seg_cnt, stride_b, mode, hard, seg_shift);
            else if (tier_b == 2560) rc = launch_bin_segment_sort<E, S, 256, 10, 12>(d, sb, out, seg_off, seg_cnt, stride_b, mode, hard, seg_shift);
            else rc = launch_bin_segment_sort<E, S, 512, 10, 12>(d, sb, out, seg_off, seg_cnt, stride_b, mode, hard, seg_shift);
            if (rc) return rc;
            const uint32_t* hc = mode + adlhip::kDynHardCnt;
            if (tier_b <= kMsd2Stride0) return launch_wave_segment_sort<E, kMsd2Stride0 / 64, S>(d, slab_b, out, seg_off, slots, low_bits_max, seg_cnt, stride_b, mode, lowb, nullptr, hard, hc, seg_shift);
            if (tier_b == 2560) return launch_wave_segment_sort<E, 40, S>(d, slab_b, out, seg_off, slots, low_bits_max, seg_cnt, stride_b, mode, lowb, nullptr, hard, hc, seg_shift);
            return launch_wave_segment_sort<E, 80, S>(d, slab_b, out, seg_off, slots, low_bits_max, seg_cnt, stride_b, mode, lowb, nullptr, hard, hc, seg_shift);
        }
    }
    if constexpr (sizeof(E) == 8 && sizeof(S) == 8) {
        if (d->rank_mode == 0) {   // "sort.rank" = 0 (pairs; large_sort_form keeps n within these tiles): the ballot-ranked finish
            if (tier_b == 1280) return launch_wave_segment_sort<E, 20, S, SOA, 0>(d, slab_b, out, seg_off, slots, low_bits_max, seg_cnt, stride_b, mode, lowb, out_vals, nullptr, nullptr, seg_shift);
            if (tier_b == kMsd2Stride0) return launch_wave_segment_sort<E, kMsd2Stride0 / 64, S, SOA, 0>(d, slab_b, out, seg_off, slots, low_bits_max, seg_cnt, stride_b, mode, lowb, out_vals, nullptr, nullptr, seg_shift);
            if (tier_b == 2560) return launch_wave_segment_sort<E, 40, S, SOA, 0>(d, slab_b, out, seg_off, slots, low_bits_max, seg_cnt, stride_b, mode, lowb, out_vals, nullptr, nullptr, seg_shift);
            return fail("internal: no ballot-ranked finish for segments of %u elements", tier_b);
        }
    }
    if (tier_b == 1280) return launch_wave_segment_sort<E, 20, S, SOA>(d, slab_b, out, seg_off, slots, low_bits_max, seg_cnt, stride_b, mode, lowb, out_vals, nullptr, nullptr, seg_shift);
    if (tier_b == kMsd2Stride0) return launch_wave_segment_sort<E, kMsd2Stride0 / 64, S, SOA>(d, slab_b, out, seg_off, slots, low_bits_max, seg_cnt, stride_b, mode, lowb, out_vals, nullptr, nullptr, seg_shift);
    if (tier_b == 2560) return launch_wave_segment_sort<E, 40, S, SOA>(d, slab_b, out, seg_off, slots, low_bits_max, seg_cnt, stride_b, mode, lowb, out_vals, nullptr, nullptr, seg_shift);
    return launch_wave_segment_sort<E, 80, S, SOA>(d, slab_b, out, seg_off, slots, low_bits_max, seg_cnt, stride_b, mode, lowb, out_vals, nullptr, nullptr, seg_shift);
}

// The stable large sort.  E / KEY64: uint64_t / false = {key, value} pairs (AoS: data / tmp; SoA: soa_keys != nullptr, the input and
// output are the two u32 arrays, data / tmp are unused -- the safety net packs the input into the first slab area and sorts it
// there against the second); uint64_t / true = u64 keys; uint32_t / false = u32 keys (whole keys: the second slab holds their low
// 16 bits, as in the cursor form).  sort_bits < key bits (Pprims.cpp:357, a multiple of 4, at least 16 here): only the low sort_bits
// bits of a key count -- the digits are placed inside them, everything is stable, so keys that agree there keep their input order
// as the reference's LSD passes would leave them.
// hybrid (whole keys only -- equal keys are indistinguishable, so the second pass need not be stable): pass A as above, then the
// CURSOR-placed second pass of the keys-only form over buckets made of pass A's sub-slabs (msd_bucket_scatter_kernel, PASS = 3).
// Measured per pass at 64 Mi u32 keys: first pass 0.138 ms by look-back vs 0.147-0.159 with cursors (the abutting runs of a
// chain's consecutive tiles meet in one XCD's L2: 1.05 x instead of 1.21 x bytes written), second pass 0.124 with cursors vs
// 0.172 by look-back (profiles/r3_first_ab_cursor_vs_lookback_u32.txt).
template <typename E, bool KEY64>
int msd2s_sort(adlhip_device* d, E* data, E* tmp, void* work, size_t n, int sort_bits, const LargePlan& plan, uint32_t* soa_keys = nullptr,
               uint32_t* soa_vals = nullptr)
{
    if (plan.form != kLargeStable && plan.form != kLargeHybrid) return fail("internal: the stable form was handed another form's plan");
    const bool hybrid = plan.form == kLargeHybrid;
    constexpr int K = sizeof(E) == 8 ? 16 : 32;
    constexpr bool k32 = sizeof(E) == 4;
    constexpr int KEY_BITS = KEY64 ? 64 : 32;
    const bool whole = sort_bits == KEY_BITS;
    uint32_t* flag = d->d_msd2 + kMsd2Flag;
    uint32_t* done = flag + 1;
    uint32_t* bar = flag + 2;
    const LargeLayout& L = plan.L;
    if (L.total == 0) return fail("internal: layout bounds of the stable large sort");
    char* wb = reinterpret_cast<char*>(work);
    uint32_t* mode = reinterpret_cast<uint32_t*>(wb + L.off_mode);
    adlhip::StablePlace* place = reinterpret_cast<adlhip::StablePlace*>(wb + L.off_place);
    uint32_t* seg_cnt = reinterpret_cast<uint32_t*>(wb + L.off_cnt);
    uint32_t* seg_off = reinterpret_cast<uint32_t*>(wb + L.off_off);
    uint32_t* hard = reinterpret_cast<uint32_t*>(wb + L.off_hard);
    uint32_t* tickets = reinterpret_cast<uint32_t*>(wb + L.off_tickets);
    uint32_t* status_a = reinterpret_cast<uint32_t*>(wb + L.off_status_a);
    uint32_t* status_b = reinterpret_cast<uint32_t*>(wb + L.off_status_b);
    E* slab_a = reinterpret_cast<E*>(wb + L.off_slab_a);
    E* slab_b = L.slab_b_in_tmp ? tmp : reinterpret_cast<E*>(wb + L.off_slab_b);
    using CT = adlhip::TileCfg<E, 8, 512, K>;
    static_assert(CT::TILE == (int)msd2s_tile(sizeof(E)), "layout and kernel agree on the tile");
    auto kern = adlhip::msd_lookback_scatter_kernel<E, 512, K, KEY64>;
    if constexpr (sizeof(E) == 8 && !KEY64) {   // pairs with "sort.rank" = 0: ballot ranking in the passes (and in the finish, below)
        if (d->rank_mode == 0) kern = adlhip::msd_lookback_scatter_kernel<E, 512, K, KEY64, 0>;
    }
    if (ensure_lds(kern, CT::LDS_BYTES)) return ADLHIP_FAILURE;
    // status rows of both passes: zero (one memset; the rows are contiguous).  Hybrid: pass A's only.
    HIPCHK(hipMemsetAsync(status_a, 0, hybrid ? L.status_bytes_a : (L.off_status_b - L.off_status_a) + L.status_bytes_b, d->stream));
    const uint32_t dup_thr = sample_dup_threshold(n);
    int rc = launch(d, "msd2s_prep", [&] {
        if (soa_keys)
            hipLaunchKernelGGL((adlhip::msd2s_prep_kernel<uint32_t, false>), dim3(adlhip::kSampleWGs), dim3(64), 0, d->stream, (const uint32_t*)soa_keys,
                               (uint32_t)n, place, tickets, L.ticket_words, bar, d->d_fault, (uint32_t)sort_bits, flag, dup_thr);
        else
            hipLaunchKernelGGL((adlhip::msd2s_prep_kernel<E, KEY64>), dim3(adlhip::kSampleWGs), dim3(64), 0, d->stream, (const E*)data, (uint32_t)n, place,
                               tickets, L.ticket_words, bar, d->d_fault, (uint32_t)sort_bits, flag, dup_thr);
    });
    if (rc) return rc;
    adlhip::LookbackPass<E> pa;
    pa.src = data; pa.dst = slab_a; pa.status = status_a; pa.status_bytes = (uint32_t)L.status_bytes_a; pa.tickets = tickets;
    pa.flag = flag; pa.fault = d->d_fault; pa.place = place; pa.which_digit = 1; pa.n = (uint32_t)n; pa.chains = L.pieces; pa.pieces = L.pieces;
    pa.rows_per_chain = L.rows_a; pa.slice = L.slice; pa.src_stride = 0; pa.status_a = nullptr; pa.rows_per_chain_a = 0;
    pa.dst_stride = L.stride_a; pa.dst_total = 256u * L.pieces * L.stride_a;
    pa.soa_keys = soa_keys; pa.soa_vals = soa_vals; pa.dst16 = 0; pa.seg_shift = 8;
    rc = launch(d, k32 ? "msd2s_pass1_u32" : KEY64 ? "msd2s_pass1_u64" : soa_keys ? "msd2s_pass1_soa" : "msd2s_pass1_kv32", [&] {
        hipLaunchKernelGGL(kern, dim3(L.pieces * L.rows_a), dim3(512), CT::LDS_BYTES, d->stream, pa);
    });
    if (rc) return rc;
    const bool slab16 = plan.slab16;    // whole u32 keys: a segment's keys share everything above their low 16 bits
    uint32_t* cur_b = nullptr;
    if constexpr (sizeof(E) == 4 || KEY64) {
        if (hybrid) {
            if (!whole || soa_keys) return fail("internal: the hybrid form sorts whole keys only");
            cur_b = d->d_msd2 + kMsd2CursorsB;   // 65536 cursors [bucket][digit], zero between sorts (the offsets kernel clears them)
            auto kern2 = adlhip::msd_bucket_scatter_kernel<E, 512, K, 3>;
            if (ensure_lds(kern2, CT::LDS_BYTES)) return ADLHIP_FAILURE;
            adlhip::BucketPass<E> pc;
            pc.src = slab_a; pc.dst = slab_b; pc.cursors = cur_b; pc.cursor_shift = 0; pc.src_count_shift = 0; pc.flag = flag;
            pc.src_counts = nullptr; pc.n = (uint32_t)n; pc.src_stride = L.stride_a; pc.tiles_per_bucket = L.rows_b;
            pc.dst_stride = L.stride_b; pc.dst_total = L.slots * L.stride_b; pc.start_bit = 0; pc.zero_me = nullptr; pc.sample = nullptr;
            pc.which_digit = 2; pc.dst16 = slab16 ? 1 : 0;
            pc.place = place; pc.status_a = status_a; pc.pieces = L.pieces; pc.rows_per_chain_a = L.rows_a; pc.slice = L.slice;
            pc.seg_shift = L.seg_shift; pc.tickets = nullptr;
            rc = launch(d, k32 ? "msd2h_pass2_u32" : "msd2h_pass2_u64", [&] {
                hipLaunchKernelGGL(kern2, dim3(256 * L.rows_b), dim3(512), CT::LDS_BYTES, d->stream, pc);
            });
            if (rc) return rc;
        }
    }
    adlhip::LookbackPass<E> pb = pa;
    pb.src = slab_a; pb.dst = slab_b; pb.status = status_b; pb.status_bytes = (uint32_t)L.status_bytes_b;
    pb.tickets = tickets + 32 * adlhip::kTicketStride; pb.which_digit = 2; pb.chains = 256; pb.rows_per_chain = L.rows_b;
    pb.src_stride = L.stride_a; pb.status_a = status_a; pb.rows_per_chain_a = L.rows_a; pb.dst_stride = L.stride_b;
    pb.dst_total = L.slots * L.stride_b; pb.seg_shift = L.seg_shift;
    pb.soa_keys = nullptr; pb.soa_vals = nullptr;
    pb.dst16 = slab16 ? 1 : 0;
    if (!cur_b) {
        rc = launch(d, k32 ? "msd2s_pass2_u32" : KEY64 ? "msd2s_pass2_u64" : soa_keys ? "msd2s_pass2_soa" : "msd2s_pass2_kv32", [&] {
            hipLaunchKernelGGL(kern, dim3(256 * L.rows_b), dim3(512), CT::LDS_BYTES, d->stream, pb);
        });
        if (rc) return rc;
    }
    uint32_t* ctable = reinterpret_cast<uint32_t*>(wb + L.off_coop);
    constexpr int NK = sizeof(E) == 4 ? 32 : 16;
    // whole-key sorts: keys of few values are sorted by counting (equal keys are interchangeable), pairs with such keys by ONE
    // stable pass on the key's rank among the values (dict_kernels.hpp)
    adlhip::DictBlock* net_dict = whole && (!soa_keys || sizeof(E) == 8) && d->dict_path ? d->d_dict : nullptr;
    using CC = adlhip::TileCfg<E, 8, 512, NK>;   // the safety net's tile (it runs in the offsets kernel when a run did not fit)
    // the net's look-back passes: whole keys; SoA input (packed into the first slab area) and sorts on part of the key run its
    // count-scan-scatter passes
    constexpr int NP = KEY64 ? 8 : 4;   // key bytes: passes of the net's look-back sort (run four at a time)
    auto ko = adlhip::msd2s_offsets_kernel<E, CT::TILE, 512, NK, 1, NP>;
    if constexpr (sizeof(E) == 8 && !KEY64) {
        if (d->rank_mode == 0) ko = adlhip::msd2s_offsets_kernel<E, CT::TILE, 512, NK, 0, NP>;   // the net ranks by ballots too
    }
    if (ensure_lds(ko, CC::LDS_BYTES)) return ADLHIP_FAILURE;
    const adlhip::OsNet os = net_onesweep_args(d, (NP && whole && !soa_keys) ? wb + L.off_slab_a : nullptr, L.off_slab_b - L.off_slab_a, n, 4, CC::TILE);
    rc = launch(d, "msd2s_offsets", [&] {
        hipLaunchKernelGGL(ko, dim3(net_wgs(d)), dim3(512), CC::LDS_BYTES, d->stream,
                           (const uint32_t*)status_a, L.rows_a, L.slice, L.pieces, (const uint32_t*)status_b, L.rows_b, L.stride_a, flag,
                           done, bar, seg_cnt, seg_off, mode, (uint32_t)n, (const adlhip::StablePlace*)place,
                           soa_keys ? slab_a : data, soa_keys ? slab_b : tmp, ctable, d->d_fault, soa_keys, soa_vals, cur_b, 8u - L.seg_shift,
                           net_dict, net_stats(d), os);
    });
    if (rc) return rc;
    const int low_max = sort_bits - 8 - (int)L.seg_shift;
    const bool bin = plan.bin;
    if constexpr (k32) {
        if (slab16) return launch_large_finish<E, uint16_t>(d, slab_b, data, nullptr, seg_off, seg_cnt, L.stride_b, L.tier_b, mode, hard, low_max, bin, L.seg_shift);
        return launch_large_finish<E, E>(d, slab_b, data, nullptr, seg_off, seg_cnt, L.stride_b, L.tier_b, mode, hard, low_max, false, L.seg_shift);
    } else {
        if (soa_keys)   // the finish writes keys and values to their own arrays
            return launch_large_finish<E, E, true>(d, slab_b, reinterpret_cast<E*>(soa_keys), soa_vals, seg_off, seg_cnt, L.stride_b, L.tier_b, mode,
                                                   hard, low_max, false, L.seg_shift);
        return launch_large_finish<E, E>(d, slab_b, data, nullptr, seg_off, seg_cnt, L.stride_b, L.tier_b, mode, hard, low_max, bin, L.seg_shift);
    }
}

// Work bytes with which a sort of n elements on sort_bits bits runs at full speed (level 1), or runs at all (level 0: the
// per-digit three-kernel passes -- the reference's own contract: a table of a few KiB beside the n-element partner array,
// Pprims.cpp:332-337), or keeps the large sort for whole u32 / u64 keys with 12 % instead of 50 % of head-room in the first
// slabs (level 2, "lean": 64 Mi u32 keys 307 MB instead of 451).  With anything in between, every path checks its own need and
// the sort takes the fastest one that fits.
size_t sort_work_bytes_at(const adlhip_device* d, int elem_kind, size_t n, int sort_bits, int level)
{
    const size_t a = work_bytes_three_kernel(d, n);
    if (level == 0) return a;
    size_t b;
    if (elem_kind == ADLHIP_ELEM_U32) b = onesweep_layout(d, n, max_passes_for(d, 32), buf_tile<AosBuf<uint32_t>>(d, n)).total;
    else if (elem_kind == ADLHIP_ELEM_SOA32) b = onesweep_layout(d, n, max_passes_for(d, 64), buf_tile<SoaBuf>(d, n)).total;
    else b = onesweep_layout(d, n, max_passes_for(d, 64), buf_tile<AosBuf<uint64_t>>(d, n)).total;   // as onesweep_sort<Buf>()
    const size_t c = n <= kMidMaxU32 ? mid_layout(n).total : mid_layout(kMidMaxU32).total;   // mid-size sort (monotone in n)
    const size_t e = large_work_bytes_at(elem_kind, n, sort_bits, level);   // the large sort (large_plan.hpp)
    return std::max(std::max(a, b), std::max(c, e));
}

// Work bytes that suffice for EVERY n' <= n with the current knobs: the requirement of one n is not monotone (a smaller
// input selects a smaller tile, which needs more status rows; from 16 Mi keys the second slab of whole u32 keys moves into the
// partner array), so a caller that sizes its scratch once for its largest batch must get the maximum over the sizes at which
// such a choice changes.  Changing "sort.tile", "sort.digit_bits" or "sort.algo" afterwards can raise the requirement.
}  // namespace
size_t adlhip_internal::sort_work_bytes(const adlhip_device* d, int elem_kind, size_t n, int sort_bits, int level)
{
    const size_t esz = (elem_kind == ADLHIP_ELEM_U32) ? 4 : 8;
    size_t need = sort_work_bytes_at(d, elem_kind, n, sort_bits, level);
    for (size_t edge : {(size_t(8) << 20) / esz, (size_t(24) << 20) / esz - 1, kSlabInTmpMin - 1, kMsd2sMax, kMsd2MaxU32})
        if (edge < n) need = std::max(need, sort_work_bytes_at(d, elem_kind, edge, sort_bits, level));
    return need;
}
namespace {

// choose the path (shared by the AoS and SoA entry points)
template <typename Buf>
int run_sort(adlhip_device* d, Buf data, Buf tmp, void* work, size_t work_bytes, size_t n, const std::vector<PassPlan>& plan)
{
    {   // a work buffer sized by the reference's contract (level 0) holds the three-kernel pass's table and nothing else
        const size_t os = onesweep_layout(d, n, max_passes_for(d, Buf::kElemBytes == 4 && !Buf::kSoa ? 32 : 64), buf_tile<Buf>(d, n)).total;
        if (work_bytes < os) {
            if (d->sort_algo == 0)
                return fail("work buffer too small for the one-sweep path the knobs ask for: %zu < %zu (adlhip_radix_sort_scratch_bytes)",
                            work_bytes, os);
            return three_kernel_sort<Buf>(d, data, tmp, work, n, plan);
        }
    }
    if (d->sort_algo < 0) {   // automatic choice by size (profiles/r1_ncurve.txt)
        // the one-sweep path has more fixed cost (histogram, tables) and wins from ~24 MiB of data (fresh random keys,
        // profiles/r1_ncurve.txt: 4Mi u32 keys 78 vs 88 us, 8Mi 124 vs 117 us, 16Mi 224 vs 174 us)
        // (AoS pairs: from ~36 MiB; 4 Mi pairs 0.103 vs 0.125 ms, 5 Mi pairs 0.149 vs 0.127 ms)
        const size_t edge = (Buf::kElemBytes == 8 && !Buf::kSoa) ? (size_t(36) << 20) : (size_t(24) << 20);
        if (n * Buf::kElemBytes < edge) return three_kernel_sort<Buf>(d, data, tmp, work, n, plan);
    }
    // tile status words carry 30-bit counts: beyond 2^30 elements use the table-based pass
    if (d->sort_algo == 1 || n >= (size_t(1) << 30)) return three_kernel_sort<Buf>(d, data, tmp, work, n, plan);
    return onesweep_sort<Buf>(d, data, tmp, work, n, plan);
}

int check_sort_args(adlhip_device* d, int elem_kind, const void* a, const void* b, const void* work, size_t work_bytes,
                    size_t n, int sort_bits, int max_bits)
{
    if (sort_bits < 4 || sort_bits > max_bits || (sort_bits & 3))   // Pprims.cpp:330
        return fail("sort_bits must be a multiple of 4 in [4,%d], got %d", max_bits, sort_bits);
    if (n > kMaxElems) return fail("n = %zu exceeds the supported maximum %zu", n, (size_t)kMaxElems);
    if (n == 0) return ADLHIP_SUCCESS;
    if (!a || !b || !work) return fail("null buffer passed to radix sort");
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(work)) & 15u)
        return fail("sort buffers must be 16-byte aligned");
    const size_t need = sort_work_bytes(d, elem_kind, n, sort_bits, 0);
    if (work_bytes < need)
        return fail("work buffer too small: %zu < %zu (the minimum; adlhip_radix_sort_scratch_bytes gives the size for full speed)",
                    work_bytes, need);
    return ADLHIP_SUCCESS;
}

template <typename E>
int sort_entry(adlhip_device* d, int elem_kind, E* data, E* tmp, void* work, size_t work_bytes, size_t n,
               int sort_bits, int max_bits)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (check_sort_args(d, elem_kind, data, tmp, work, work_bytes, n, sort_bits, max_bits)) return ADLHIP_FAILURE;
    if (n == 0) return ADLHIP_SUCCESS;
    if (trace_level())
        fprintf(stderr, "[adlhip] sort kind %d n %zu bits %d data %p tmp %p work %p + %zu\n", elem_kind, n, sort_bits, (void*)data, (void*)tmp,
                work, work_bytes);
    const std::vector<PassPlan> plan = plan_passes(sort_bits, d->digit_bits);
    // one workgroup, one launch -- except u32 keys just below its limit, which the two-launch mid-size sort does faster (while
    // the mid-size sort's own reports do not keep them off it, choose_mid_form)
    const bool small = d->sort_algo < 0 && n <= kSmallMax;
    const bool small_mid = small && sizeof(E) == 4 && sort_bits == max_bits && n > kMidMinU32 && (d->mid_path == 2 || d->mid2_skip == 0);
    if (small && !small_mid) return small_sort<E>(d, data, n, plan);
    if (mid_eligible(d, sizeof(E), n, sort_bits, max_bits) && mid_layout(n).total <= work_bytes) {
        const int form = choose_mid_form(d, sizeof(E) == 4);
        if constexpr (sizeof(E) == 4) {
            if (form == 2) return mid_sort_keys(d, data, tmp, work, n);   // two launches
        }
        if (small) return small_sort<E>(d, data, n, plan);                // (a small input never takes the slower forms)
        if (form == 3) return mid_sort<E>(d, data, tmp, work, n);         // three launches
    }
    if (small) return small_sort<E>(d, data, n, plan);
    const bool keys = (int)sizeof(E) * 8 == max_bits;
    // the form, its head-room and its layout, by what the caller's work buffer holds (large_plan.hpp)
    const LargePlan large = large_plan(d, sizeof(E), keys, n, sort_bits, max_bits, work_bytes);
    // The large sort takes every input it is eligible for by size, bits and scratch -- whatever the keys are like: runs that do not fit
    // their slabs are detected on the device and the sort's own offsets kernel then sorts the untouched input (net_sort: counting
    // sort for few distinct values, else LSD passes with grid barriers).  Nothing is reported to the host and nothing is remembered:
    // a handle's first sort of an input takes the time its hundredth does.
    if (large.form != kLargeNone) {
        if (large.form == kLargeCursor) return msd2_sort<E>(d, data, tmp, work, n, large);
        if constexpr (sizeof(E) == 4) {
            return msd2s_sort<E, false>(d, data, tmp, work, n, sort_bits, large);
        } else {
            if (keys) return msd2s_sort<E, true>(d, data, tmp, work, n, sort_bits, large);
            return msd2s_sort<E, false>(d, data, tmp, work, n, sort_bits, large);
        }
    }
    return run_sort<AosBuf<E>>(d, AosBuf<E>{data}, AosBuf<E>{tmp}, work, work_bytes, n, plan);
}

}  // namespace
int adlhip_internal::sort_elements(adlhip_device* d, int elem_kind, void* data, void* tmp, void* work, size_t work_bytes, size_t n, int sort_bits)
{
    if (elem_kind == ADLHIP_ELEM_U32) return sort_entry<uint32_t>(d, elem_kind, (uint32_t*)data, (uint32_t*)tmp, work, work_bytes, n, sort_bits, 32);
    return sort_entry<uint64_t>(d, elem_kind, (uint64_t*)data, (uint64_t*)tmp, work, work_bytes, n, sort_bits, elem_kind == ADLHIP_ELEM_U64 ? 64 : 32);
}

int adlhip_internal::launch_scan_single(adlhip_device* d, const char* name, const uint32_t* src, uint32_t* dst, size_t n, uint32_t* d_total)
{
    return launch(d, name, [&] { hipLaunchKernelGGL(adlhip::scan_single_kernel, dim3(1), dim3(adlhip::kScanNT), 0, d->stream, src, dst, n, d_total); });
}
namespace {

// ---- MSB partition (multi-GPU send side) -----------------------------------------------------------
// E = uint32_t (keys) or uint64_t ({key, value} pairs: the key is the low dword, so its top byte is bits 24..31)

// One three-kernel pass on the top byte: out = in, stably ordered by bits 24..31; *totals_at (device pointer into the
// work buffer) = the 256 digit totals.
template <typename E>
int partition_top_byte(adlhip_device* d, const E* in, E* out, void* work, size_t work_bytes, size_t n, uint32_t** totals_at)
{
    if (n > kMaxElems) return fail("n too large");
    if (!in || !out) return fail("null buffer");
    const size_t need = work_bytes_three_kernel(d, n);
    if (work_bytes < need || !work) return fail("work buffer too small: %zu < %zu", work_bytes, need);
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(work)) & 15u)
        return fail("buffers must be 16-byte aligned");
    // From 24 MiB of data, and with a work buffer of the sort's full-speed size: ONE look-back pass on the top byte -- the one-sweep
    // path's histogram, tables and chain kernel with a one-pass plan -- instead of count -> scan -> scatter: the keys are read twice
    // instead of three times and there is no table scan (64 Mi keys: 0.26 -> ~0.19 ms).  Both are stable: the same output, bit for bit.
    if (d->sort_algo != 1 && d->digit_bits == 8 && d->partition_lookback && n * sizeof(E) >= (size_t(24) << 20) && n < (size_t(1) << 30) &&
        onesweep_layout(d, n, max_passes_for(d, sizeof(E) == 4 ? 32 : 64), buf_tile<AosBuf<E>>(d, n)).total <= work_bytes) {
        const std::vector<PassPlan> plan{PassPlan{24, 8}};
        return onesweep_sort<AosBuf<E>>(d, AosBuf<E>{const_cast<E*>(in)}, AosBuf<E>{out}, work, n, plan, /*copy_back=*/false, totals_at);
    }
    int rc = three_kernel_pass<AosBuf<E>, 8>(d, AosBuf<E>{const_cast<E*>(in)}, AosBuf<E>{out}, work, n, 24, /*need_totals=*/true);
    if (rc) return rc;
    *totals_at = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(work) + table_bytes(d, n, kMinTile));
    return ADLHIP_SUCCESS;
}

template <typename E>
int partition_msb(adlhip_device* d, const E* in, E* out, uint32_t* counts, void* work, size_t work_bytes, size_t n,
                         int num_buckets)
{
    if (bind(d)) return ADLHIP_FAILURE;
    int lg = 0;
    while ((1 << lg) < num_buckets) ++lg;
    if (num_buckets < 1 || num_buckets > 256 || (1 << lg) != num_buckets)
        return fail("num_buckets must be a power of two in [1,256], got %d", num_buckets);
    if (!counts) return fail("null counts pointer");
    if (n > kMaxElems) return fail("n too large");
    if (n == 0 || num_buckets == 1) {
        HIPCHK(hipMemsetAsync(counts, 0, 4 * (size_t)num_buckets, d->stream));
        if (n) {
            if (!in || !out) return fail("null buffer");
            HIPCHK(hipMemcpyAsync(out, in, n * sizeof(E), hipMemcpyDeviceToDevice, d->stream));
            return adlhip_fill_u32(d, counts, (uint32_t)n, 1);   // counts[0] = n  (stream-ordered fill of one word: one workgroup)
        }
        return ADLHIP_SUCCESS;
    }
    // one three-kernel pass on the top byte (the top `lg` bits decide the bucket; ordering by the
    // whole top byte refines buckets without mixing them), then fold the 256 digit totals into buckets
    uint32_t* totals = nullptr;
    int rc = partition_top_byte<E>(d, in, out, work, work_bytes, n, &totals);
    if (rc) return rc;
    return launch(d, "fold_buckets", [&] {
        hipLaunchKernelGGL(adlhip::fold_buckets_kernel, dim3(1), dim3(256), 0, d->stream, (const uint32_t*)totals, counts, num_buckets);
    });
}

// the same pass with the 256 top-byte totals handed to the caller (who chooses balanced splitters from them)
template <typename E>
int partition_top_byte_entry(adlhip_device* d, const E* in, E* out, uint32_t* totals256, void* work, size_t work_bytes, size_t n)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!totals256) return fail("null totals pointer");
    if (n == 0) {
        HIPCHK(hipMemsetAsync(totals256, 0, 256 * 4, d->stream));
        return ADLHIP_SUCCESS;
    }
    uint32_t* totals = nullptr;
    int rc = partition_top_byte<E>(d, in, out, work, work_bytes, n, &totals);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(totals256, totals, 256 * 4, hipMemcpyDeviceToDevice, d->stream));
    return ADLHIP_SUCCESS;
}

// ---- SoA key-value sort with 4- / 8-byte keys and 4- / 8- / 16-byte values (soa_wide_kernels.hpp) -----------------------------
}  // namespace
SoaWideLayout adlhip_internal::soa_wide_layout(const adlhip_device* d, size_t n)
{
    SoaWideLayout L;
    L.off_pairs_a = 0;
    L.off_pairs_b = align_up(n * 8, 256);
    L.off_kv = 2 * L.off_pairs_b;
    L.kv_bytes = sort_work_bytes(d, ADLHIP_ELEM_KV32, n, 32, 1);   // (whole keys need the least of the large sort's forms; partial
    L.kv_bytes = std::max(L.kv_bytes, sort_work_bytes(d, ADLHIP_ELEM_KV32, n, 28, 1));   // sorts the most: size for either)
    L.total = L.off_kv + L.kv_bytes;
    return L;
}

int adlhip_internal::soa_check_widths(int key_bytes, int value_bytes)
{
    if (key_bytes != 4 && key_bytes != 8) return fail("key_bytes must be 4 or 8, got %d", key_bytes);
    if (value_bytes != 4 && value_bytes != 8 && value_bytes != 16) return fail("value_bytes must be 4, 8 or 16, got %d", value_bytes);
    return ADLHIP_SUCCESS;
}
namespace {

template <typename K, typename V>
int soa_wide_sort(adlhip_device* d, K* keys, V* vals, K* tmp_keys, V* tmp_vals, void* work, size_t n, int sort_bits)
{
    const SoaWideLayout L = soa_wide_layout(d, n);
    char* w = static_cast<char*>(work);
    uint64_t* pa = reinterpret_cast<uint64_t*>(w + L.off_pairs_a);
    uint64_t* pb = reinterpret_cast<uint64_t*>(w + L.off_pairs_b);
    void* kv = w + L.off_kv;
    const uint32_t nn = (uint32_t)n;
    const uint32_t wgs = (uint32_t)stride32_wgs(d->prop, n);
    int rc = launch(d, sizeof(K) == 4 ? "soa_pack_index_k32" : "soa_pack_index_k64", [&] {
        hipLaunchKernelGGL(adlhip::soa_pack_index_kernel<K>, dim3(wgs), dim3(adlhip::kSoaNT), 0, d->stream, (const K*)keys, pa, nn);
    });
    if (rc) return rc;
    // the stable pair sort of Pprims::radixSort(Buffer<uint2>) (Pprims.h:38) on {low key dword, index}
    rc = sort_entry<uint64_t>(d, ADLHIP_ELEM_KV32, pa, pb, kv, L.kv_bytes, n, std::min(sort_bits, 32), 32);
    if (rc) return rc;
    const uint64_t* sorted = pa;
    if constexpr (sizeof(K) == 8) {
        if (sort_bits > 32) {   // second 32-bit digit; the sort is stable, so equal high dwords keep the order of their low dwords
            rc = launch(d, "soa_repack_high", [&] {
                hipLaunchKernelGGL(adlhip::soa_repack_high_kernel, dim3(wgs), dim3(adlhip::kSoaNT), 0, d->stream, (const uint64_t*)keys,
                                   (const uint64_t*)pa, pb, nn);
            });
            if (rc) return rc;
            rc = sort_entry<uint64_t>(d, ADLHIP_ELEM_KV32, pb, pa, kv, L.kv_bytes, n, sort_bits - 32, 32);
            if (rc) return rc;
            sorted = pb;
        }
    }
    // u32 keys are the pairs' own low dwords and go straight to the caller's array; everything that is gathered lands in the
    // partner arrays first (the gather reads its source out of order) and is copied back (Pprims.cpp:298-301 copies back too)
    K* kout = sizeof(K) == 4 ? keys : tmp_keys;
    rc = launch(d, "soa_gather", [&] {
        hipLaunchKernelGGL((adlhip::soa_gather_kernel<K, V>), dim3(wgs), dim3(adlhip::kSoaNT), 0, d->stream, sorted, (const K*)keys, kout,
                           (const V*)vals, tmp_vals, nn);
    });
    if (rc) return rc;
    if (sizeof(K) == 8) HIPCHK(hipMemcpyAsync(keys, tmp_keys, n * sizeof(K), hipMemcpyDeviceToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(vals, tmp_vals, n * sizeof(V), hipMemcpyDeviceToDevice, d->stream));
    return ADLHIP_SUCCESS;
}

}  // namespace

// 256-thread and 1024-thread workgroups; blocks the calling thread until the result is back
static int run_lds_order_selftest(adlhip_device* d, int workgroups, uint32_t* mismatches)
{
    static uint32_t salt = 0;
    uint32_t* slot = d->d_fault + 8;
    HIPCHK(hipMemsetAsync(slot, 0, 4, d->stream));
    hipLaunchKernelGGL(adlhip::lds_order_selftest_kernel, dim3(workgroups), dim3(256), 0, d->stream, slot, ++salt);
    hipLaunchKernelGGL(adlhip::lds_order_selftest_kernel, dim3(workgroups), dim3(1024), 0, d->stream, slot, ++salt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(d->h_fault + 8, slot, 4, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    *mismatches = d->h_fault[8];
    return ADLHIP_SUCCESS;
}

// ---- what a handle owns for the sorts (handle.hip: create_common, release_handle) ------------------------------------------------
// The idle table's three areas at their idle values, then what the device answers.  A failure leaves what exists to sort_state_destroy.
int adlhip_internal::sort_state_create(adlhip_device* d)
{
    if (hipMalloc(&d->d_mid_hist, kMidHistWords * 4) != hipSuccess || hipMemsetAsync(d->d_mid_hist, 0, kMidHistWords * 4, d->stream) != hipSuccess)
        return fail("cannot allocate the mid-size sort's histogram area");
    // the large sort's handle-owned words (cursors, flags: 270 KB), zero between sorts -- allocated here rather than by a handle's
    // first large sort
    if (hipMalloc(&d->d_msd2, (kMsd2Words + kMsd2TicketWords) * 4) != hipSuccess ||
        hipMemsetAsync(d->d_msd2, 0, (kMsd2Words + kMsd2TicketWords) * 4, d->stream) != hipSuccess ||
        hipMemsetAsync(d->d_msd2 + kMsd2SampleAnd, 0xff, kMsd2SampleAndWords * 4, d->stream) != hipSuccess)   // all ones when idle
        return fail("cannot allocate the large sort's cursors");
    // (the larger dictionary of dict_big_kernels.hpp lies behind the small one: the kernels find it at d_dict + 1)
    static_assert(sizeof(adlhip::DictBlock) % 16 == 0, "the second block starts aligned");
    if (hipMalloc(&d->d_dict, (size_t)kDictWords * 4) != hipSuccess || hipMemsetAsync(d->d_dict, 0, (size_t)kDictWords * 4, d->stream) != hipSuccess)
        return fail("cannot allocate the counting sort's dictionary");
    if (trace_level())
        fprintf(stderr, "[adlhip] handle %p: d_fault %p h_fault %p d_mid_hist %p d_msd2 %p d_dict %p\n", (void*)d, (void*)d->d_fault,
                (void*)d->h_fault, (void*)d->d_mid_hist, (void*)d->d_msd2, (void*)d->d_dict);
    {   // self-test: are returning DS atomics lane-ordered on this device?  (enables "sort.rank" = 1)
        uint32_t mism = 1;
        d->lds_ordered = (run_lds_order_selftest(d, 64, &mism) == ADLHIP_SUCCESS && mism == 0) ? 1 : 0;
        d->rank_mode = d->lds_ordered;
    }
    {   // how many workgroups of the kernels that hold a grid-wide barrier (the safety nets of the mid-size and large sorts, 256
        // workgroups each) this device keeps resident at once: asked of the runtime for the two largest of them
        int a = 0, b = 0;
        using CS = adlhip::TileCfg<uint32_t, 8, 512, 32>;
        using CO = adlhip::TileCfg<uint32_t, 8, 512, 32>;
        const size_t lds_s = std::max<size_t>(sizeof(uint32_t) * 512 * 32 + (size_t)8 * 256 * 6 + 64, CS::LDS_BYTES);
        auto ks = adlhip::segment_sort_kernel<uint32_t, 512, 32, 8>;
        auto ko = adlhip::msd2_offsets_kernel<uint32_t, 512, 32>;   // (the net's look-back passes)
        // (the most LDS of all: the pairs' tile + the dictionary values of coop_dict_pair_sort)
        using CP = adlhip::TileCfg<uint64_t, 8, 512, 16>;
        auto kp = adlhip::msd2s_offsets_kernel<uint64_t, CP::TILE, 512, 16, 1, 4>;
        int c = 0;
        if (ensure_lds(ks, lds_s) == ADLHIP_SUCCESS && ensure_lds(ko, CO::LDS_BYTES) == ADLHIP_SUCCESS &&
            ensure_lds(kp, CP::LDS_BYTES) == ADLHIP_SUCCESS &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, reinterpret_cast<const void*>(ks), 512, lds_s) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, reinterpret_cast<const void*>(ko), 512, CO::LDS_BYTES) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&c, reinterpret_cast<const void*>(kp), 512, CP::LDS_BYTES) == hipSuccess)
            d->resident_wgs = std::min(std::min(a, b), c) * d->prop.multiProcessorCount;
        else
            d->resident_wgs = d->prop.multiProcessorCount;   // one per CU at least
        d->resident_wgs_device = d->resident_wgs;
        (void)hipGetLastError();
    }
    return ADLHIP_SUCCESS;
}

void adlhip_internal::sort_state_destroy(adlhip_device* d)
{
    if (d->d_mid_hist) hipFree(d->d_mid_hist);
    if (d->d_msd2) hipFree(d->d_msd2);
    if (d->d_dict) hipFree(d->d_dict);
}

// ---- the knobs that are words of that state, not fields of the handle (handle.hip: adlhip_set_param, adlhip_get_param) ------------
int adlhip_internal::sort_set_param(adlhip_device* d, const char* name, int value)
{
    if (strcmp(name, "debug.idle_poke")) return kNoSuchParam;
    // the idle checker's positive control: flips bit 0 of one handle-owned word, in stream order (a second poke undoes it)
    const int region = (int)((uint32_t)value >> 24);
    const uint32_t word = (uint32_t)value & 0xffffffu;
    if (region < 1 || region > kIdleRegions || word >= idle_region_words(region))
        return fail("debug.idle_poke: no word %u in region %d (region << 24 | word; regions 1 d_msd2, 2 d_mid_hist, 3 d_dict, 4 d_fault)", word, region);
    if (bind(d)) return ADLHIP_FAILURE;
    hipLaunchKernelGGL(idle_poke_kernel, dim3(1), dim3(1), 0, d->stream, idle_region_base(d, region) + word);
    HIPCHK(hipGetLastError());
    return ADLHIP_SUCCESS;
}

int adlhip_internal::sort_get_param(adlhip_device* d, const char* name, int* value)
{
    if (!strcmp(name, "stat.net_runs") || !strcmp(name, "stat.net_counting")) {
        // how often the large sort's safety net has run on this handle, and how often it sorted by counting (waits for the stream)
        uint32_t v[2] = {0u, 0u};
        HIPCHK(hipMemcpyAsync(v, net_stats(d), 8, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        *value = (int)v[name[9] == 'c' ? 1 : 0];
    } else if (!strcmp(name, "debug.idle_dirty") || !strcmp(name, "debug.idle_first")) {
        // handle-owned words that are not at their idle value (kIdleTable), and the first of them as region << 24 | word (0 = clean);
        // waits for the stream, changes nothing on the device
        uint32_t dirty = 0u, first = 0u;
        if (idle_check(d, &dirty, &first)) return ADLHIP_FAILURE;
        *value = (int)(name[11] == 'd' ? dirty : first);
    } else if (!strncmp(name, "debug.net_stamp", 15) && name[15] >= '0' && name[15] <= '9' && !name[16]) {
        // diagnostic: when workgroup 0 of the last net reached its k-th phase boundary, in 10-ns ticks (low 31 bits; tools/net_phases.py)
        uint32_t v = 0u;
        HIPCHK(hipMemcpyAsync(&v, net_stats(d) + 4 + (name[15] - '0'), 4, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        *value = (int)(v & 0x7fffffffu);
    } else {
        return kNoSuchParam;
    }
    return ADLHIP_SUCCESS;
}

// ================================================================================================
extern "C" {

int adlhip_selftest_lds_order(adlhip_device* d, int workgroups, uint32_t* mismatches)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!mismatches) return fail("null out pointer");
    if (workgroups < 1 || workgroups > 65536) return fail("selftest: workgroups must be in [1,65536]");
    return run_lds_order_selftest(d, workgroups, mismatches);
}

int adlhip_selftest_probe_positions(adlhip_device* d, size_t n, uint32_t* max_index, uint32_t* out_of_cell)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (!max_index || !out_of_cell) return fail("null out pointer");
    if (n < 16384 || n > kMaxElems) return fail("selftest: n must be in [16384, %zu]", (size_t)kMaxElems);
    // two words of the dictionary block's count[] serve as the result (free between sorts: a net that uses the dictionary clears
    // count[] before it counts, kIdleTable)
    uint32_t* res = d->d_dict->count;
    HIPCHK(hipMemsetAsync(res, 0, 8, d->stream));
    int rc = launch(d, "probe_positions_selftest", [&] {
        hipLaunchKernelGGL(adlhip::probe_positions_selftest_kernel, dim3(1), dim3(1024), 0, d->stream, (uint32_t)n, res);
    });
    if (rc) return rc;
    uint32_t h[2] = {0u, 0u};
    HIPCHK(hipMemcpyAsync(h, res, 8, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipMemsetAsync(res, 0, 8, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    *max_index = h[0];
    *out_of_cell = h[1];
    return ADLHIP_SUCCESS;
}

// ---- sort ---------------------------------------------------------------------------------------

int adlhip_radix_sort_scratch_bytes_for(adlhip_device* d, int elem_kind, size_t n, int sort_bits, int level, size_t* tmp_bytes,
                                        size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    if (elem_kind < ADLHIP_ELEM_U32 || elem_kind > ADLHIP_ELEM_SOA32) return fail("bad element kind %d", elem_kind);
    const int max_bits = elem_kind == ADLHIP_ELEM_U64 ? 64 : 32;
    if (sort_bits < 4 || sort_bits > max_bits || (sort_bits & 3)) return fail("sort_bits must be a multiple of 4 in [4,%d], got %d", max_bits, sort_bits);
    if (level < 0 || level > 2) return fail("level must be 0 (minimum), 1 (full speed) or 2 (lean), got %d", level);
    if (n > kMaxElems) return fail("n = %zu exceeds the supported maximum %zu", n, (size_t)kMaxElems);   // as the sorts themselves refuse it
    const size_t esz = (elem_kind == ADLHIP_ELEM_U32 || elem_kind == ADLHIP_ELEM_SOA32) ? 4 : 8;   // SoA: per array
    if (tmp_bytes) *tmp_bytes = align_up(n * esz, 256);
    if (work_bytes) *work_bytes = sort_work_bytes(d, elem_kind, n, sort_bits, level);
    return ADLHIP_SUCCESS;
}

int adlhip_radix_sort_scratch_bytes(adlhip_device* d, int elem_kind, size_t n, size_t* tmp_bytes, size_t* work_bytes)
{
    return adlhip_radix_sort_scratch_bytes_for(d, elem_kind, n, elem_kind == ADLHIP_ELEM_U64 ? 64 : 32, 1, tmp_bytes, work_bytes);
}

int adlhip_radix_sort_u32(adlhip_device* d, uint32_t* keys, uint32_t* tmp, void* work, size_t work_bytes, size_t n, int sort_bits)
{
    return sort_elements(d, ADLHIP_ELEM_U32, keys, tmp, work, work_bytes, n, sort_bits);
}

int adlhip_radix_sort_kv32(adlhip_device* d, void* pairs, void* tmp, void* work, size_t work_bytes, size_t n, int sort_bits)
{
    return sort_elements(d, ADLHIP_ELEM_KV32, pairs, tmp, work, work_bytes, n, sort_bits);
}

int adlhip_radix_sort_u64(adlhip_device* d, uint64_t* keys, uint64_t* tmp, void* work, size_t work_bytes, size_t n, int sort_bits)
{
    return sort_elements(d, ADLHIP_ELEM_U64, keys, tmp, work, work_bytes, n, sort_bits);
}

int adlhip_radix_sort_soa32(adlhip_device* d, uint32_t* keys, uint32_t* vals, uint32_t* tmp_keys, uint32_t* tmp_vals,
                            void* work, size_t work_bytes, size_t n, int sort_bits)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (check_sort_args(d, ADLHIP_ELEM_SOA32, keys, tmp_keys, work, work_bytes, n, sort_bits, 32)) return ADLHIP_FAILURE;
    if (n == 0) return ADLHIP_SUCCESS;
    if (!vals || !tmp_vals) return fail("null value buffer passed to radix sort");
    if ((reinterpret_cast<uintptr_t>(vals) | reinterpret_cast<uintptr_t>(tmp_vals)) & 15u)
        return fail("sort buffers must be 16-byte aligned");
    const LargePlan large = large_plan(d, 8, /*keys=*/false, n, sort_bits, 32, work_bytes);   // pairs: the stable form, full or lean
    if (large.form != kLargeNone) return msd2s_sort<uint64_t, false>(d, nullptr, nullptr, work, n, sort_bits, large, keys, vals);
    const std::vector<PassPlan> plan = plan_passes(sort_bits, d->digit_bits);
    return run_sort<SoaBuf>(d, SoaBuf{keys, vals}, SoaBuf{tmp_keys, tmp_vals}, work, work_bytes, n, plan);
}

int adlhip_radix_sort_soa_scratch_bytes(adlhip_device* d, int key_bytes, int value_bytes, size_t n, int sort_bits, size_t* tmp_keys_bytes,
                                        size_t* tmp_vals_bytes, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    if (soa_check_widths(key_bytes, value_bytes)) return ADLHIP_FAILURE;
    if (sort_bits < 4 || sort_bits > 8 * key_bytes || (sort_bits & 3)) return fail("sort_bits must be a multiple of 4 in [4,%d], got %d", 8 * key_bytes, sort_bits);
    if (n > kMaxElems) return fail("n = %zu exceeds the supported maximum %zu", n, (size_t)kMaxElems);   // as the sorts themselves refuse it
    if (tmp_keys_bytes) *tmp_keys_bytes = align_up(n * (size_t)key_bytes, 256);
    if (tmp_vals_bytes) *tmp_vals_bytes = align_up(n * (size_t)value_bytes, 256);
    if (work_bytes) {
        if (key_bytes == 4 && value_bytes == 4) *work_bytes = sort_work_bytes(d, ADLHIP_ELEM_SOA32, n, sort_bits, 1);
        else *work_bytes = soa_wide_layout(d, n).total;
    }
    return ADLHIP_SUCCESS;
}

int adlhip_radix_sort_soa(adlhip_device* d, void* keys, int key_bytes, void* vals, int value_bytes, void* tmp_keys, void* tmp_vals,
                          void* work, size_t work_bytes, size_t n, int sort_bits)
{
    if (soa_check_widths(key_bytes, value_bytes)) return ADLHIP_FAILURE;
    if (key_bytes == 4 && value_bytes == 4)
        return adlhip_radix_sort_soa32(d, (uint32_t*)keys, (uint32_t*)vals, (uint32_t*)tmp_keys, (uint32_t*)tmp_vals, work, work_bytes, n, sort_bits);
    if (bind(d)) return ADLHIP_FAILURE;
    if (sort_bits < 4 || sort_bits > 8 * key_bytes || (sort_bits & 3))   // Pprims.cpp:330
        return fail("sort_bits must be a multiple of 4 in [4,%d], got %d", 8 * key_bytes, sort_bits);
    if (n > kMaxElems || n >= (size_t(1) << 32)) return fail("n = %zu exceeds the supported maximum", n);
    if (n == 0) return ADLHIP_SUCCESS;
    if (!keys || !vals || !tmp_vals || !work || (key_bytes == 8 && !tmp_keys)) return fail("null buffer passed to radix sort");
    if ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(vals) | reinterpret_cast<uintptr_t>(tmp_keys) |
         reinterpret_cast<uintptr_t>(tmp_vals) | reinterpret_cast<uintptr_t>(work)) & 15u)
        return fail("sort buffers must be 16-byte aligned");
    const size_t need = soa_wide_layout(d, n).total;
    if (work_bytes < need) return fail("work buffer too small: %zu < %zu (adlhip_radix_sort_soa_scratch_bytes)", work_bytes, need);
#define ADLHIP_SOA(K_, V_) return soa_wide_sort<K_, V_>(d, (K_*)keys, (V_*)vals, (K_*)tmp_keys, (V_*)tmp_vals, work, n, sort_bits)
    if (key_bytes == 4) {
        if (value_bytes == 8) ADLHIP_SOA(uint32_t, uint64_t);
        ADLHIP_SOA(uint32_t, V16);
    }
    if (value_bytes == 4) ADLHIP_SOA(uint64_t, uint32_t);
    if (value_bytes == 8) ADLHIP_SOA(uint64_t, uint64_t);
    ADLHIP_SOA(uint64_t, V16);
#undef ADLHIP_SOA
}

int adlhip_segment_sort(adlhip_device* d, int elem_kind, void* data, const uint32_t* seg_start, size_t num_segments,
                        size_t max_segment, int low_bits)
{
    if (bind(d)) return ADLHIP_FAILURE;
    if (elem_kind != ADLHIP_ELEM_U32 && elem_kind != ADLHIP_ELEM_KV32) return fail("segment sort: u32 keys or {key, value} pairs only");
    if (low_bits < 1 || low_bits > 27) return fail("segment sort: low_bits must be in [1,27], got %d", low_bits);
    if (num_segments == 0) return ADLHIP_SUCCESS;
    if (!data || !seg_start) return fail("null buffer passed to segment sort");
    if (num_segments > 0x7fffffffull) return fail("segment sort: too many segments");
    if (!d->lds_ordered) return fail("segment sort needs lane-ordered DS atomics; the device self-test failed");
    if (elem_kind == ADLHIP_ELEM_U32)
        return segment_sort<uint32_t>(d, static_cast<const uint32_t*>(data), static_cast<uint32_t*>(data), seg_start, num_segments,
                                      max_segment, low_bits, nullptr);
    return segment_sort<uint64_t>(d, static_cast<const uint64_t*>(data), static_cast<uint64_t*>(data), seg_start, num_segments,
                                  max_segment, low_bits, nullptr);
}

// ---- scan ---------------------------------------------------------------------------------------

int adlhip_scan_scratch_bytes(adlhip_device* d, size_t n, size_t* work_bytes)
{
    if (!d) return fail("null device handle");
    // the sorts' limit.  (The kernels index with size_t, but one workgroup per tile passes HIP's 2^32 work-items per grid
    // dimension at 2^36 elements, and nothing beyond kMaxElems has ever run.)
    if (n > kMaxElems) return fail("scan: n = %zu exceeds the supported maximum %zu", n, (size_t)kMaxElems);
    const size_t blocks = (n + adlhip::kScanTile - 1) / adlhip::kScanTile;
    if (work_bytes) *work_bytes = align_up((blocks + 2) * 4, 256);
    return ADLHIP_SUCCESS;
}

int adlhip_exclusive_scan_u32(adlhip_device* d, uint32_t* dst, const uint32_t* src, void* work, size_t work_bytes,
                              size_t n, uint32_t* h_sum)
{
    if (bind(d)) return ADLHIP_FAILURE;
    size_t need = 0;
    if (adlhip_scan_scratch_bytes(d, n, &need)) return ADLHIP_FAILURE;   // n beyond the limit
    if (work_bytes < need || !work) return fail("scan work buffer too small: %zu < %zu", work_bytes, need);
    uint32_t* partial = reinterpret_cast<uint32_t*>(work);
    if (n == 0) {
        if (h_sum) *h_sum = 0;
        return ADLHIP_SUCCESS;
    }
    if (!dst || !src) return fail("null buffer passed to scan");
    const size_t blocks = (n + adlhip::kScanTile - 1) / adlhip::kScanTile;
    uint32_t* d_total = partial + blocks;   // grand total lives behind the block sums
    int rc;
    if (blocks <= 8) {
        rc = launch_scan_single(d, "scan_single", src, dst, n, d_total);
        if (rc) return rc;
    } else {
        rc = launch(d, "scan_reduce", [&] {
            hipLaunchKernelGGL(adlhip::scan_reduce_kernel, dim3((uint32_t)blocks), dim3(adlhip::kScanNT), 0, d->stream, src, partial, n);
        });
        if (rc) return rc;
        rc = launch_scan_single(d, "scan_partials", partial, partial, blocks, d_total);
        if (rc) return rc;
        rc = launch(d, "scan_apply", [&] {
            hipLaunchKernelGGL(adlhip::scan_apply_kernel, dim3((uint32_t)blocks), dim3(adlhip::kScanNT), 0, d->stream,
                               src, dst, (const uint32_t*)partial, n);
        });
        if (rc) return rc;
    }
    if (h_sum) HIPCHK(hipMemcpyAsync(h_sum, d_total, 4, hipMemcpyDeviceToHost, d->stream));   // Pprims.cpp:164-167
    return ADLHIP_SUCCESS;
}

// ---- MSB partition (multi-GPU send side) -----------------------------------------------------------

int adlhip_partition_msb_u32(adlhip_device* d, const uint32_t* in, uint32_t* out, uint32_t* counts, void* work,
                             size_t work_bytes, size_t n, int num_buckets)
{
    return partition_msb<uint32_t>(d, in, out, counts, work, work_bytes, n, num_buckets);
}

int adlhip_partition_msb_kv32(adlhip_device* d, const void* in, void* out, uint32_t* counts, void* work, size_t work_bytes,
                              size_t n, int num_buckets)
{
    return partition_msb<uint64_t>(d, static_cast<const uint64_t*>(in), static_cast<uint64_t*>(out), counts, work, work_bytes, n,
                                   num_buckets);
}

int adlhip_partition_top_byte_u32(adlhip_device* d, const uint32_t* in, uint32_t* out, uint32_t* totals256, void* work,
                                  size_t work_bytes, size_t n)
{
    return partition_top_byte_entry<uint32_t>(d, in, out, totals256, work, work_bytes, n);
}

int adlhip_partition_top_byte_kv32(adlhip_device* d, const void* in, void* out, uint32_t* totals256, void* work,
                                   size_t work_bytes, size_t n)
{
    return partition_top_byte_entry<uint64_t>(d, static_cast<const uint64_t*>(in), static_cast<uint64_t*>(out), totals256, work,
                                              work_bytes, n);
}

#ifdef ADLHIP_STAMPS
// Diagnostic build only: point the phase-stamp side buffer at caller-provided device memory ([tiles][16] u64).
int adlhip_debug_set_stamp_buffer(adlhip_device* d, void* dptr)
{
    if (bind(d)) return ADLHIP_FAILURE;
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(adlhip::g_stamp_buf), &dptr, sizeof(void*)));
    return ADLHIP_SUCCESS;
}
#endif

}  // extern "C"

#ifdef ADLHIP_SINGLE_TU
#include "handle.hip"
#include "primitives.hip"
#endif
