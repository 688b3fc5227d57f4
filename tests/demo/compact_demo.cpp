// compact_demo -- Pprims::compactFlagged / Pprims::compactIf (stream compaction: select and stable partition by flag bytes or by a
// comparison with a threshold) checked against a loop written here, one OK / FAIL line per case.
//   --host     run on an Adl TYPE_HOST device (the CPU path of src/TypedSort.cpp); default: the HIP device
//   --dump     also print, for the small cases,
//                "DUMP flagged <item type> <select|partition> <n> : <flag bytes, hex> | <item bits, hex> | <S> | <items out> | <index out>"
//                "DUMP if <key type> <value type or none> <cmp> <threshold bits, hex> <select|partition> <n> : <key bits> | <value bits> |
//                 <S> | <keys out> | <values out> | <index out>"
//              (outputs: the first S elements, all n of a partition) so that a caller can check them against a reference of its own
// Exit status: 0 when every case is OK.
#include <Adl/Adl.h>
#include <Tahoe/ParallelPrimitives/Pprims.h>

#include <cstdio>
#include <cstring>
#include <vector>

using namespace adl;
using namespace Tahoe;

namespace {

int g_failed = 0;

unsigned long long g_state = 0x9E3779B97F4A7C15ull;
unsigned long long nextBits()   // splitmix64
{
    unsigned long long z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// "a sorts before b", stated per type and independently of the library's key codec: integers by value; floats by sign, then by
// magnitude bits (IEEE-754 totalOrder: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN)
template <typename T> struct Order { static bool less(T a, T b) { return a < b; } };
template <typename F, typename B>
bool floatLess(F a, F b)
{
    B x, y;
    memcpy(&x, &a, sizeof(B));
    memcpy(&y, &b, sizeof(B));
    const B sign = (B)1 << (8 * sizeof(B) - 1);
    const bool na = (x & sign) != 0, nb = (y & sign) != 0;
    if (na != nb) return na;                 // negative before positive
    const B ma = x & ~sign, mb = y & ~sign;
    return na ? ma > mb : ma < mb;           // negatives: the larger magnitude first
}
template <> struct Order<float> { static bool less(float a, float b) { return floatLess<float, u32>(a, b); } };
template <> struct Order<double> { static bool less(double a, double b) { return floatLess<double, u64>(a, b); } };

const unsigned long long special64[] = {
    0x0000000000000000ull, 0x8000000000000000ull, 0x0000000000000001ull, 0x8000000000000001ull, 0x0010000000000000ull,
    0x8010000000000000ull, 0x7fefffffffffffffull, 0xffefffffffffffffull, 0x7ff0000000000000ull, 0xfff0000000000000ull,
    0x7ff8000000000001ull, 0xfff8000000000001ull, 0x7ff8000000000002ull, 0xfff4000000000000ull, 0x7fffffffffffffffull,
    0xffffffffffffffffull};
const unsigned special32[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x00800000u, 0x80800000u,
                              0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00001u, 0xffc00001u,
                              0x7fc00002u, 0xffa00000u, 0x7fffffffu, 0xffffffffu};

// random bit patterns with the special ones sprinkled in
template <typename T, typename B>
void fillBits(std::vector<T>& v)
{
    for (size_t i = 0; i < v.size(); ++i) {
        B b = (B)nextBits();
        if (i % 7 == 5) b = sizeof(B) == 4 ? (B)special32[(i / 7) % 16] : (B)special64[(i / 7) % 16];
        memcpy(&v[i], &b, sizeof(B));
    }
}

template <typename T, typename B>
void printBits(const T* p, int n)
{
    for (int i = 0; i < n; ++i) {
        B b;
        memcpy(&b, &p[i], sizeof(B));
        printf(" %llx", (unsigned long long)b);
    }
}

// the stable order of a compaction: the kept positions, then (partition) the others
int orderOf(const std::vector<unsigned char>& keep, bool partition, std::vector<u32>& order)
{
    order.clear();
    for (size_t i = 0; i < keep.size(); ++i)
        if (keep[i]) order.push_back((u32)i);
    const int kept = (int)order.size();
    if (partition)
        for (size_t i = 0; i < keep.size(); ++i)
            if (!keep[i]) order.push_back((u32)i);
    return kept;
}

// got[0 .. m) is src gathered through order, got[m .. n) still holds the fill pattern
template <typename T>
bool gathered(const std::vector<T>& got, const std::vector<T>& src, const std::vector<u32>& order)
{
    for (size_t j = 0; j < order.size(); ++j)
        if (memcmp(&got[j], &src[order[j]], sizeof(T)) != 0) return false;
    for (size_t j = order.size(); j < got.size(); ++j)
        for (size_t b = 0; b < sizeof(T); ++b)
            if (((const unsigned char*)&got[j])[b] != 0xA5) return false;
    return true;
}

template <typename T, typename B>
void runFlagged(Device* d, Pprims& p, const char* tname, int n, int pattern, bool partition, bool dump)
{
    std::vector<T> items((size_t)n), got((size_t)n), after((size_t)n);
    std::vector<unsigned char> flags((size_t)n), afterF((size_t)n);
    std::vector<u32> idx((size_t)n), order;
    fillBits<T, B>(items);
    for (int i = 0; i < n; ++i) {
        const unsigned r = (unsigned)(nextBits() % 100u);
        const bool on = pattern == 0 ? false : pattern == 1 ? true : pattern == 2 ? (i & 1) != 0 : pattern == 3 ? r < 50u : r < 3u;
        flags[i] = on ? (unsigned char)(1u << (i % 8)) : 0;   // any non-zero byte selects
    }
    const int want = orderOf(flags, partition, order);
    memset(got.data(), 0xA5, sizeof(T) * (size_t)n);
    memset(idx.data(), 0xA5, sizeof(u32) * (size_t)n);
    int kept = -1;
    {
        Buffer<T> ib(d, n), ob(d, n);
        Buffer<unsigned char> fb(d, n);
        Buffer<u32> xb(d, n);
        ib.write(items.data(), n);
        fb.write(flags.data(), n);
        ob.write(got.data(), n);
        xb.write(idx.data(), n);
        DeviceUtils::waitForCompletion(d);
        kept = p.compactFlagged(d, ib, fb, ob, &xb, n, partition);
        ob.read(got.data(), n);
        xb.read(idx.data(), n);
        ib.read(after.data(), n);
        fb.read(afterF.data(), n);
        DeviceUtils::waitForCompletion(d);
    }
    std::vector<u32> positions((size_t)n);
    for (int i = 0; i < n; ++i) positions[i] = (u32)i;
    const bool okCount = kept == want;
    const bool okOut = gathered(got, items, order) && gathered(idx, positions, order);
    const bool okIntact = memcmp(after.data(), items.data(), sizeof(T) * (size_t)n) == 0 && memcmp(afterF.data(), flags.data(), (size_t)n) == 0;
    const bool ok = okCount && okOut && okIntact && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] Compact.flagged.%s %s pattern=%d n=%d%s%s%s\n", ok ? "OK" : "FAIL", tname, partition ? "partition" : "select", pattern, n,
           okCount ? "" : " (the count differs from the loop)", okOut ? "" : " (the outputs differ from the loop)",
           okIntact ? "" : " (an input was changed)");
    if (dump && n <= 1000) {
        const int m = partition ? n : (kept < 0 ? 0 : kept);
        printf("DUMP flagged %s %s %d :", tname, partition ? "partition" : "select", n);
        printBits<unsigned char, unsigned char>(flags.data(), n);
        printf(" |");
        printBits<T, B>(items.data(), n);
        printf(" | %d |", kept);
        printBits<T, B>(got.data(), m);
        printf(" |");
        printBits<u32, u32>(idx.data(), m);
        printf("\n");
    }
}

template <typename K, typename KB, typename V, typename VB>
void runIf(Device* d, Pprims& p, const char* kname, const char* vname, int n, int cmp, int special, bool partition, bool dump)
{
    static const char* const cmpName[6] = {"lt", "le", "gt", "ge", "eq", "ne"};
    const bool valued = strcmp(vname, "none") != 0;
    std::vector<K> keys((size_t)n), gotK((size_t)n), afterK((size_t)n);
    std::vector<V> vals((size_t)n), gotV((size_t)n), afterV((size_t)n);
    std::vector<u32> idx((size_t)n), order;
    fillBits<K, KB>(keys);
    fillBits<V, VB>(vals);
    KB tb = sizeof(KB) == 4 ? (KB)special32[special < 0 ? 0 : special % 16] : (KB)special64[special < 0 ? 0 : special % 16];
    if (special < 0) memcpy(&tb, &keys[(size_t)n / 2], sizeof(KB));   // an element of the input
    K threshold;
    memcpy(&threshold, &tb, sizeof(KB));
    std::vector<unsigned char> keep((size_t)n);
    for (int i = 0; i < n; ++i) {
        const bool lt = Order<K>::less(keys[i], threshold), eq = memcmp(&keys[i], &threshold, sizeof(K)) == 0;
        keep[i] = (cmp == ADLHIP_CMP_LT ? lt : cmp == ADLHIP_CMP_LE ? lt || eq : cmp == ADLHIP_CMP_GT ? !lt && !eq :
                   cmp == ADLHIP_CMP_GE ? !lt : cmp == ADLHIP_CMP_EQ ? eq : !eq) ? 1 : 0;
    }
    const int want = orderOf(keep, partition, order);
    memset(gotK.data(), 0xA5, sizeof(K) * (size_t)n);
    memset(gotV.data(), 0xA5, sizeof(V) * (size_t)n);
    memset(idx.data(), 0xA5, sizeof(u32) * (size_t)n);
    int kept = -1;
    {
        Buffer<K> kb(d, n), ko(d, n);
        Buffer<V> vb(d, n), vo(d, n);
        Buffer<u32> xb(d, n);
        kb.write(keys.data(), n);
        vb.write(vals.data(), n);
        ko.write(gotK.data(), n);
        vo.write(gotV.data(), n);
        xb.write(idx.data(), n);
        DeviceUtils::waitForCompletion(d);
        if (valued) kept = p.compactIf<K, V>(d, kb, &vb, cmp, threshold, ko, &vo, &xb, n, partition);
        else kept = p.compactIf<K>(d, kb, cmp, threshold, ko, &xb, n, partition);
        ko.read(gotK.data(), n);
        vo.read(gotV.data(), n);
        xb.read(idx.data(), n);
        kb.read(afterK.data(), n);
        vb.read(afterV.data(), n);
        DeviceUtils::waitForCompletion(d);
    }
    std::vector<u32> positions((size_t)n);
    for (int i = 0; i < n; ++i) positions[i] = (u32)i;
    const bool okCount = kept == want;
    const bool okOut = gathered(gotK, keys, order) && gathered(idx, positions, order) &&
                       gathered(gotV, vals, valued ? order : std::vector<u32>());
    const bool okIntact = memcmp(afterK.data(), keys.data(), sizeof(K) * (size_t)n) == 0 && memcmp(afterV.data(), vals.data(), sizeof(V) * (size_t)n) == 0;
    const bool ok = okCount && okOut && okIntact && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] Compact.if.%s.%s %s threshold=%llx %s n=%d%s%s%s\n", ok ? "OK" : "FAIL", kname, vname, cmpName[cmp], (unsigned long long)tb,
           partition ? "partition" : "select", n, okCount ? "" : " (the count differs from the loop)",
           okOut ? "" : " (the outputs differ from the loop)", okIntact ? "" : " (an input was changed)");
    if (dump && n <= 1000) {
        const int m = partition ? n : (kept < 0 ? 0 : kept);
        printf("DUMP if %s %s %s %llx %s %d :", kname, vname, cmpName[cmp], (unsigned long long)tb, partition ? "partition" : "select", n);
        printBits<K, KB>(keys.data(), n);
        printf(" |");
        if (valued) printBits<V, VB>(vals.data(), n);
        printf(" | %d |", kept);
        printBits<K, KB>(gotK.data(), m);
        printf(" |");
        if (valued) printBits<V, VB>(gotV.data(), m);
        printf(" |");
        printBits<u32, u32>(idx.data(), m);
        printf("\n");
    }
}

}  // namespace

int main(int argc, char** argv)
{
    bool host = false, dump = false;
    for (int i = 1; i < argc; ++i) {
        host |= !strcmp(argv[i], "--host");
        dump |= !strcmp(argv[i], "--dump");
    }
    DeviceUtils::Config cfg;
    cfg.m_type = host ? DeviceUtils::Config::DEVICE_CPU : DeviceUtils::Config::DEVICE_GPU;
    Device* d = DeviceUtils::allocate(host ? TYPE_HOST : TYPE_CL, cfg);
    if (adl_assert_failures() || !d) {
        printf("[ FAIL ] cannot open the device\n");
        return 1;
    }
    {
        Pprims p;
        const int sizes[] = {1, 7, 1000, 100003};
        for (int s = 0; s < 4; ++s)
            for (int part = 0; part < 2; ++part) {
                const int n = sizes[s];
                for (int pattern = 0; pattern < 5; ++pattern) {
                    runFlagged<float, u32>(d, p, "f32", n, pattern, part != 0, dump);
                    runFlagged<long long, u64>(d, p, "i64", n, pattern, part != 0, dump);
                }
                for (int cmp = 0; cmp < 6; ++cmp) {
                    const int special = (cmp * 5 + s * 3 + part) % 16;
                    // every key type; both key widths with both value widths and without values
                    runIf<u32, u32, u32, u32>(d, p, "u32", "none", n, cmp, special, part != 0, dump);
                    runIf<int, u32, double, u64>(d, p, "i32", "f64", n, cmp, special, part != 0, dump);
                    runIf<float, u32, int, u32>(d, p, "f32", "i32", n, cmp, special, part != 0, dump);
                    runIf<float, u32, u32, u32>(d, p, "f32", "none", n, cmp, -1, part != 0, dump);
                    runIf<u64, u64, float, u32>(d, p, "u64", "f32", n, cmp, special, part != 0, dump);
                    runIf<long long, u64, u32, u32>(d, p, "i64", "none", n, cmp, special, part != 0, dump);
                    runIf<double, u64, long long, u64>(d, p, "f64", "i64", n, cmp, special, part != 0, dump);
                    runIf<double, u64, u32, u32>(d, p, "f64", "none", n, cmp, -1, part != 0, dump);
                }
            }
    }
    DeviceUtils::deallocate(d);
    g_failed += adl_assert_failures();
    return g_failed ? 1 : 0;
}
