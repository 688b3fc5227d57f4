// histogram_demo -- Pprims::histogramRange / Pprims::binCount (bin counts by sorted edges, counts per integer value) checked against a
// loop written here, one OK / FAIL line per case.
//   --host     run on an Adl TYPE_HOST device (the CPU path of src/TypedSort.cpp); default: the HIP device
//   --dump     also print, for the small cases,
//                "DUMP range <key type> <include upper: 0|1> <n> <bins> : <key bits, hex> | <edge bits, hex> | <counts, decimal>"
//                "DUMP bincount <key type> <n> <bins> : <key bits, hex> | <counts, decimal>"
//              so that a caller can check them against a reference of its own
// Exit status: 0 when every case is OK.
#include <Adl/Adl.h>
#include <Tahoe/ParallelPrimitives/Pprims.h>

#include <algorithm>
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

template <typename T, typename B>
void runRange(Device* d, Pprims& p, const char* tname, int n, int bins, int edgeKind, bool upper, bool dump)
{
    std::vector<T> keys((size_t)n), edges((size_t)bins + 1), afterK((size_t)n), afterE((size_t)bins + 1);
    fillBits<T, B>(keys);
    g_state += 12345;
    fillBits<T, B>(edges);
    if (edgeKind == 1)   // repeated edges: every third one copies its neighbour
        for (int b = 1; b <= bins; ++b)
            if (b % 3 == 1) edges[b] = edges[b - 1];
    if (edgeKind == 2)   // all edges equal
        for (int b = 1; b <= bins; ++b) edges[b] = edges[0];
    std::sort(edges.begin(), edges.end(), Order<T>::less);
    for (int i = 0; i < n; i += 5) keys[i] = edges[(size_t)(nextBits() % (unsigned)(bins + 1))];   // keys that lie on edges
    if (n > 3) keys[3] = edges[(size_t)bins];

    // the loop: the key's bin is (the number of edges that do not sort behind it) - 1
    std::vector<u32> want((size_t)bins, 0u), got((size_t)bins + 4);
    int upperBin = bins - 1;
    for (int b = bins - 1; b >= 0; --b)
        if (Order<T>::less(edges[b], edges[(size_t)bins])) {
            upperBin = b;
            break;
        }
    for (int i = 0; i < n; ++i) {
        const int pos = (int)(std::upper_bound(edges.begin(), edges.end(), keys[i], Order<T>::less) - edges.begin());
        if (pos >= 1 && pos <= bins) ++want[pos - 1];
        else if (pos > bins && upper && memcmp(&keys[i], &edges[(size_t)bins], sizeof(T)) == 0) ++want[upperBin];
    }
    memset(got.data(), 0xA5, sizeof(u32) * got.size());
    {
        Buffer<T> kb(d, n), eb(d, bins + 1);
        Buffer<u32> cb(d, bins + 4);
        kb.write(keys.data(), n);
        eb.write(edges.data(), bins + 1);
        cb.write(got.data(), bins + 4);
        DeviceUtils::waitForCompletion(d);
        p.histogramRange(d, kb, eb, cb, n, bins, upper);
        cb.read(got.data(), bins + 4);
        kb.read(afterK.data(), n);
        eb.read(afterE.data(), bins + 1);
        DeviceUtils::waitForCompletion(d);
    }
    bool okOut = memcmp(got.data(), want.data(), sizeof(u32) * (size_t)bins) == 0;
    bool okGuard = true;
    for (int j = bins; j < bins + 4; ++j) okGuard &= got[j] == 0xA5A5A5A5u;
    const bool okIntact = memcmp(afterK.data(), keys.data(), sizeof(T) * (size_t)n) == 0 &&
                          memcmp(afterE.data(), edges.data(), sizeof(T) * ((size_t)bins + 1)) == 0;
    const bool ok = okOut && okGuard && okIntact && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] Histogram.range.%s bins=%d edges=%d upper=%d n=%d%s%s%s\n", ok ? "OK" : "FAIL", tname, bins, edgeKind, upper ? 1 : 0, n,
           okOut ? "" : " (the counts differ from the loop)", okGuard ? "" : " (written behind the counters)",
           okIntact ? "" : " (an input was changed)");
    if (dump && n <= 1000 && bins <= 64) {
        printf("DUMP range %s %d %d %d :", tname, upper ? 1 : 0, n, bins);
        printBits<T, B>(keys.data(), n);
        printf(" |");
        printBits<T, B>(edges.data(), bins + 1);
        printf(" |");
        for (int b = 0; b < bins; ++b) printf(" %u", got[b]);
        printf("\n");
    }
}

template <typename T, typename B>
void runBincount(Device* d, Pprims& p, const char* tname, int n, int bins, bool dump)
{
    std::vector<T> keys((size_t)n), afterK((size_t)n);
    for (int i = 0; i < n; ++i) {
        const unsigned long long r = nextBits();
        B b = (B)(r % (unsigned long long)(2 * (long long)bins));   // half of them out of range
        if (i % 11 == 3) b = (B)r;                                  // anything: negative, far above 2^32
        if (i % 13 == 5) b = (B)0 - (B)(1 + r % 5);                 // small negative numbers
        if (i % 17 == 7) b = (B)(bins - 1);
        if (i % 19 == 9) b = (B)bins;
        memcpy(&keys[i], &b, sizeof(B));
    }
    std::vector<u32> want((size_t)bins, 0u), got((size_t)bins + 4);
    for (int i = 0; i < n; ++i)
        if (!Order<T>::less(keys[i], (T)0) && Order<T>::less(keys[i], (T)bins)) ++want[(size_t)keys[i]];
    memset(got.data(), 0xA5, sizeof(u32) * got.size());
    {
        Buffer<T> kb(d, n);
        Buffer<u32> cb(d, bins + 4);
        kb.write(keys.data(), n);
        cb.write(got.data(), bins + 4);
        DeviceUtils::waitForCompletion(d);
        p.binCount(d, kb, cb, n, bins);
        cb.read(got.data(), bins + 4);
        kb.read(afterK.data(), n);
        DeviceUtils::waitForCompletion(d);
    }
    const bool okOut = memcmp(got.data(), want.data(), sizeof(u32) * (size_t)bins) == 0;
    bool okGuard = true;
    for (int j = bins; j < bins + 4; ++j) okGuard &= got[j] == 0xA5A5A5A5u;
    const bool okIntact = memcmp(afterK.data(), keys.data(), sizeof(T) * (size_t)n) == 0;
    const bool ok = okOut && okGuard && okIntact && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] Histogram.bincount.%s bins=%d n=%d%s%s%s\n", ok ? "OK" : "FAIL", tname, bins, n,
           okOut ? "" : " (the counts differ from the loop)", okGuard ? "" : " (written behind the counters)",
           okIntact ? "" : " (an input was changed)");
    if (dump && n <= 1000 && bins <= 1000) {
        printf("DUMP bincount %s %d %d :", tname, n, bins);
        printBits<T, B>(keys.data(), n);
        printf(" |");
        for (int b = 0; b < bins; ++b) printf(" %u", got[b]);
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
        const int rangeBins[] = {1, 5, 64, 1000};
        const int countBins[] = {1, 1000, 20000};   // 20000: above the LDS limit, the sorted path
        for (int s = 0; s < 4; ++s) {
            const int n = sizes[s];
            for (int b = 0; b < 4; ++b)
                for (int upper = 0; upper < 2; ++upper) {
                    const int bins = rangeBins[b], edgeKind = (s + b + upper) % 3;
                    runRange<u32, u32>(d, p, "u32", n, bins, edgeKind, upper != 0, dump);
                    runRange<int, u32>(d, p, "i32", n, bins, edgeKind, upper != 0, dump);
                    runRange<float, u32>(d, p, "f32", n, bins, edgeKind, upper != 0, dump);
                    runRange<u64, u64>(d, p, "u64", n, bins, edgeKind, upper != 0, dump);
                    runRange<long long, u64>(d, p, "i64", n, bins, edgeKind, upper != 0, dump);
                    runRange<double, u64>(d, p, "f64", n, bins, edgeKind, upper != 0, dump);
                }
            for (int b = 0; b < 3; ++b) {
                runBincount<u32, u32>(d, p, "u32", n, countBins[b], dump);
                runBincount<int, u32>(d, p, "i32", n, countBins[b], dump);
                runBincount<u64, u64>(d, p, "u64", n, countBins[b], dump);
                runBincount<long long, u64>(d, p, "i64", n, countBins[b], dump);
            }
        }
    }
    DeviceUtils::deallocate(d);
    g_failed += adl_assert_failures();
    return g_failed ? 1 : 0;
}
