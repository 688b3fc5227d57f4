// unique_demo -- Pprims::unique (the distinct keys of signed, float and descending keys in sorted order, and their counts) checked
// against a comparison sort written here, one OK / FAIL line per case.
//   --host     run on an Adl TYPE_HOST device (the CPU path of src/TypedSort.cpp); default: the HIP device
//   --dump     also print, for the small cases, "DUMP <type> <order> <n> : <key bits, hex> | <uniqueOut bits, hex> | <countsOut>"
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

template <typename T>
struct ByKey {
    bool descending;
    bool operator()(const T& a, const T& b) const { return descending ? Order<T>::less(b, a) : Order<T>::less(a, b); }
};

template <typename T, typename B>
void fillKeys(std::vector<T>& keys, int distinct)
{
    const int n = (int)keys.size();
    static const unsigned long long special64[] = {
        0x0000000000000000ull, 0x8000000000000000ull, 0x0000000000000001ull, 0x8000000000000001ull, 0x0010000000000000ull,
        0x8010000000000000ull, 0x7fefffffffffffffull, 0xffefffffffffffffull, 0x7ff0000000000000ull, 0xfff0000000000000ull,
        0x7ff8000000000001ull, 0xfff8000000000001ull, 0x7ff8000000000002ull, 0xfff4000000000000ull, 0x7fffffffffffffffull,
        0xffffffffffffffffull};
    static const unsigned special32[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x00800000u, 0x80800000u,
                                         0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00001u, 0xffc00001u,
                                         0x7fc00002u, 0xffa00000u, 0x7fffffffu, 0xffffffffu};
    std::vector<B> pool((size_t)distinct);
    for (int k = 0; k < distinct; ++k) pool[k] = (B)nextBits();
    for (int i = 0; i < n; ++i) {
        B b = pool[nextBits() % (unsigned long long)distinct];
        if (i % 61 == 7) b = sizeof(B) == 4 ? (B)special32[(i / 61) % 16] : (B)special64[(i / 61) % 16];
        memcpy(&keys[i], &b, sizeof(B));
    }
}

template <typename T, typename B>
void runCase(Device* d, Pprims& p, const char* name, int n, int distinct, bool descending, bool dump)
{
    std::vector<T> keys((size_t)n);
    fillKeys<T, B>(keys, distinct);
    std::vector<T> sorted(keys);
    ByKey<T> cmp = {descending};
    std::stable_sort(sorted.begin(), sorted.end(), cmp);
    std::vector<T> wantKeys;
    std::vector<u32> wantCounts;
    for (int j = 0; j < n; ++j) {
        if (j == 0 || memcmp(&sorted[j], &sorted[j - 1], sizeof(T)) != 0) {   // bit for bit: NaN payloads, -0
            wantKeys.push_back(sorted[j]);
            wantCounts.push_back(0);
        }
        ++wantCounts.back();
    }
    const int want = (int)wantKeys.size();

    const unsigned char mark = 0xA5;
    std::vector<T> gotKeys((size_t)n), after((size_t)n);
    std::vector<u32> gotCounts((size_t)n);
    memset(gotKeys.data(), mark, sizeof(T) * (size_t)n);
    memset(gotCounts.data(), mark, sizeof(u32) * (size_t)n);
    int got = -1;
    {
        Buffer<T> kb(d, n);
        Buffer<T> ub(d, n);
        Buffer<u32> cb(d, n);
        kb.write(keys.data(), n);
        ub.write(gotKeys.data(), n);
        cb.write(gotCounts.data(), n);
        DeviceUtils::waitForCompletion(d);
        got = p.unique(d, kb, ub, cb, n, descending);
        ub.read(gotKeys.data(), n);
        cb.read(gotCounts.data(), n);
        kb.read(after.data(), n);
        DeviceUtils::waitForCompletion(d);
    }
    const bool okCount = got == want;
    bool okKeys = okCount, okCounts = okCount, okTail = true;
    if (okCount) {
        okKeys = memcmp(gotKeys.data(), wantKeys.data(), sizeof(T) * (size_t)want) == 0;
        okCounts = memcmp(gotCounts.data(), wantCounts.data(), sizeof(u32) * (size_t)want) == 0;
        const unsigned char* kt = (const unsigned char*)(gotKeys.data() + want);
        const unsigned char* ct = (const unsigned char*)(gotCounts.data() + want);
        for (size_t i = 0; i < sizeof(T) * (size_t)(n - want); ++i) okTail &= kt[i] == mark;
        for (size_t i = 0; i < sizeof(u32) * (size_t)(n - want); ++i) okTail &= ct[i] == mark;
    }
    const bool okIntact = memcmp(after.data(), keys.data(), sizeof(T) * (size_t)n) == 0;
    const bool ok = okCount && okKeys && okCounts && okTail && okIntact && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] Unique.%s %s n=%d distinct=%d%s%s%s%s%s\n", ok ? "OK" : "FAIL", name, descending ? "descending" : "ascending", n, want,
           okCount ? "" : " (the number of distinct keys differs)", okKeys ? "" : " (keys differ from std::stable_sort)",
           okCounts ? "" : " (counts differ)", okTail ? "" : " (elements behind the last run were written)",
           okIntact ? "" : " (unique changed its input)");
    if (dump && n <= 1000) {
        printf("DUMP %s %s %d :", name, descending ? "descending" : "ascending", n);
        for (int i = 0; i < n; ++i) {
            B b;
            memcpy(&b, &keys[i], sizeof(B));
            printf(" %llx", (unsigned long long)b);
        }
        printf(" |");
        for (int j = 0; j < got && j < n; ++j) {
            B b;
            memcpy(&b, &gotKeys[j], sizeof(B));
            printf(" %llx", (unsigned long long)b);
        }
        printf(" |");
        for (int j = 0; j < got && j < n; ++j) printf(" %u", gotCounts[j]);
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
        const int sizes[][2] = {{1, 1}, {1000, 37}, {1000, 1000}, {100003, 256}, {100003, 100003}};   // {n, values the keys are drawn from}
        for (int s = 0; s < 5; ++s)
            for (int desc = 0; desc < 2; ++desc) {
                const int n = sizes[s][0], v = sizes[s][1];
                runCase<u32, u32>(d, p, "u32", n, v, desc != 0, dump);
                runCase<int, u32>(d, p, "i32", n, v, desc != 0, dump);
                runCase<float, u32>(d, p, "f32", n, v, desc != 0, dump);
                runCase<u64, u64>(d, p, "u64", n, v, desc != 0, dump);
                runCase<long long, u64>(d, p, "i64", n, v, desc != 0, dump);
                runCase<double, u64>(d, p, "f64", n, v, desc != 0, dump);
            }
    }
    DeviceUtils::deallocate(d);
    g_failed += adl_assert_failures();
    return g_failed ? 1 : 0;
}
