// search_demo -- Pprims::searchSorted (the lower / upper bound of every needle in a sorted sequence of typed keys) checked against a
// counting loop written here, one OK / FAIL line per case.
//   --host     run on an Adl TYPE_HOST device (the CPU path of src/TypedSort.cpp); default: the HIP device
//   --dump     also print, for the small cases,
//                "DUMP search <key type> <asc|desc> <left|right> <m> <n> : <sorted bits, hex> | <needle bits> | <positions>"
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
struct Before {   // a goes in front of b in the asked order
    bool descending;
    bool operator()(const T& a, const T& b) const { return descending ? Order<T>::less(b, a) : Order<T>::less(a, b); }
};

const unsigned long long special64[] = {
    0x0000000000000000ull, 0x8000000000000000ull, 0x0000000000000001ull, 0x8000000000000001ull, 0x0010000000000000ull,
    0x8010000000000000ull, 0x7fefffffffffffffull, 0xffefffffffffffffull, 0x7ff0000000000000ull, 0xfff0000000000000ull,
    0x7ff8000000000001ull, 0xfff8000000000001ull, 0x7ff8000000000002ull, 0xfff4000000000000ull, 0x7fffffffffffffffull,
    0xffffffffffffffffull};
const unsigned special32[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x00800000u, 0x80800000u,
                              0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00001u, 0xffc00001u,
                              0x7fc00002u, 0xffa00000u, 0x7fffffffu, 0xffffffffu};

// pattern 0: random bit patterns with the special ones sprinkled in; 1: three special values only, so that long runs of ties meet;
// 2: one value
template <typename T, typename B>
void fillBits(std::vector<T>& v, int pattern)
{
    for (size_t i = 0; i < v.size(); ++i) {
        B b = (B)nextBits();
        const size_t s = pattern == 0 ? (i / 7) % 16 : pattern == 1 ? (size_t)(nextBits() % 3u) * 4u : 9u;
        if (pattern != 0 || i % 7 == 5) b = sizeof(B) == 4 ? (B)special32[s] : (B)special64[s];
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

template <typename K, typename KB>
void runSearch(Device* d, Pprims& p, const char* kname, int m, int n, int pattern, bool descending, bool right, bool dump)
{
    std::vector<K> s((size_t)m), x((size_t)n), afterS((size_t)m), afterX((size_t)n);
    std::vector<u32> got((size_t)n), want((size_t)n);
    fillBits<K, KB>(s, pattern);
    fillBits<K, KB>(x, pattern);
    for (int i = 0; i < n && m; i += 3) x[(size_t)i] = s[(size_t)(nextBits() % (unsigned long long)m)];   // needles that are in the sequence
    Before<K> before = {descending};
    std::stable_sort(s.begin(), s.end(), before);
    for (int i = 0; i < n; ++i) {   // counted, not searched: the elements in front of the needle (right: not behind it)
        u32 c = 0;
        for (int j = 0; j < m; ++j) c += (right ? !before(x[(size_t)i], s[(size_t)j]) : before(s[(size_t)j], x[(size_t)i])) ? 1u : 0u;
        want[(size_t)i] = c;
    }
    memset(got.data(), 0xA5, sizeof(u32) * (size_t)n);
    {
        Buffer<K> sb(d, m ? m : 1), xb(d, n);
        Buffer<u32> pb(d, n);
        if (m) sb.write(s.data(), m);
        xb.write(x.data(), n);
        pb.write(got.data(), n);
        DeviceUtils::waitForCompletion(d);
        p.searchSorted<K>(d, sb, xb, pb, m, n, descending, right);
        pb.read(got.data(), n);
        if (m) sb.read(afterS.data(), m);
        xb.read(afterX.data(), n);
        DeviceUtils::waitForCompletion(d);
    }
    const bool okOut = memcmp(got.data(), want.data(), sizeof(u32) * (size_t)n) == 0;
    const bool okIntact = memcmp(afterS.data(), s.data(), sizeof(K) * (size_t)m) == 0 && memcmp(afterX.data(), x.data(), sizeof(K) * (size_t)n) == 0;
    const bool ok = okOut && okIntact && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] Search.%s %s %s pattern=%d m=%d n=%d%s%s\n", ok ? "OK" : "FAIL", kname, descending ? "desc" : "asc", right ? "right" : "left",
           pattern, m, n, okOut ? "" : " (the positions differ from the count)", okIntact ? "" : " (an input was changed)");
    if (dump && m <= 1000 && n <= 1000) {
        printf("DUMP search %s %s %s %d %d :", kname, descending ? "desc" : "asc", right ? "right" : "left", m, n);
        printBits<K, KB>(s.data(), m);
        printf(" |");
        printBits<K, KB>(x.data(), n);
        printf(" |");
        printBits<u32, u32>(got.data(), n);
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
        const int sizes[][2] = {{0, 5}, {1, 1}, {2, 9}, {300, 700}, {4097, 2049}, {20011, 3001}};   // {m, n}
        for (int s = 0; s < 6; ++s)
            for (int desc = 0; desc < 2; ++desc)
                for (int right = 0; right < 2; ++right)
                    for (int pattern = 0; pattern < 3; ++pattern) {
                        const int m = sizes[s][0], n = sizes[s][1];
                        runSearch<u32, u32>(d, p, "u32", m, n, pattern, desc != 0, right != 0, dump);
                        runSearch<int, u32>(d, p, "i32", m, n, pattern, desc != 0, right != 0, dump);
                        runSearch<float, u32>(d, p, "f32", m, n, pattern, desc != 0, right != 0, dump);
                        runSearch<u64, u64>(d, p, "u64", m, n, pattern, desc != 0, right != 0, dump);
                        runSearch<long long, u64>(d, p, "i64", m, n, pattern, desc != 0, right != 0, dump);
                        runSearch<double, u64>(d, p, "f64", m, n, pattern, desc != 0, right != 0, dump);
                    }
    }
    DeviceUtils::deallocate(d);
    g_failed += adl_assert_failures();
    return g_failed ? 1 : 0;
}
