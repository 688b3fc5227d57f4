// join_demo -- Pprims::joinSorted (inner, left, semi and anti join of two sorted sequences of typed keys, as pairs of positions) and
// Pprims::expandRuns (run-length decode) checked against loops written here, one OK / FAIL line per case.
//   --host     run on an Adl TYPE_HOST device (the CPU path of src/TypedSort.cpp); default: the HIP device
//   --dump     also print, for the small cases,
//                "DUMP join <kind> <key type> <asc|desc> <na> <nb> <cap> : <A bits, hex> | <B bits> | <T> | <index a> | <index b>"
//                "DUMP expand <value type> <runs> <cap> : <counts, hex> | <value bits> | <T> | <run> | <rank> | <values out>"
//              so that a caller can check them against a reference of its own
// Exit status: 0 when every case is OK.
#include <Adl/Adl.h>
#include <Tahoe/ParallelPrimitives/Pprims.h>
#include <adlhip.h>

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

// pattern 0: a few dozen random bit patterns and the special ones, so that keys of A meet equal keys of B in short runs; 1: three
// special values only, so that long runs meet long runs
template <typename T, typename B>
void fillBits(std::vector<T>& v, int pattern, const std::vector<B>& pool)
{
    for (size_t i = 0; i < v.size(); ++i) {
        B b = pool[(size_t)(nextBits() % pool.size())];
        const size_t s = pattern == 0 ? (size_t)(nextBits() % 16u) : (size_t)(nextBits() % 3u) * 4u;
        if (pattern != 0 || i % 5 == 3) b = sizeof(B) == 4 ? (B)special32[s] : (B)special64[s];
        memcpy(&v[i], &b, sizeof(B));
    }
}

template <typename T, typename B>
void printBits(const T* p, size_t n)
{
    for (size_t i = 0; i < n; ++i) {
        B b;
        memcpy(&b, &p[i], sizeof(B));
        printf(" %llx", (unsigned long long)b);
    }
}

const char* const kKinds[] = {"inner", "left", "semi", "anti"};

template <typename K, typename KB>
void runJoin(Device* d, Pprims& p, const char* kname, int kind, int na, int nb, int pattern, bool descending, int capMode, bool dump)
{
    std::vector<K> a((size_t)na), b((size_t)nb), afterA((size_t)na), afterB((size_t)nb);
    std::vector<KB> pool(40);
    for (size_t i = 0; i < pool.size(); ++i) pool[i] = (KB)nextBits();
    fillBits<K, KB>(a, pattern, pool);
    fillBits<K, KB>(b, pattern, pool);
    Before<K> before = {descending};
    std::stable_sort(a.begin(), a.end(), before);
    std::stable_sort(b.begin(), b.end(), before);
    // every pair (i, j) with equal bits, by a double loop; B is sorted, so the j of one i are consecutive and ascending
    std::vector<u32> wantA, wantB;
    for (int i = 0; i < na; ++i) {
        size_t m = 0;
        for (int j = 0; j < nb; ++j) {
            if (memcmp(&a[(size_t)i], &b[(size_t)j], sizeof(K)) != 0) continue;
            if (kind == ADLHIP_JOIN_INNER || kind == ADLHIP_JOIN_LEFT || (kind == ADLHIP_JOIN_SEMI && m == 0)) {
                wantA.push_back((u32)i);
                wantB.push_back((u32)j);
            }
            ++m;
        }
        if (m == 0 && (kind == ADLHIP_JOIN_LEFT || kind == ADLHIP_JOIN_ANTI)) {
            wantA.push_back((u32)i);
            wantB.push_back(ADLHIP_JOIN_NONE);
        }
    }
    const size_t total = wantA.size();
    // capMode 0: the counting call; 1: exactly T; 2: T + 7; 3: half of T
    const int cap = capMode == 0 ? 0 : capMode == 1 ? (int)total : capMode == 2 ? (int)total + 7 : (int)(total / 2);
    const size_t rows = std::min(total, (size_t)cap);
    std::vector<u32> gotA((size_t)cap), gotB((size_t)cap);
    if (cap) memset(gotA.data(), 0xA5, sizeof(u32) * (size_t)cap), memset(gotB.data(), 0xA5, sizeof(u32) * (size_t)cap);
    unsigned long long count = 0;
    {
        Buffer<K> ab(d, na ? na : 1), bb(d, nb ? nb : 1);
        Buffer<u32> ia(d, cap ? cap : 1), ib(d, cap ? cap : 1);
        if (na) ab.write(a.data(), na);
        if (nb) bb.write(b.data(), nb);
        if (cap) ia.write(gotA.data(), cap), ib.write(gotB.data(), cap);
        DeviceUtils::waitForCompletion(d);
        count = p.joinSorted<K>(d, kind, ab, bb, cap ? &ia : 0, cap && kind != ADLHIP_JOIN_SEMI ? &ib : 0, na, nb, cap, descending);
        if (cap) ia.read(gotA.data(), cap), ib.read(gotB.data(), cap);
        if (na) ab.read(afterA.data(), na);
        if (nb) bb.read(afterB.data(), nb);
        DeviceUtils::waitForCompletion(d);
    }
    bool okOut = count == (unsigned long long)total && memcmp(gotA.data(), wantA.data(), sizeof(u32) * rows) == 0;
    if (kind != ADLHIP_JOIN_SEMI) okOut = okOut && memcmp(gotB.data(), wantB.data(), sizeof(u32) * rows) == 0;
    for (size_t o = rows; o < (size_t)cap; ++o) okOut = okOut && gotA[o] == 0xA5A5A5A5u && gotB[o] == 0xA5A5A5A5u;   // nothing behind the rows
    for (size_t o = 0; o < rows && kind == ADLHIP_JOIN_SEMI; ++o) okOut = okOut && gotB[o] == 0xA5A5A5A5u;          // nor in an output not given
    const bool okIntact = memcmp(afterA.data(), a.data(), sizeof(K) * (size_t)na) == 0 && memcmp(afterB.data(), b.data(), sizeof(K) * (size_t)nb) == 0;
    const bool ok = okOut && okIntact && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] Join.%s %s %s pattern=%d na=%d nb=%d cap=%d rows=%llu%s%s\n", ok ? "OK" : "FAIL", kKinds[kind], kname, descending ? "desc" : "asc",
           pattern, na, nb, cap, count, okOut ? "" : " (the rows differ from the double loop)", okIntact ? "" : " (an input was changed)");
    if (dump && na + nb <= 600) {
        printf("DUMP join %s %s %s %d %d %d :", kKinds[kind], kname, descending ? "desc" : "asc", na, nb, cap);
        printBits<K, KB>(a.data(), (size_t)na);
        printf(" |");
        printBits<K, KB>(b.data(), (size_t)nb);
        printf(" | %llu |", count);
        printBits<u32, u32>(gotA.data(), rows);
        printf(" |");
        if (kind != ADLHIP_JOIN_SEMI) printBits<u32, u32>(gotB.data(), rows);
        printf("\n");
    }
}

template <typename V, typename VB>
void runExpand(Device* d, Pprims& p, const char* vname, int runs, int pattern, int capMode, bool dump)
{
    std::vector<u32> counts((size_t)runs);
    std::vector<V> vals((size_t)runs);
    for (int i = 0; i < runs; ++i) {
        const unsigned r = (unsigned)(nextBits() % 100u);
        // pattern 0: mostly short runs, a third of them empty; 1: stretches of empty runs and a few long ones
        counts[(size_t)i] = pattern == 0 ? (r < 33 ? 0u : r % 5u) : ((i / 50) % 2 ? 0u : (r < 4 ? 700u + r : r % 2u));
        const VB b = (VB)nextBits();
        memcpy(&vals[(size_t)i], &b, sizeof(VB));
    }
    std::vector<u32> wantRun, wantRank;
    std::vector<V> wantVals;
    for (int i = 0; i < runs; ++i)
        for (u32 r = 0; r < counts[(size_t)i]; ++r) {
            wantRun.push_back((u32)i);
            wantRank.push_back(r);
            wantVals.push_back(vals[(size_t)i]);
        }
    const size_t total = wantRun.size();
    const int cap = capMode == 0 ? 0 : capMode == 1 ? (int)total : capMode == 2 ? (int)total + 7 : (int)(total / 2);
    const size_t rows = std::min(total, (size_t)cap);
    std::vector<u32> gotRun((size_t)cap), gotRank((size_t)cap);
    std::vector<V> gotVals((size_t)cap);
    if (cap) {
        memset(gotRun.data(), 0xA5, sizeof(u32) * (size_t)cap);
        memset(gotRank.data(), 0xA5, sizeof(u32) * (size_t)cap);
        memset(gotVals.data(), 0xA5, sizeof(V) * (size_t)cap);
    }
    unsigned long long count = 0;
    {
        Buffer<u32> cb(d, runs ? runs : 1), rb(d, cap ? cap : 1), kb(d, cap ? cap : 1);
        Buffer<V> vb(d, runs ? runs : 1), ob(d, cap ? cap : 1);
        if (runs) cb.write(counts.data(), runs), vb.write(vals.data(), runs);
        if (cap) rb.write(gotRun.data(), cap), kb.write(gotRank.data(), cap), ob.write(gotVals.data(), cap);
        DeviceUtils::waitForCompletion(d);
        count = p.expandRuns<V>(d, cb, &vb, cap ? &rb : 0, cap ? &kb : 0, cap ? &ob : 0, runs, cap);
        if (cap) rb.read(gotRun.data(), cap), kb.read(gotRank.data(), cap), ob.read(gotVals.data(), cap);
        DeviceUtils::waitForCompletion(d);
    }
    bool ok = count == (unsigned long long)total && memcmp(gotRun.data(), wantRun.data(), sizeof(u32) * rows) == 0 &&
              memcmp(gotRank.data(), wantRank.data(), sizeof(u32) * rows) == 0 && memcmp(gotVals.data(), wantVals.data(), sizeof(V) * rows) == 0;
    for (size_t o = rows; o < (size_t)cap; ++o) ok = ok && gotRun[o] == 0xA5A5A5A5u && gotRank[o] == 0xA5A5A5A5u;
    ok = ok && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] Expand.%s pattern=%d runs=%d cap=%d rows=%llu\n", ok ? "OK" : "FAIL", vname, pattern, runs, cap, count);
    if (dump && runs <= 600 && total <= 3000) {
        printf("DUMP expand %s %d %d :", vname, runs, cap);
        printBits<u32, u32>(counts.data(), (size_t)runs);
        printf(" |");
        printBits<V, VB>(vals.data(), (size_t)runs);
        printf(" | %llu |", count);
        printBits<u32, u32>(gotRun.data(), rows);
        printf(" |");
        printBits<u32, u32>(gotRank.data(), rows);
        printf(" |");
        printBits<V, VB>(gotVals.data(), rows);
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
        const int sizes[][2] = {{1, 0}, {7, 9}, {300, 200}, {2049, 700}, {1500, 4100}};   // {na, nb}
        for (int s = 0; s < 5; ++s)
            for (int kind = 0; kind < 4; ++kind)
                for (int desc = 0; desc < 2; ++desc)
                    for (int pattern = 0; pattern < 2; ++pattern) {
                        const int na = sizes[s][0], nb = sizes[s][1], capMode = (s + kind + desc + pattern) % 4;
                        if (pattern == 1 && (long long)na * nb > 2000000) continue;   // (three keys only: a third of na x nb rows)
                        runJoin<u32, u32>(d, p, "u32", kind, na, nb, pattern, desc != 0, capMode, dump);
                        runJoin<int, u32>(d, p, "i32", kind, na, nb, pattern, desc != 0, (capMode + 1) % 4, dump);
                        runJoin<float, u32>(d, p, "f32", kind, na, nb, pattern, desc != 0, (capMode + 2) % 4, dump);
                        runJoin<u64, u64>(d, p, "u64", kind, na, nb, pattern, desc != 0, (capMode + 3) % 4, dump);
                        runJoin<long long, u64>(d, p, "i64", kind, na, nb, pattern, desc != 0, capMode, dump);
                        runJoin<double, u64>(d, p, "f64", kind, na, nb, pattern, desc != 0, (capMode + 1) % 4, dump);
                    }
        const int runs[] = {1, 9, 300, 2049, 5000};
        for (int s = 0; s < 5; ++s)
            for (int pattern = 0; pattern < 2; ++pattern)
                for (int capMode = 0; capMode < 4; ++capMode) {
                    runExpand<u32, u32>(d, p, "u32", runs[s], pattern, capMode, dump);
                    runExpand<double, u64>(d, p, "f64", runs[s], pattern, capMode, dump);
                }
    }
    DeviceUtils::deallocate(d);
    g_failed += adl_assert_failures();
    return g_failed ? 1 : 0;
}
