// setop_demo -- Pprims::setOp (intersection, union, difference and symmetric difference of two sorted sequences of typed keys with
// thrust's multiset semantics, values and positions along) checked against counting loops written here, one OK / FAIL line per case.
//   --host     run on an Adl TYPE_HOST device (the CPU path of src/TypedSort.cpp); default: the HIP device
//   --dump     also print, for the small cases,
//                "DUMP setop <op> <key type> <value type or none> <asc|desc> <na> <nb> : <a bits, hex> | <b bits> | <a's value bits> |
//                 <b's value bits> | <count> | <keys out> | <values out> | <index out>"
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

const char* const kOpName[4] = {"intersection", "union", "difference", "symmetric_difference"};

template <typename K, typename KB>
bool sameBits(const K& x, const K& y)
{
    return memcmp(&x, &y, sizeof(KB)) == 0;
}

template <typename K, typename KB, typename V, typename VB>
void runSetOp(Device* d, Pprims& p, int op, const char* kname, const char* vname, int na, int nb, int pattern, bool descending, bool dump)
{
    const bool valued = strcmp(vname, "none") != 0;
    const bool both = op == ADLHIP_SETOP_UNION || op == ADLHIP_SETOP_SYMMETRIC_DIFFERENCE;
    const int n = na + nb, cap = both ? n : na;
    std::vector<K> a((size_t)na), b((size_t)nb), gotK((size_t)cap), wantK, afterA((size_t)na), afterB((size_t)nb);
    std::vector<V> va((size_t)na), vb((size_t)nb), gotV((size_t)cap), wantV;
    std::vector<u32> idx((size_t)cap), wantI;
    fillBits<K, KB>(a, pattern);
    fillBits<K, KB>(b, pattern);
    fillBits<V, VB>(va, 0);
    fillBits<V, VB>(vb, 0);
    Before<K> before = {descending};
    std::stable_sort(a.begin(), a.end(), before);
    std::stable_sort(b.begin(), b.end(), before);
    // the expected result, by counting: the stable merge (a tie takes a), every element with its rank r in its own input's run and
    // the length of the same key's run in the other input
    for (int i = 0, j = 0; i < na || j < nb;) {
        const bool takeB = i >= na || (j < nb && before(b[j], a[i]));
        const K x = takeB ? b[j] : a[i];
        int r = 0, other = 0;
        if (takeB) {
            while (j - r - 1 >= 0 && sameBits<K, KB>(b[j - r - 1], x)) ++r;
            for (int t = 0; t < na; ++t) other += sameBits<K, KB>(a[t], x) ? 1 : 0;
        } else {
            while (i - r - 1 >= 0 && sameBits<K, KB>(a[i - r - 1], x)) ++r;
            for (int t = 0; t < nb; ++t) other += sameBits<K, KB>(b[t], x) ? 1 : 0;
        }
        bool keep;
        if (takeB) keep = both && r >= other;
        else keep = op == ADLHIP_SETOP_UNION ? true : (op == ADLHIP_SETOP_INTERSECTION ? r < other : r >= other);
        if (keep) {
            wantK.push_back(x);
            wantV.push_back(takeB ? vb[j] : va[i]);
            wantI.push_back(takeB ? (u32)(na + j) : (u32)i);
        }
        if (takeB) ++j;
        else ++i;
    }
    const int want = (int)wantK.size();
    memset(gotK.data(), 0xA5, sizeof(K) * (size_t)cap);
    memset(gotV.data(), 0xA5, sizeof(V) * (size_t)cap);
    memset(idx.data(), 0xA5, sizeof(u32) * (size_t)cap);
    int got = -1;
    {
        Buffer<K> ab(d, na ? na : 1), bb(d, nb ? nb : 1), ko(d, cap ? cap : 1);
        Buffer<V> vab(d, na ? na : 1), vbb(d, nb ? nb : 1), vo(d, cap ? cap : 1);
        Buffer<u32> xb(d, cap ? cap : 1);
        if (na) ab.write(a.data(), na);
        if (nb) bb.write(b.data(), nb);
        if (na) vab.write(va.data(), na);
        if (nb) vbb.write(vb.data(), nb);
        if (cap) ko.write(gotK.data(), cap);
        if (cap) vo.write(gotV.data(), cap);
        if (cap) xb.write(idx.data(), cap);
        DeviceUtils::waitForCompletion(d);
        if (valued) got = p.setOp<K, V>(d, op, ab, &vab, bb, &vbb, ko, &vo, &xb, na, nb, descending);
        else got = p.setOp<K, V>(d, op, ab, (const Buffer<V>*)0, bb, (const Buffer<V>*)0, ko, (Buffer<V>*)0, &xb, na, nb, descending);
        if (cap) ko.read(gotK.data(), cap);
        if (cap) vo.read(gotV.data(), cap);
        if (cap) xb.read(idx.data(), cap);
        if (na) ab.read(afterA.data(), na);
        if (nb) bb.read(afterB.data(), nb);
        DeviceUtils::waitForCompletion(d);
    }
    bool okOut = got == want;
    if (okOut) {
        okOut = memcmp(gotK.data(), wantK.data(), sizeof(K) * (size_t)want) == 0 && memcmp(idx.data(), wantI.data(), sizeof(u32) * (size_t)want) == 0;
        if (valued) okOut = okOut && memcmp(gotV.data(), wantV.data(), sizeof(V) * (size_t)want) == 0;
        // nothing at the count or beyond is written (and no value at all without values)
        for (size_t i = sizeof(K) * (size_t)want; i < sizeof(K) * (size_t)cap; ++i) okOut &= ((const unsigned char*)gotK.data())[i] == 0xA5;
        for (size_t i = sizeof(u32) * (size_t)want; i < sizeof(u32) * (size_t)cap; ++i) okOut &= ((const unsigned char*)idx.data())[i] == 0xA5;
        for (size_t i = valued ? sizeof(V) * (size_t)want : 0; i < sizeof(V) * (size_t)cap; ++i) okOut &= ((const unsigned char*)gotV.data())[i] == 0xA5;
    }
    const bool okIntact = memcmp(afterA.data(), a.data(), sizeof(K) * (size_t)na) == 0 && memcmp(afterB.data(), b.data(), sizeof(K) * (size_t)nb) == 0;
    const bool ok = okOut && okIntact && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] SetOp.%s.%s.%s %s pattern=%d na=%d nb=%d count=%d%s%s\n", ok ? "OK" : "FAIL", kOpName[op], kname, vname, descending ? "desc" : "asc",
           pattern, na, nb, want, okOut ? "" : " (the outputs differ from the loop)", okIntact ? "" : " (an input was changed)");
    if (dump && n <= 1000 && got >= 0 && got <= cap) {
        printf("DUMP setop %s %s %s %s %d %d :", kOpName[op], kname, vname, descending ? "desc" : "asc", na, nb);
        printBits<K, KB>(a.data(), na);
        printf(" |");
        printBits<K, KB>(b.data(), nb);
        printf(" |");
        if (valued) printBits<V, VB>(va.data(), na);
        printf(" |");
        if (valued) printBits<V, VB>(vb.data(), nb);
        printf(" | %d |", got);
        printBits<K, KB>(gotK.data(), got);
        printf(" |");
        if (valued) printBits<V, VB>(gotV.data(), got);
        printf(" |");
        printBits<u32, u32>(idx.data(), got);
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
        const int sizes[][2] = {{0, 5}, {5, 0}, {300, 700}, {2047, 1}, {5003, 4001}};
        for (int s = 0; s < 5; ++s)
            for (int op = 0; op < 4; ++op)
                for (int desc = 0; desc < 2; ++desc)
                    for (int pattern = 0; pattern < 2; ++pattern) {
                        const int na = sizes[s][0], nb = sizes[s][1];
                        // every key type; both key widths with both value widths and without values
                        runSetOp<u32, u32, u32, u32>(d, p, op, "u32", "none", na, nb, pattern, desc != 0, dump);
                        runSetOp<int, u32, double, u64>(d, p, op, "i32", "f64", na, nb, pattern, desc != 0, dump);
                        runSetOp<float, u32, int, u32>(d, p, op, "f32", "i32", na, nb, pattern, desc != 0, dump);
                        runSetOp<u64, u64, float, u32>(d, p, op, "u64", "f32", na, nb, pattern, desc != 0, dump);
                        runSetOp<long long, u64, u32, u32>(d, p, op, "i64", "none", na, nb, pattern, desc != 0, dump);
                        runSetOp<double, u64, long long, u64>(d, p, op, "f64", "i64", na, nb, pattern, desc != 0, dump);
                    }
    }
    DeviceUtils::deallocate(d);
    g_failed += adl_assert_failures();
    return g_failed ? 1 : 0;
}
