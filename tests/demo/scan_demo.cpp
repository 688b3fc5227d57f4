// scan_demo -- Pprims::scanTyped / Pprims::scanByKey (inclusive and exclusive prefix sum / min / max, plain and within the runs of grouped
// keys) checked against a loop written here, one OK / FAIL line per case; every case runs out of place and in place (dst = src).
//   --host     run on an Adl TYPE_HOST device (the CPU path of src/TypedSort.cpp); default: the HIP device
//   --dump     also print, for the small cases, "DUMP <key type or none> <value type> <op> <inclusive|exclusive> <n> : <key bits, hex> |
//              <value bits, hex> | <dst bits, hex>" so that a caller can check them against a reference of its own
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

template <typename T> struct IsFloat { enum { value = 0 }; };
template <> struct IsFloat<float> { enum { value = 1 }; };
template <> struct IsFloat<double> { enum { value = 1 }; };

const unsigned long long special64[] = {
    0x0000000000000000ull, 0x8000000000000000ull, 0x0000000000000001ull, 0x8000000000000001ull, 0x0010000000000000ull,
    0x8010000000000000ull, 0x7fefffffffffffffull, 0xffefffffffffffffull, 0x7ff0000000000000ull, 0xfff0000000000000ull,
    0x7ff8000000000001ull, 0xfff8000000000001ull, 0x7ff8000000000002ull, 0xfff4000000000000ull, 0x7fffffffffffffffull,
    0xffffffffffffffffull};
const unsigned special32[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x00800000u, 0x80800000u,
                              0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00001u, 0xffc00001u,
                              0x7fc00002u, 0xffa00000u, 0x7fffffffu, 0xffffffffu};

// values on which the result does not depend on the order of the operations: any bits for integer sums (they wrap) and for min / max;
// small integers stored as floats for float sums
template <typename V, typename B>
void fillValues(std::vector<V>& vals, int op)
{
    const int n = (int)vals.size();
    for (int i = 0; i < n; ++i) {
        if (IsFloat<V>::value && op == ADLHIP_REDUCE_SUM) {
            vals[i] = (V)((int)(nextBits() % 17u) - 8);
            continue;
        }
        B b = (B)nextBits();
        if (i % 53 == 5) b = sizeof(B) == 4 ? (B)special32[(i / 53) % 16] : (B)special64[(i / 53) % 16];
        memcpy(&vals[i], &b, sizeof(B));
    }
}

template <typename V, typename B>
void step(V& acc, const V& v, int op)
{
    if (op == ADLHIP_REDUCE_SUM) {
        if (IsFloat<V>::value) {
            acc = (V)(acc + v);
        } else {
            B a, b;
            memcpy(&a, &acc, sizeof(B));
            memcpy(&b, &v, sizeof(B));
            a = (B)(a + b);
            memcpy(&acc, &a, sizeof(B));
        }
    } else if (op == ADLHIP_REDUCE_MIN ? Order<V>::less(v, acc) : Order<V>::less(acc, v)) {
        memcpy(&acc, &v, sizeof(V));
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


// the first / last pattern of V in ascending order, stated per type and independently of the library's codec
template <typename V> struct Extremes;
template <> struct Extremes<u32> { static u32 lo() { return 0u; } static u32 hi() { return 0xffffffffu; } };
template <> struct Extremes<int> { static u32 lo() { return 0x80000000u; } static u32 hi() { return 0x7fffffffu; } };
template <> struct Extremes<float> { static u32 lo() { return 0xffffffffu; } static u32 hi() { return 0x7fffffffu; } };   // -NaN / +NaN, all-ones payload
template <> struct Extremes<u64> { static u64 lo() { return 0ull; } static u64 hi() { return ~0ull; } };
template <> struct Extremes<long long> { static u64 lo() { return 1ull << 63; } static u64 hi() { return ~(1ull << 63); } };
template <> struct Extremes<double> { static u64 lo() { return ~0ull; } static u64 hi() { return ~(1ull << 63); } };

struct NoKey {};

// grouped keys: runs of 1 .. maxRun elements; the bit patterns come back (A A B A), adjacent runs differ
template <typename K, typename KB>
void fillRuns(std::vector<K>& keys, int maxRun)
{
    const int n = (int)keys.size();
    KB pool[5];
    for (int k = 0; k < 5; ++k) pool[k] = (KB)nextBits();
    pool[3] = sizeof(KB) == 4 ? (KB)special32[10] : (KB)special64[10];   // a NaN pattern
    int i = 0, pick = 0;
    while (i < n) {
        pick = (pick + 1 + (int)(nextBits() % 4u)) % 5;   // never the pool entry of the run before
        int len = 1 + (int)(nextBits() % (unsigned long long)maxRun);
        for (; len > 0 && i < n; --len, ++i) memcpy(&keys[i], &pool[pick], sizeof(KB));
    }
}

template <typename K, typename KB, typename V, typename VB>
void runCase(Device* d, Pprims& p, const char* kname, const char* vname, int n, int maxRun, int op, bool exclusive, bool dump)
{
    static const char* const opName[3] = {"sum", "min", "max"};
    const bool keyed = strcmp(kname, "none") != 0;
    std::vector<KB> keys((size_t)n);
    std::vector<V> vals((size_t)n), want((size_t)n);
    if (keyed) fillRuns<KB, KB>(keys, maxRun);
    fillValues<V, VB>(vals, op);
    V acc = V();
    for (int i = 0; i < n; ++i) {
        const bool head = i == 0 || (keyed && keys[i] != keys[i - 1]);
        if (exclusive) {
            if (head) {
                VB b = op == ADLHIP_REDUCE_SUM ? (VB)0 : op == ADLHIP_REDUCE_MIN ? (VB)Extremes<V>::hi() : (VB)Extremes<V>::lo();
                memcpy(&want[i], &b, sizeof(VB));
            } else {
                memcpy(&want[i], &acc, sizeof(V));
            }
        }
        if (head) memcpy(&acc, &vals[i], sizeof(V));
        else step<V, VB>(acc, vals[i], op);
        if (!exclusive) memcpy(&want[i], &acc, sizeof(V));
    }

    std::vector<V> got((size_t)n), inPlace((size_t)n), afterV((size_t)n);
    std::vector<KB> afterK((size_t)n);
    memset(got.data(), 0xA5, sizeof(V) * (size_t)n);
    {
        Buffer<K> kb(d, n);
        Buffer<V> vb(d, n), ob(d, n);
        if (keyed) kb.write((const K*)keys.data(), n);
        vb.write(vals.data(), n);
        ob.write(got.data(), n);
        DeviceUtils::waitForCompletion(d);
        if (keyed) p.scanByKey(d, kb, vb, ob, n, op, exclusive);
        else p.scanTyped(d, vb, ob, n, op, exclusive);
        ob.read(got.data(), n);
        vb.read(afterV.data(), n);
        if (keyed) kb.read((K*)afterK.data(), n);
        DeviceUtils::waitForCompletion(d);
        if (keyed) p.scanByKey(d, kb, vb, vb, n, op, exclusive);
        else p.scanTyped(d, vb, vb, n, op, exclusive);
        vb.read(inPlace.data(), n);
        DeviceUtils::waitForCompletion(d);
    }
    const bool okOut = memcmp(got.data(), want.data(), sizeof(V) * (size_t)n) == 0;
    const bool okIn = memcmp(inPlace.data(), want.data(), sizeof(V) * (size_t)n) == 0;
    const bool okIntact = memcmp(afterV.data(), vals.data(), sizeof(V) * (size_t)n) == 0 &&
                          (!keyed || memcmp(afterK.data(), keys.data(), sizeof(KB) * (size_t)n) == 0);
    const bool ok = okOut && okIn && okIntact && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] Scan.%s.%s %s %s n=%d%s%s%s\n", ok ? "OK" : "FAIL", kname, vname, opName[op], exclusive ? "exclusive" : "inclusive", n,
           okOut ? "" : " (dst differs from the loop)", okIn ? "" : " (the in-place result differs from the loop)",
           okIntact ? "" : " (the scan changed an input)");
    if (dump && n <= 1000) {
        printf("DUMP %s %s %s %s %d :", kname, vname, opName[op], exclusive ? "exclusive" : "inclusive", n);
        if (keyed) printBits<KB, KB>(keys.data(), n);
        printf(" |");
        printBits<V, VB>(vals.data(), n);
        printf(" |");
        printBits<V, VB>(got.data(), n);
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
        const int sizes[][2] = {{1, 1}, {1000, 9}, {1000, 1000}, {100003, 5000}};   // {n, the longest run of the keys}
        for (int s = 0; s < 4; ++s)
            for (int op = 0; op < 3; ++op)
                for (int excl = 0; excl < 2; ++excl) {
                    const int n = sizes[s][0], r = sizes[s][1];
                    // every value type plain and keyed, both key widths with both value widths
                    runCase<u32, u32, float, u32>(d, p, "none", "f32", n, r, op, excl != 0, dump);
                    runCase<u32, u32, long long, u64>(d, p, "none", "i64", n, r, op, excl != 0, dump);
                    runCase<u32, u32, u32, u32>(d, p, "none", "u32", n, r, op, excl != 0, dump);
                    runCase<u32, u32, double, u64>(d, p, "none", "f64", n, r, op, excl != 0, dump);
                    runCase<u32, u32, float, u32>(d, p, "u32", "f32", n, r, op, excl != 0, dump);
                    runCase<float, u32, long long, u64>(d, p, "f32", "i64", n, r, op, excl != 0, dump);
                    runCase<u64, u64, int, u32>(d, p, "u64", "i32", n, r, op, excl != 0, dump);
                    runCase<double, u64, double, u64>(d, p, "f64", "f64", n, r, op, excl != 0, dump);
                    runCase<long long, u64, u64, u64>(d, p, "i64", "u64", n, r, op, excl != 0, dump);
                }
    }
    DeviceUtils::deallocate(d);
    g_failed += adl_assert_failures();
    return g_failed ? 1 : 0;
}
