// reduce_demo -- Pprims::reduceByKey (sum / min / max of the values of every distinct key, keys in sorted order) checked against a
// comparison sort and a loop written here, one OK / FAIL line per case.
//   --host     run on an Adl TYPE_HOST device (the CPU path of src/TypedSort.cpp); default: the HIP device
//   --dump     also print, for the small cases, "DUMP <key type> <value type> <op> <order> <n> : <key bits, hex> | <value bits, hex> |
//              <uniqueOut bits, hex> | <reducedOut bits, hex>" so that a caller can check them against a reference of its own
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

template <typename T> struct IsFloat { enum { value = 0 }; };
template <> struct IsFloat<float> { enum { value = 1 }; };
template <> struct IsFloat<double> { enum { value = 1 }; };

template <typename T>
struct Item {
    T key;
    int idx;
};
template <typename T>
struct ByKey {
    bool descending;
    bool operator()(const Item<T>& a, const Item<T>& b) const { return descending ? Order<T>::less(b.key, a.key) : Order<T>::less(a.key, b.key); }
};

const unsigned long long special64[] = {
    0x0000000000000000ull, 0x8000000000000000ull, 0x0000000000000001ull, 0x8000000000000001ull, 0x0010000000000000ull,
    0x8010000000000000ull, 0x7fefffffffffffffull, 0xffefffffffffffffull, 0x7ff0000000000000ull, 0xfff0000000000000ull,
    0x7ff8000000000001ull, 0xfff8000000000001ull, 0x7ff8000000000002ull, 0xfff4000000000000ull, 0x7fffffffffffffffull,
    0xffffffffffffffffull};
const unsigned special32[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x00800000u, 0x80800000u,
                              0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00001u, 0xffc00001u,
                              0x7fc00002u, 0xffa00000u, 0x7fffffffu, 0xffffffffu};

template <typename T, typename B>
void fillKeys(std::vector<T>& keys, int distinct)
{
    const int n = (int)keys.size();
    std::vector<B> pool((size_t)distinct);
    for (int k = 0; k < distinct; ++k) pool[k] = (B)nextBits();
    for (int i = 0; i < n; ++i) {
        B b = pool[nextBits() % (unsigned long long)distinct];
        if (i % 61 == 7) b = sizeof(B) == 4 ? (B)special32[(i / 61) % 16] : (B)special64[(i / 61) % 16];
        memcpy(&keys[i], &b, sizeof(B));
    }
}

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

template <typename K, typename KB, typename V, typename VB>
void runCase(Device* d, Pprims& p, const char* kname, const char* vname, int n, int distinct, int op, bool descending, bool dump)
{
    static const char* const opName[3] = {"sum", "min", "max"};
    std::vector<K> keys((size_t)n);
    std::vector<V> vals((size_t)n);
    fillKeys<K, KB>(keys, distinct);
    fillValues<V, VB>(vals, op);
    std::vector<Item<K> > sorted((size_t)n);
    for (int i = 0; i < n; ++i) {
        sorted[i].key = keys[i];
        sorted[i].idx = i;
    }
    ByKey<K> cmp = {descending};
    std::stable_sort(sorted.begin(), sorted.end(), cmp);
    std::vector<K> wantKeys;
    std::vector<V> wantRed;
    for (int j = 0; j < n; ++j) {
        if (j == 0 || memcmp(&sorted[j].key, &sorted[j - 1].key, sizeof(K)) != 0) {   // bit for bit: NaN payloads, -0
            wantKeys.push_back(sorted[j].key);
            wantRed.push_back(vals[sorted[j].idx]);
        } else {
            step<V, VB>(wantRed.back(), vals[sorted[j].idx], op);
        }
    }
    const int want = (int)wantKeys.size();

    const unsigned char mark = 0xA5;
    std::vector<K> gotKeys((size_t)n), afterK((size_t)n);
    std::vector<V> gotRed((size_t)n), afterV((size_t)n);
    memset(gotKeys.data(), mark, sizeof(K) * (size_t)n);
    memset(gotRed.data(), mark, sizeof(V) * (size_t)n);
    int got = -1;
    {
        Buffer<K> kb(d, n), ub(d, n);
        Buffer<V> vb(d, n), rb(d, n);
        kb.write(keys.data(), n);
        vb.write(vals.data(), n);
        ub.write(gotKeys.data(), n);
        rb.write(gotRed.data(), n);
        DeviceUtils::waitForCompletion(d);
        got = p.reduceByKey(d, kb, vb, ub, rb, n, op, descending);
        ub.read(gotKeys.data(), n);
        rb.read(gotRed.data(), n);
        kb.read(afterK.data(), n);
        vb.read(afterV.data(), n);
        DeviceUtils::waitForCompletion(d);
    }
    const bool okCount = got == want;
    bool okKeys = okCount, okRed = okCount, okTail = true;
    if (okCount) {
        okKeys = memcmp(gotKeys.data(), wantKeys.data(), sizeof(K) * (size_t)want) == 0;
        okRed = memcmp(gotRed.data(), wantRed.data(), sizeof(V) * (size_t)want) == 0;
        const unsigned char* kt = (const unsigned char*)(gotKeys.data() + want);
        const unsigned char* rt = (const unsigned char*)(gotRed.data() + want);
        for (size_t i = 0; i < sizeof(K) * (size_t)(n - want); ++i) okTail &= kt[i] == mark;
        for (size_t i = 0; i < sizeof(V) * (size_t)(n - want); ++i) okTail &= rt[i] == mark;
    }
    const bool okIntact = memcmp(afterK.data(), keys.data(), sizeof(K) * (size_t)n) == 0 && memcmp(afterV.data(), vals.data(), sizeof(V) * (size_t)n) == 0;
    const bool ok = okCount && okKeys && okRed && okTail && okIntact && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] ReduceByKey.%s.%s %s %s n=%d distinct=%d%s%s%s%s%s\n", ok ? "OK" : "FAIL", kname, vname, opName[op],
           descending ? "descending" : "ascending", n, want, okCount ? "" : " (the number of distinct keys differs)",
           okKeys ? "" : " (keys differ from std::stable_sort)", okRed ? "" : " (reduced values differ from the loop)",
           okTail ? "" : " (elements behind the last run were written)", okIntact ? "" : " (reduceByKey changed an input)");
    if (dump && n <= 1000) {
        printf("DUMP %s %s %s %s %d :", kname, vname, opName[op], descending ? "descending" : "ascending", n);
        printBits<K, KB>(keys.data(), n);
        printf(" |");
        printBits<V, VB>(vals.data(), n);
        printf(" |");
        printBits<K, KB>(gotKeys.data(), got < n ? (got < 0 ? 0 : got) : n);
        printf(" |");
        printBits<V, VB>(gotRed.data(), got < n ? (got < 0 ? 0 : got) : n);
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
        const int sizes[][2] = {{1, 1}, {1000, 37}, {1000, 1000}, {100003, 256}};   // {n, values the keys are drawn from}
        for (int s = 0; s < 4; ++s)
            for (int op = 0; op < 3; ++op)
                for (int desc = 0; desc < 2; ++desc) {
                    const int n = sizes[s][0], v = sizes[s][1];
                    // every key type and every value type once, both widths on both sides
                    runCase<u32, u32, float, u32>(d, p, "u32", "f32", n, v, op, desc != 0, dump);
                    runCase<int, u32, long long, u64>(d, p, "i32", "i64", n, v, op, desc != 0, dump);
                    runCase<float, u32, int, u32>(d, p, "f32", "i32", n, v, op, desc != 0, dump);
                    runCase<u64, u64, double, u64>(d, p, "u64", "f64", n, v, op, desc != 0, dump);
                    runCase<long long, u64, u32, u32>(d, p, "i64", "u32", n, v, op, desc != 0, dump);
                    runCase<double, u64, u64, u64>(d, p, "f64", "u64", n, v, op, desc != 0, dump);
                }
    }
    DeviceUtils::deallocate(d);
    g_failed += adl_assert_failures();
    return g_failed ? 1 : 0;
}
