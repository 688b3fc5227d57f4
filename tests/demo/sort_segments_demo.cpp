// sort_segments_demo -- Pprims::sortSegments / argsortSegments (every segment [offsets[s], offsets[s + 1]) of a key array sorted on its
// own, stably; signed, float and descending keys; ragged lengths with empty segments) checked against a comparison sort written here,
// one OK / FAIL line per case.
//   --host     run on an Adl TYPE_HOST device (the CPU path of src/TypedSort.cpp); default: the HIP device
//   --dump     also print, for the small cases, "DUMP <type> <order> <segments> <n> <global> : <offsets> ; <bits of the input, hex> |
//              <indexOut> | <keysOut bits, hex>" so that a caller can check them against a reference of its own
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
    const T* keys;
    bool descending;
    bool operator()(u32 i, u32 j) const { return descending ? Order<T>::less(keys[j], keys[i]) : Order<T>::less(keys[i], keys[j]); }
};

template <typename T, typename B>
void fillKeys(std::vector<T>& keys)
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
    B pool[37];   // few values: ties make the tie rule meaningful
    for (int k = 0; k < 37; ++k) pool[k] = (B)nextBits();
    for (int i = 0; i < n; ++i) {
        B b = pool[nextBits() % 37];
        if (i % 61 == 7) b = sizeof(B) == 4 ? (B)special32[(i / 61) % 16] : (B)special64[(i / 61) % 16];
        memcpy(&keys[i], &b, sizeof(B));
    }
}

struct Shape {
    std::vector<int> lens;
    int maxSegment;   // the bound handed to the library (0: unknown)
    bool globalIndex;
};

template <typename T, typename B>
void runCase(Device* d, Pprims& p, const char* name, const Shape& sh, bool descending, bool dump)
{
    const int S = (int)sh.lens.size();
    std::vector<u32> off((size_t)S + 1, 0u);
    for (int s = 0; s < S; ++s) off[s + 1] = off[s] + (u32)sh.lens[s];
    const int n = (int)off[S];
    std::vector<T> keys((size_t)n);
    fillKeys<T, B>(keys);
    std::vector<u32> want((size_t)n);
    std::vector<T> wantKeys((size_t)n);
    std::vector<u32> perm;
    for (int s = 0; s < S; ++s) {
        const u32 lo = off[s], len = off[s + 1] - lo;
        perm.resize(len);
        for (u32 i = 0; i < len; ++i) perm[i] = i;
        ByKey<T> cmp = {keys.data() + lo, descending};
        std::stable_sort(perm.begin(), perm.end(), cmp);
        for (u32 j = 0; j < len; ++j) {
            want[lo + j] = perm[j] + (sh.globalIndex ? lo : 0u);
            wantKeys[lo + j] = keys[lo + perm[j]];
        }
    }

    bool okIndex = true, okIntact = true, okKeys = true, okArgsort = true;
    std::vector<u32> got((size_t)n), gotArg((size_t)n);
    std::vector<T> gotKeys((size_t)n);
    {
        Buffer<T> kb(d, n);
        Buffer<u32> ob(d, S + 1);
        Buffer<T> ko(d, n);
        Buffer<u32> ib(d, n);
        Buffer<u32> ab(d, n);
        kb.write(keys.data(), n);
        ob.write(off.data(), S + 1);
        DeviceUtils::waitForCompletion(d);
        p.sortSegments(d, kb, ob, ko, ib, n, S, sh.maxSegment, descending, sh.globalIndex);
        p.argsortSegments(d, kb, ob, ab, n, S, sh.maxSegment, descending, sh.globalIndex);
        std::vector<T> after((size_t)n);
        ib.read(got.data(), n);
        ab.read(gotArg.data(), n);
        ko.read(gotKeys.data(), n);
        kb.read(after.data(), n);
        DeviceUtils::waitForCompletion(d);
        okIndex = memcmp(got.data(), want.data(), sizeof(u32) * (size_t)n) == 0;
        okArgsort = memcmp(gotArg.data(), want.data(), sizeof(u32) * (size_t)n) == 0;
        okKeys = memcmp(gotKeys.data(), wantKeys.data(), sizeof(T) * (size_t)n) == 0;   // bit for bit: NaN payloads, -0
        okIntact = memcmp(after.data(), keys.data(), sizeof(T) * (size_t)n) == 0;
    }
    const bool ok = okIndex && okArgsort && okIntact && okKeys && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] SortSegments.%s %s segments=%d n=%d max=%d global=%d%s%s%s%s\n", ok ? "OK" : "FAIL", name,
           descending ? "descending" : "ascending", S, n, sh.maxSegment, sh.globalIndex ? 1 : 0,
           okIndex ? "" : " (indices differ from std::stable_sort)", okArgsort ? "" : " (argsortSegments differs from std::stable_sort)",
           okIntact ? "" : " (sortSegments changed its input)", okKeys ? "" : " (keys differ from std::stable_sort)");
    if (dump && n <= 2000) {
        printf("DUMP %s %s %d %d %d :", name, descending ? "descending" : "ascending", S, n, sh.globalIndex ? 1 : 0);
        for (int s = 0; s <= S; ++s) printf(" %u", off[s]);
        printf(" ;");
        for (int i = 0; i < n; ++i) {
            B b;
            memcpy(&b, &keys[i], sizeof(B));
            printf(" %llx", (unsigned long long)b);
        }
        printf(" |");
        for (int j = 0; j < n; ++j) printf(" %u", got[j]);
        printf(" |");
        for (int j = 0; j < n; ++j) {
            B b;
            memcpy(&b, &gotKeys[j], sizeof(B));
            printf(" %llx", (unsigned long long)b);
        }
        printf("\n");
    }
}

Shape shape(const int* lens, int count, int maxSegment, bool globalIndex)
{
    Shape s;
    s.lens.assign(lens, lens + count);
    s.maxSegment = maxSegment;
    s.globalIndex = globalIndex;
    return s;
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
        // ragged lengths with empty segments first, last and in runs (the segment kernel, several classes in one call); a full tile's
        // segment beside short ones; one segment with no bound (the flat argsort itself); segments above the 4096 keys a workgroup
        // sorts (the flat path); positions in the whole array; many short segments
        static const int a[] = {0, 5, 0, 0, 1, 33, 2, 0, 100, 7, 0};
        static const int b[] = {300, 0, 17, 4096, 1};
        static const int c[] = {1000};
        static const int e[] = {5000, 0, 7, 4097};
        static const int f[] = {0, 0, 3, 0};
        int g[40];
        for (int i = 0; i < 40; ++i) g[i] = (i * 7) % 13;
        std::vector<Shape> shapes;
        shapes.push_back(shape(a, 11, 100, false));
        shapes.push_back(shape(b, 5, 4096, false));
        shapes.push_back(shape(c, 1, 0, false));
        shapes.push_back(shape(e, 4, 0, true));
        shapes.push_back(shape(f, 4, 3, true));
        shapes.push_back(shape(g, 40, 12, true));
        for (size_t s = 0; s < shapes.size(); ++s)
            for (int desc = 0; desc < 2; ++desc) {
                runCase<u32, u32>(d, p, "u32", shapes[s], desc != 0, dump);
                runCase<int, u32>(d, p, "i32", shapes[s], desc != 0, dump);
                runCase<float, u32>(d, p, "f32", shapes[s], desc != 0, dump);
                runCase<u64, u64>(d, p, "u64", shapes[s], desc != 0, dump);
                runCase<long long, u64>(d, p, "i64", shapes[s], desc != 0, dump);
                runCase<double, u64>(d, p, "f64", shapes[s], desc != 0, dump);
            }
    }
    DeviceUtils::deallocate(d);
    g_failed += adl_assert_failures();
    return g_failed ? 1 : 0;
}
