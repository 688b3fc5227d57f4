// sort_rows_demo -- Pprims::sortRows / argsortRows (every row of a rows x cols matrix sorted on its own, stably; signed, float and
// descending keys) checked against a comparison sort written here, one OK / FAIL line per case.
//   --host     run on an Adl TYPE_HOST device (the CPU path of src/TypedSort.cpp); default: the HIP device
//   --dump     also print, for the small cases, "DUMP <type> <order> <rows> <cols> <stride> : <bits of the whole input, hex> |
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
void fillKeys(std::vector<T>& keys, bool fewValues)
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
    B pool[37];
    for (int k = 0; k < 37; ++k) pool[k] = (B)nextBits();
    for (int i = 0; i < n; ++i) {
        B b = fewValues ? pool[nextBits() % 37] : (B)nextBits();
        if (i % 61 == 7) b = sizeof(B) == 4 ? (B)special32[(i / 61) % 16] : (B)special64[(i / 61) % 16];
        memcpy(&keys[i], &b, sizeof(B));
    }
}

template <typename T, typename B>
void runCase(Device* d, Pprims& p, const char* name, int rows, int cols, int stride, bool descending, bool dump)
{
    const int n = (rows - 1) * stride + cols;   // the padding behind the last row does not exist
    std::vector<T> keys((size_t)n);
    fillKeys<T, B>(keys, /*fewValues=*/true);   // ties make the tie rule meaningful; the padding holds keys like any other
    const int nk = rows * cols;
    std::vector<u32> want((size_t)nk);
    std::vector<T> wantKeys((size_t)nk);
    std::vector<u32> perm((size_t)cols);
    for (int r = 0; r < rows; ++r) {
        for (int i = 0; i < cols; ++i) perm[i] = (u32)i;
        ByKey<T> cmp = {keys.data() + (size_t)r * stride, descending};
        std::stable_sort(perm.begin(), perm.end(), cmp);
        for (int j = 0; j < cols; ++j) {
            want[(size_t)r * cols + j] = perm[j];
            wantKeys[(size_t)r * cols + j] = keys[(size_t)r * stride + perm[j]];
        }
    }

    bool okIndex = true, okIntact = true, okKeys = true, okArgsort = true;
    std::vector<u32> got((size_t)nk), gotArg((size_t)nk);
    std::vector<T> gotKeys((size_t)nk);
    {
        Buffer<T> kb(d, n);
        Buffer<T> ko(d, nk);
        Buffer<u32> ib(d, nk);
        Buffer<u32> ab(d, nk);
        kb.write(keys.data(), n);
        DeviceUtils::waitForCompletion(d);
        p.sortRows(d, kb, ko, ib, rows, cols, descending, stride);
        p.argsortRows(d, kb, ab, rows, cols, descending, stride);
        std::vector<T> after((size_t)n);
        ib.read(got.data(), nk);
        ab.read(gotArg.data(), nk);
        ko.read(gotKeys.data(), nk);
        kb.read(after.data(), n);
        DeviceUtils::waitForCompletion(d);
        okIndex = memcmp(got.data(), want.data(), sizeof(u32) * (size_t)nk) == 0;
        okArgsort = memcmp(gotArg.data(), want.data(), sizeof(u32) * (size_t)nk) == 0;
        okKeys = memcmp(gotKeys.data(), wantKeys.data(), sizeof(T) * (size_t)nk) == 0;   // bit for bit: NaN payloads, -0
        okIntact = memcmp(after.data(), keys.data(), sizeof(T) * (size_t)n) == 0;
    }
    const bool ok = okIndex && okArgsort && okIntact && okKeys && adl_assert_failures() == 0;
    if (!ok) ++g_failed;
    printf("[ %s ] SortRows.%s %s rows=%d cols=%d stride=%d%s%s%s%s\n", ok ? "OK" : "FAIL", name, descending ? "descending" : "ascending", rows,
           cols, stride, okIndex ? "" : " (columns differ from std::stable_sort)", okArgsort ? "" : " (argsortRows differs from std::stable_sort)",
           okIntact ? "" : " (sortRows changed its input)", okKeys ? "" : " (keys differ from std::stable_sort)");
    if (dump && nk <= 2000) {
        printf("DUMP %s %s %d %d %d :", name, descending ? "descending" : "ascending", rows, cols, stride);
        for (int i = 0; i < n; ++i) {
            B b;
            memcpy(&b, &keys[i], sizeof(B));
            printf(" %llx", (unsigned long long)b);
        }
        printf(" |");
        for (int j = 0; j < nk; ++j) printf(" %u", got[j]);
        printf(" |");
        for (int j = 0; j < nk; ++j) {
            B b;
            memcpy(&b, &gotKeys[j], sizeof(B));
            printf(" %llx", (unsigned long long)b);
        }
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
        // {rows, cols, stride}: many short rows, rows that do not fill a power of two, a partial last tile, stride > cols, one row, and
        // cols above the 4096 items a workgroup sorts (the flat path), with and without padding
        const int sizes[][3] = {{40, 33, 33}, {3, 300, 305}, {130, 7, 8}, {1, 1000, 1000}, {5, 4096, 4099}, {3, 4097, 4097}, {2, 10001, 10004}};
        for (int s = 0; s < 7; ++s)
            for (int desc = 0; desc < 2; ++desc) {
                const int rows = sizes[s][0], cols = sizes[s][1], stride = sizes[s][2];
                runCase<u32, u32>(d, p, "u32", rows, cols, stride, desc != 0, dump);
                runCase<int, u32>(d, p, "i32", rows, cols, stride, desc != 0, dump);
                runCase<float, u32>(d, p, "f32", rows, cols, stride, desc != 0, dump);
                runCase<u64, u64>(d, p, "u64", rows, cols, stride, desc != 0, dump);
                runCase<long long, u64>(d, p, "i64", rows, cols, stride, desc != 0, dump);
                runCase<double, u64>(d, p, "f64", rows, cols, stride, desc != 0, dump);
            }
    }
    DeviceUtils::deallocate(d);
    g_failed += adl_assert_failures();
    return g_failed ? 1 : 0;
}
