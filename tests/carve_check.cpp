// Host check of csrc/carve.hpp (tests/test_carve.py compiles and runs this; plain C++17, no HIP).
// A malloc-backed buffer stands in for byz::Buffer.  Checked: the first array at the base; every array 16-byte aligned, inside
// the buffer and clear of every other one, for mixed float / double / int32_t / int64_t arrays of 1, 3, 1025 and 0 elements in
// every order of the four types; total() = the end of the last array rounded up; a second commit into a buffer that is large
// enough allocates nothing; a negative count, a count whose byte size overflows and one array more than the table holds are
// refused before the buffer is touched.
// Exit status 0 when every property holds; the first violations are printed otherwise.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "carve.hpp"

namespace byz {
static char last_error[256] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
}
}  // namespace byz

namespace {

int failures = 0;

void fail(const char* what, long long a, long long b) {
    if (failures < 20) std::printf("FAIL %s: %lld %lld\n", what, a, b);
    ++failures;
}

struct HostBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    int allocations = 0, calls = 0;
    ~HostBuffer() { std::free(ptr); }
    int ensure(size_t need) {
        ++calls;
        if (need <= bytes) return BYZ_OK;
        std::free(ptr);
        ptr = std::aligned_alloc(256, (need + 255) / 256 * 256);     // (hipMalloc's alignment)
        bytes = need;
        ++allocations;
        return ptr ? BYZ_OK : BYZ_E_HIP;
    }
};

struct Span {
    uintptr_t begin, bytes;
};

// the arrays of one layout: type t of 0..3 = float, double, int32_t, int64_t
constexpr size_t kElem[4] = {sizeof(float), sizeof(double), sizeof(int32_t), sizeof(int64_t)};

struct Arrays {
    float* f[8];
    double* d[8];
    int32_t* i[8];
    int64_t* l[8];
};

void take(byz::Carve& c, Arrays& a, int type, int k, int64_t count) {
    if (type == 0) c.take(&a.f[k], count);
    if (type == 1) c.take(&a.d[k], count);
    if (type == 2) c.take(&a.i[k], count);
    if (type == 3) c.take(&a.l[k], count);
}
uintptr_t address(const Arrays& a, int type, int k) {
    const void* p = type == 0 ? (const void*)a.f[k] : type == 1 ? (const void*)a.d[k] : type == 2 ? (const void*)a.i[k] : (const void*)a.l[k];
    return reinterpret_cast<uintptr_t>(p);
}

// one layout: the four types in the order `perm`, every type with the counts rotated by `shift`; then written through
void check_layout(const int (&perm)[4], int shift) {
    const int64_t counts[4] = {1, 3, 1025, 0};
    byz::Carve c;
    Arrays a;
    std::memset(&a, 0, sizeof(a));
    int types[16], ks[16];
    int64_t ns[16];
    int n = 0;
    for (int k = 0; k < 4; ++k)
        for (int t = 0; t < 4; ++t) {
            types[n] = perm[t], ks[n] = k, ns[n] = counts[(k + t + shift) % 4];
            take(c, a, types[n], ks[n], ns[n]);
            ++n;
        }
    HostBuffer buf;
    if (c.commit(buf) != BYZ_OK) return fail("commit", 0, 0);
    const uintptr_t base = reinterpret_cast<uintptr_t>(buf.ptr);
    Span spans[16];
    for (int s = 0; s < n; ++s) {
        spans[s] = {address(a, types[s], ks[s]), static_cast<uintptr_t>(ns[s]) * kElem[types[s]]};
        if (spans[s].begin == 0) fail("an array was not bound", s, 0);
        if (spans[s].begin % 16 != 0) fail("an array is off a 16-byte boundary", s, (long long)(spans[s].begin - base));
        if (spans[s].begin < base || spans[s].begin + spans[s].bytes > base + c.total()) fail("an array leaves the buffer", s, 0);
        if (spans[s].begin - base != c.offset(s)) fail("offset() disagrees with the bound pointer", s, 0);
    }
    if (spans[0].begin != base) fail("the first array is not at the base", (long long)(spans[0].begin - base), 0);
    for (int s = 0; s < n; ++s)
        for (int r = 0; r < n; ++r) {
            if (r == s) continue;
            if (spans[r].begin == spans[s].begin) fail("two arrays share an address", r, s);     // (the empty ones included)
            if (spans[r].begin < spans[s].begin + spans[s].bytes && spans[s].begin < spans[r].begin + spans[r].bytes) fail("two arrays overlap", r, s);
        }
    const uintptr_t end = spans[n - 1].begin + std::max<uintptr_t>(spans[n - 1].bytes, 1) - base;
    if (c.total() != (end + 15) / 16 * 16) fail("total() is not the end of the last array rounded up", (long long)c.total(), (long long)end);
    if (c.slots() != n) fail("slots()", c.slots(), n);
    // every element written with its array's number, then read back: no store reached a neighbour
    for (int s = 0; s < n; ++s)
        for (int64_t e = 0; e < ns[s]; ++e) {
            if (types[s] == 0) a.f[ks[s]][e] = static_cast<float>(s);
            if (types[s] == 1) a.d[ks[s]][e] = s;
            if (types[s] == 2) a.i[ks[s]][e] = s;
            if (types[s] == 3) a.l[ks[s]][e] = s;
        }
    for (int s = 0; s < n; ++s)
        for (int64_t e = 0; e < ns[s]; ++e) {
            const double got = types[s] == 0 ? a.f[ks[s]][e] : types[s] == 1 ? a.d[ks[s]][e] : types[s] == 2 ? a.i[ks[s]][e] : (double)a.l[ks[s]][e];
            if (got != s) fail("an element was overwritten", s, e);
        }
}

// commit() must fail with BYZ_E_INVALID and a message, leave the buffer alone and bind nothing
void check_refused(const char* what, byz::Carve& c, float* const& sentinel_slot) {
    HostBuffer buf;
    byz::last_error[0] = 0;
    const int rc = c.commit(buf);
    if (rc != BYZ_E_INVALID) fail(what, rc, 0);
    if (byz::last_error[0] == 0) fail("a refusal without a message", 0, 0);
    if (buf.calls != 0) fail("a refused layout touched the buffer", buf.calls, 0);
    if (sentinel_slot != nullptr) fail("a refused layout bound a pointer", 0, 0);
}

}  // namespace

int main() {
    int perm[4] = {0, 1, 2, 3};
    int layouts = 0;
    do {
        for (int shift = 0; shift < 4; ++shift, ++layouts) check_layout(perm, shift);
    } while (std::next_permutation(perm, perm + 4));

    {   // a second commit into a buffer that is already large enough: the same pointers, no allocation
        HostBuffer buf;
        float* x = nullptr;
        int64_t* y = nullptr;
        byz::Carve first;
        first.take(&x, 1025);
        first.take(&y, 3);
        if (first.commit(buf) != BYZ_OK || buf.allocations != 1) fail("first commit", buf.allocations, 0);
        const void* base = buf.ptr;
        const float* x0 = x;
        byz::Carve second;
        second.take(&x, 3);
        second.take(&y, 1);
        if (second.commit(buf) != BYZ_OK) fail("second commit", 0, 0);
        if (buf.allocations != 1 || buf.ptr != base) fail("the second commit reallocated", buf.allocations, 0);
        if (x != x0 || reinterpret_cast<const char*>(y) != reinterpret_cast<const char*>(base) + 16) fail("the second layout", 0, 0);
    }
    {   // an empty layout is no error and asks for nothing
        HostBuffer buf;
        byz::Carve none;
        if (none.commit(buf) != BYZ_OK || none.total() != 0 || buf.allocations != 0) fail("the empty layout", (long long)none.total(), 0);
    }
    {
        float* first = nullptr;
        double* d = nullptr;
        byz::Carve negative;
        negative.take(&first, 4);
        negative.take(&d, -1);
        check_refused("a negative count was not refused", negative, first);
    }
    {
        float* first = nullptr;
        double* d = nullptr;
        int32_t* after = nullptr;
        byz::Carve huge;
        huge.take(&first, 4);
        huge.take(&d, INT64_MAX / 4);          // 2^61 doubles: 2^64 bytes
        huge.take(&after, 1);
        check_refused("an overflowing byte size was not refused", huge, first);
        byz::Carve sum;                        // each fits, the sum does not
        first = nullptr;
        int64_t* l[3] = {};
        sum.take(&first, 4);
        for (int k = 0; k < 3; ++k) sum.take(&l[k], INT64_MAX / 16);
        check_refused("an overflowing total was not refused", sum, first);
    }
    {
        float* slots[byz::Carve::kMaxSlots + 1] = {};
        byz::Carve full;
        for (int k = 0; k < byz::Carve::kMaxSlots; ++k) full.take(&slots[k], k);
        HostBuffer buf;
        if (full.commit(buf) != BYZ_OK || slots[byz::Carve::kMaxSlots - 1] == nullptr) fail("a full table was refused", 0, 0);
        for (int k = 0; k < byz::Carve::kMaxSlots; ++k) slots[k] = nullptr;
        full.take(&slots[byz::Carve::kMaxSlots], 1);
        check_refused("capacity + 1 was not refused", full, slots[0]);
    }

    if (failures != 0) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("carve ok: %d layouts of 16 arrays\n", layouts);
    return 0;
}
