// Host check of csrc/order_keys.hpp (tests/test_order_keys.py compiles and runs this; plain C++17, no HIP).
// Inputs: every float whose low 16 bits are 0x0000, 0x0001 or 0xffff -- all exponents, both signs, denormals, infinities,
// quiet and signalling NaNs -- and for the fp64 overload the same values widened plus fp64's own edge values.
// Exit status 0 when every property holds; the first violations are printed otherwise.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "order_keys.hpp"

namespace {

int failures = 0;

void fail(const char* what, uint64_t a, uint64_t b) {
    if (failures < 20) std::printf("FAIL %s: %016llx %016llx\n", what, (unsigned long long)a, (unsigned long long)b);
    ++failures;
}

uint32_t bits_of(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }
float float_of(uint32_t b) { float x; std::memcpy(&x, &b, 4); return x; }
uint64_t bits_of(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }
double double_of(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }

// IEEE `<`, except that -0.0 counts as below +0.0 when strict_zero
template <typename T>
bool below(T a, T b, bool strict_zero) {
    if (a < b) return true;
    return strict_zero && a == T(0) && b == T(0) && std::signbit(a) && !std::signbit(b);
}

// keys[i] belongs to values[i], no NaN among them.  With strict_zero (the plain map): keys are distinct and ordered like the
// values, -0.0 strictly below +0.0.  Without (the total map): equal values share a key, otherwise ordered like the values.
// The chain over the key-sorted sequence proves it for every pair (`<` is transitive away from NaN); a strided subset is
// checked pair by pair as well.
template <typename T, typename K>
void check_order(const char* what, const std::vector<T>& values, const std::vector<K>& keys, bool strict_zero) {
    std::vector<size_t> order(values.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return keys[a] < keys[b]; });
    for (size_t i = 1; i < order.size(); ++i) {
        const T a = values[order[i - 1]], b = values[order[i]];
        const K ka = keys[order[i - 1]], kb = keys[order[i]];
        const bool ok = ka < kb ? below(a, b, strict_zero) : (!strict_zero && a == b);
        if (!ok) fail(what, bits_of(a), bits_of(b));
    }
    const size_t stride = values.size() / 1500 + 1;
    for (size_t i = 0; i < values.size(); i += stride)
        for (size_t j = 0; j < values.size(); j += stride) {
            const T a = values[i], b = values[j];
            if (below(a, b, strict_zero) != (keys[i] < keys[j])) fail(what, bits_of(a), bits_of(b));
            if (!strict_zero && (a == b) != (keys[i] == keys[j])) fail(what, bits_of(a), bits_of(b));
        }
}

}  // namespace

int main() {
    using namespace byz;
    std::vector<float> inputs;
    for (uint32_t hi = 0; hi < 0x10000u; ++hi)
        for (uint32_t lo : {0x0000u, 0x0001u, 0xffffu}) inputs.push_back(float_of((hi << 16) | lo));

    const uint32_t pos_inf_key = ordered_bits(INFINITY);
    if (ordered_bits_total(INFINITY) != pos_inf_key || !(pos_inf_key < 0xffffffffu)) fail("+inf's key", pos_inf_key, 0);
    if (ordered_bits_total(-0.0f) != ordered_bits_total(0.0f)) fail("total: the zeros share a key", 0, 0);
    if (!(ordered_bits(-0.0f) < ordered_bits(0.0f))) fail("plain: -0.0 strictly below +0.0", 0, 0);

    std::vector<float> numbers;                    // the inputs that are not NaN
    std::vector<uint32_t> plain_keys, total_keys;
    for (const float x : inputs) {
        const uint32_t b = bits_of(x);
        const uint32_t key = ordered_bits(x);
        if (bits_of(from_ordered_bits(key)) != b) fail("round trip", b, key);
        const uint32_t total = ordered_bits_total(x);
        if (std::isnan(x)) {
            if (total != 0xffffffffu) fail("total: a NaN's key is all ones", b, total);
        } else {
            if (b != 0x80000000u && total != key) fail("total: the plain map away from NaN and -0.0", b, total);
            numbers.push_back(x);
            plain_keys.push_back(key);
            total_keys.push_back(total);
        }
        if (ordered_is_finite(total) != std::isfinite(x)) fail("ordered_is_finite", b, total);
        if (finite_bits(x) != std::isfinite(x)) fail("finite_bits", b, 0);
    }
    check_order("plain map's order", numbers, plain_keys, true);
    check_order("total map's order", numbers, total_keys, false);

    // fp64: the floats widened (NaNs stay NaNs, payload and sign as the conversion leaves them), and fp64's own edges
    std::vector<double> wide;
    for (const float x : inputs) wide.push_back(static_cast<double>(x));
    for (const double m : {0.0, DBL_TRUE_MIN, DBL_MIN, std::nextafter(DBL_MIN, 0.0), 1.0, std::nextafter(1.0, 0.0), std::nextafter(1.0, 2.0),
                           1e20, std::nextafter(1e20, 0.0), DBL_MAX, std::nextafter(DBL_MAX, 0.0), double(INFINITY)}) {
        wide.push_back(m);
        wide.push_back(-m);
    }
    for (const uint64_t nan : {0x7ff8000000000000ull, 0xfff8000000000000ull, 0x7ff0000000000001ull, 0xfff0000000000001ull,
                               0x7fffffffffffffffull, 0xffffffffffffffffull, 0x7ff4000000000000ull, 0xfff4000000000000ull})
        wide.push_back(double_of(nan));
    const uint64_t sign64 = uint64_t{1} << 63;
    const uint64_t pos_inf_key64 = ordered_bits_total(double(INFINITY));
    if (!(pos_inf_key64 < ~uint64_t{0})) fail("fp64: +inf's key below all ones", pos_inf_key64, 0);
    if (ordered_bits_total(-0.0) != ordered_bits_total(0.0)) fail("fp64: the zeros share a key", 0, 0);
    std::vector<double> numbers64;
    std::vector<uint64_t> keys64;
    for (const double x : wide) {
        const uint64_t b = bits_of(x);
        const uint64_t total = ordered_bits_total(x);
        if (std::isnan(x)) {
            if (total != ~uint64_t{0}) fail("fp64: a NaN's key is all ones", b, total);
            continue;
        }
        const uint64_t plain = (b & sign64) ? ~b : (b | sign64);       // the plain map, restated for 64 bits
        if (b != sign64 && total != plain) fail("fp64: the plain map away from NaN and -0.0", b, total);
        numbers64.push_back(x);
        keys64.push_back(total);
    }
    check_order("fp64 total map's order", numbers64, keys64, false);

    if (visit_position(0) != 1 || visit_position(1) != 0) fail("visit positions of rows 0 and 1", 0, 0);
    for (int u = 0; u < (1 << 20); ++u)
        if (row_of_visit(visit_position(u)) != u) fail("row_of_visit(visit_position(u))", static_cast<uint64_t>(u), 0);

    if (failures != 0) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("order_keys ok: %zu floats, %zu doubles\n", inputs.size(), wide.size());
    return 0;
}
