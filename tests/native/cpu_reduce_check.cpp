// The host reduction (csrc/host/cpu_reduce.h) on integer edge values, built stand-alone with ASan + UBSan
// (tests/test_exact_cpu.py): signed SUM / PRODUCT wrap without signed overflow, AVG divides the wrapped sum
// truncating toward zero, and the results equal the same arithmetic done here in unsigned 64-bit.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

#include "host/cpu_reduce.h"

namespace {

using pdcc::host::RedOpType;
long g_checked = 0;
int g_bad = 0;

template <class T>
std::vector<T> edges() {
  using L = std::numeric_limits<T>;
  std::vector<T> e = {T(0), T(1), T(2), T(3), L::max(), T(L::max() - 1), T(L::max() / 2 + 1), L::min(), T(L::min() + 1)};
  if (L::is_signed) {
    e.push_back(T(-1));
    e.push_back(T(-2));
    e.push_back(T(-3));
    e.push_back(T(L::min() / 2));
  }
  if (sizeof(T) == 8) {
    e.push_back(T(0xFFFFFFFFll));
    e.push_back(T(0x100000000ll));
    e.push_back(T(0x1234567880000000ll));
  }
  if (sizeof(T) >= 4) e.push_back(T(46341));
  if (sizeof(T) >= 2) e.push_back(T(181)), e.push_back(T(256));
  return e;
}

// two's-complement wrap of a 64-bit pattern to T, without any signed arithmetic
template <class T>
T wrap(uint64_t v) {
  using U = std::make_unsigned_t<T>;
  const U u = static_cast<U>(v);
  T t;
  std::memcpy(&t, &u, sizeof(T));
  return t;
}
template <class T>
uint64_t bits(T t) {
  std::make_unsigned_t<T> u;
  std::memcpy(&u, &t, sizeof(T));
  return static_cast<uint64_t>(u);
}

template <class T>
void check(at::ScalarType st, const char* name) {
  const std::vector<T> e = edges<T>();
  const size_t m = e.size(), n = m * m * m;  // every triple: three sources
  std::vector<T> a(n), b(n), c(n), out(n);
  for (size_t i = 0; i < n; ++i) a[i] = e[i / (m * m)], b[i] = e[(i / m) % m], c[i] = e[i % m];
  const void* srcs[3] = {a.data(), b.data(), c.data()};
  for (RedOpType op : {RedOpType::SUM, RedOpType::PRODUCT, RedOpType::AVG}) {
    pdcc::host::reduce_cpu(st, out.data(), srcs, 3, n, op, 3);
    for (size_t i = 0; i < n; ++i) {
      T want;
      if (op == RedOpType::PRODUCT) {
        want = wrap<T>(bits(a[i]) * bits(b[i]) * bits(c[i]));
      } else {
        want = wrap<T>(bits(a[i]) + bits(b[i]) + bits(c[i]));
        if (op == RedOpType::AVG) want = static_cast<T>(want / T(3));  // (promoted for narrow types: no overflow)
      }
      ++g_checked;
      if (out[i] != want && g_bad++ < 10)
        std::printf("%s op %d: %lld %lld %lld -> %lld, want %lld\n", name, (int)op, (long long)a[i], (long long)b[i],
                    (long long)c[i], (long long)out[i], (long long)want);
    }
  }
  // in place (dst aliases srcs[0]), two sources
  std::vector<T> d = a;
  const void* two[2] = {d.data(), b.data()};
  pdcc::host::reduce_cpu(st, d.data(), two, 2, n, RedOpType::SUM, 2);
  for (size_t i = 0; i < n; ++i, ++g_checked)
    if (d[i] != wrap<T>(bits(a[i]) + bits(b[i])) && g_bad++ < 10) std::printf("%s in place: element %zu\n", name, i);
}

}  // namespace

int main() {
  check<int8_t>(at::kChar, "int8");
  check<uint8_t>(at::kByte, "uint8");
  check<int16_t>(at::kShort, "int16");
  check<int32_t>(at::kInt, "int32");
  check<int64_t>(at::kLong, "int64");
  if (g_bad) {
    std::printf("FAILED %d\n", g_bad);
    return 1;
  }
  std::printf("ok %ld\n", g_checked);
  return 0;
}
