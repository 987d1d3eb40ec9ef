// Host-side check of csrc/kernels/mx_rot.h, built stand-alone under ASan + UBSan by tests/test_mx_rot_cpu.py.
//
//   mx_rot_check                  self-check: R^-1 R x == x on integer blocks, H H = 32 I; prints "ok"
//   mx_rot_check QUERY...         one line of hexadecimal words per query, then "ok <count>":
//     g:SEED                      the sign word of SEED
//     f:SEED:B0:...:B31           the f32 bits of R x for the block with the f32 bits B0..B31
//     i:SEED:B0:...:B31           the f32 bits of R^-1 x
// Every number is hexadecimal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kernels/mx_rot.h"

using namespace pdcc::kern;

static std::vector<uint64_t> fields(const char* s) {
  std::vector<uint64_t> out;
  std::string cur;
  for (const char* p = s;; ++p) {
    if (*p == ':' || *p == 0) {
      out.push_back(strtoull(cur.c_str(), nullptr, 16));
      cur.clear();
      if (*p == 0) break;
    } else {
      cur.push_back(*p);
    }
  }
  return out;
}

static int self_check() {
  for (uint64_t seed : {0ull, 1ull, 0xC0FFEE12345678ull, ~0ull}) {
    const uint32_t sg = mx_rot_signs(seed);
    float x[32], y[32];
    for (int j = 0; j < 32; ++j) x[j] = y[j] = (float)(((int)(seed % 977) + 131 * j * j) % 4001 - 2000);
    mx_rot_forward(y, sg);
    double first = 0;  // row 0 of H diag(s): the signed sum
    for (int j = 0; j < 32; ++j) first += ((sg >> j) & 1u) ? -(double)x[j] : (double)x[j];
    if ((double)y[0] != first) return 1;
    mx_rot_inverse(y, sg);
    if (memcmp(x, y, sizeof x) != 0) return 2;
  }
  float e[32] = {0};
  e[5] = 1.0f;
  mx_rot_butterfly(e);
  mx_rot_butterfly(e);
  for (int j = 0; j < 32; ++j)
    if (e[j] != (j == 5 ? 32.0f : 0.0f)) return 3;
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) {
    const int bad = self_check();
    if (bad) {
      printf("self-check %d failed\n", bad);
      return 1;
    }
    printf("ok\n");
    return 0;
  }
  for (int a = 1; a < argc; ++a) {
    const char kind = argv[a][0];
    if (argv[a][1] != ':') return 2;
    const std::vector<uint64_t> f = fields(argv[a] + 2);
    if (kind == 'g' && f.size() == 1) {
      printf("%x\n", mx_rot_signs(f[0]));
    } else if ((kind == 'f' || kind == 'i') && f.size() == 33) {
      float y[32];
      for (int j = 0; j < 32; ++j) y[j] = mx_rot_float((uint32_t)f[1 + j]);
      if (kind == 'f') mx_rot_forward(y, mx_rot_signs(f[0]));
      else mx_rot_inverse(y, mx_rot_signs(f[0]));
      for (int j = 0; j < 32; ++j) printf("%x%c", mx_rot_bits(y[j]), j == 31 ? '\n' : ' ');
    } else {
      return 2;
    }
  }
  printf("ok %d\n", argc - 1);
  return 0;
}
