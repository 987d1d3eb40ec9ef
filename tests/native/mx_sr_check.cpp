// Stand-alone check of csrc/kernels/mx_sr.h on the host (built with ASan + UBSan by
// tests/test_mx_sr_cpu.py). Every argument is one query, answered with one decimal number per line:
//
//   e4m3:S:U     the float8_e4m3fn byte of the scaled value with f32 bits S under the word U
//   e2m1:S:U     the e2m1 code (sign in bit 3) likewise
//   mix:X        mx_sr_mix(X)
//   key:SEED:ST  the key of a call
//   word:K:I     the word of element index I (64 bits) under the key K
//
// Numbers are hexadecimal without a prefix. The last line is "ok <queries>". Without arguments the
// program runs a self-check: on-grid values never move, and the codes are monotone in S and in U.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kernels/mx_sr.h"

using namespace pdcc::kern;

static int fail(const char* what, const char* arg) {
  fprintf(stderr, "mx_sr_check: %s: %s\n", what, arg);
  return 2;
}

static int self_check() {
  long n = 0;
  // every f32 in [0, 448] / [0, 6] in steps of 2^12 bit patterns plus the ends of the word range
  const uint32_t us[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
  for (int fmt = 0; fmt < 2; ++fmt) {
    const uint32_t top = fmt == 0 ? 0x43e00000u : 0x40c00000u;  // 448, 6
    uint32_t prev[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t s = 0; s <= top; s += 4096u) {  // (both tops are multiples of 4096)
      uint32_t last = 0xffffffffu;
      for (int j = 0; j < 6; ++j) {
        const uint32_t c = fmt == 0 ? mx_sr_e4m3(s, us[j]) : mx_sr_e2m1(s, us[j]);
        const uint32_t cn = fmt == 0 ? mx_sr_e4m3(s | 0x80000000u, us[j]) : mx_sr_e2m1(s | 0x80000000u, us[j]);
        if (cn != (c | (fmt == 0 ? 0x80u : 0x8u))) return fail("sign", "self-check");
        if (c > (fmt == 0 ? 126u : 7u)) return fail("range", "self-check");
        if (c < prev[j]) return fail("not monotone in s", "self-check");
        if (j > 0 && c > last) return fail("not monotone in u", "self-check");
        if (j > 0 && last - c > 1u) return fail("more than one step", "self-check");
        prev[j] = c;
        last = c;
        ++n;
      }
    }
  }
  printf("ok %ld\n", n);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_check();
  for (int i = 1; i < argc; ++i) {
    char kind[8] = {0};
    unsigned long long a = 0, b = 0;
    const char* c1 = strchr(argv[i], ':');
    if (!c1 || c1 - argv[i] >= (long)sizeof(kind)) return fail("bad query", argv[i]);
    memcpy(kind, argv[i], (size_t)(c1 - argv[i]));
    char* end = nullptr;
    a = strtoull(c1 + 1, &end, 16);
    if (end == c1 + 1) return fail("bad number", argv[i]);
    const bool two = *end == ':';
    if (two) {
      const char* p = end + 1;
      b = strtoull(p, &end, 16);
      if (end == p) return fail("bad number", argv[i]);
    }
    if (*end != 0) return fail("trailing text", argv[i]);
    if (!strcmp(kind, "mix") && !two) printf("%u\n", mx_sr_mix((uint32_t)a));
    else if (!strcmp(kind, "e4m3") && two) printf("%u\n", mx_sr_e4m3((uint32_t)a, (uint32_t)b));
    else if (!strcmp(kind, "e2m1") && two) printf("%u\n", mx_sr_e2m1((uint32_t)a, (uint32_t)b));
    else if (!strcmp(kind, "key") && two) printf("%u\n", mx_sr_key((uint64_t)a, (uint32_t)b));
    else if (!strcmp(kind, "word") && two) printf("%u\n", mx_sr_word((uint32_t)a, (uint64_t)b));
    else return fail("unknown query", argv[i]);
  }
  printf("ok %d\n", argc - 1);
  return 0;
}
