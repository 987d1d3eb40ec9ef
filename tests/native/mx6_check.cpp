// Stand-alone check of the `mxfp6_e2m3` parts of csrc/kernels/mx_layout.h and csrc/kernels/mx_sr.h on the
// host (built with ASan + UBSan by tests/test_mx6_cpu.py). Every argument is one query, answered with one
// line of decimal numbers:
//
//   d:N:W       N elements dealt to W chunks: "cb wire_bytes"
//   s:M:W       W shards of M elements: "cb wire_bytes"
//   c:CB        a chunk of CB blocks: "chunk_bytes payload_off(CB - 1) scale_off(0) scale_off(CB - 1)"
//   p:M:I       element I of a shard wire of M-element shards: "payload_byte scale_byte"
//   e2m3:S:U    the e2m3 code (sign in bit 5) of the scaled value with f32 bits S under the word U
//
// Numbers in the queries are hexadecimal without a prefix. The last line is "ok <queries>". Without
// arguments the program runs a self-check: the constants of the format, the other formats' numbers next to
// it, and the codes' monotony in S and in U.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kernels/mx_layout.h"
#include "kernels/mx_sr.h"

using namespace pdcc::kern;

static const MxFormat F6 = MxFormat::FP6_E2M3;

static int fail(const char* what, const char* arg) {
  fprintf(stderr, "mx6_check: %s: %s\n", what, arg);
  return 2;
}

static int self_check() {
  long n = 0;
  static_assert((int)MxFormat::FP6_E2M3 == 2, "the format's number is part of the interface");
  static_assert(mx_block_payload(MxFormat::FP6_E2M3) == 24 && mx_block_wire(MxFormat::FP6_E2M3) == 25, "24 + 1 bytes");
  static_assert(mx_block_payload(MxFormat::FP8_E4M3) == 32 && mx_block_payload(MxFormat::FP4_E2M1) == 16, "unchanged");
  // the 4096 rule: 25 cb reaches 2^20 between cb = 41936 and cb = 41952
  if (mx_chunk_blocks(F6, 41936u * 32u, 1) != 41936 || 25u * 41936u >= kMxBigChunk) return fail("below 1 MiB", "self-check");
  if (mx_chunk_blocks(F6, 41936u * 32u + 1u, 1) != 45056 || 25u * 41952u < kMxBigChunk) return fail("at 1 MiB", "self-check");
  if (mx_chunk_blocks(F6, 0, 3) != 16 || mx_wire_bytes(F6, 16, 3) != 1200) return fail("smallest chunk", "self-check");
  for (size_t cb = 16; cb <= 4096; cb += 16) {  // chunk starts and scale areas stay 16-byte aligned
    if (mx_chunk_bytes(F6, cb) % 16 || mx_scale_off(F6, cb, 0) % 16 || mx_payload_off(F6, 1) != 24) return fail("alignment", "self-check");
    ++n;
  }
  // the byte of an element's lowest bit: 6 j / 8 within the block
  for (size_t i = 0; i < 96; ++i) {
    const size_t want = (i / 32) * 24 + (6 * (i % 32)) / 8;
    if (mx_shard_payload_byte(F6, 96, i) != want) return fail("payload byte", "self-check");
    if (mx_shard_payload_byte(F6, 96, 96 + i) != want + mx_chunk_bytes(F6, 16)) return fail("second shard", "self-check");
    if (mx_shard_scale_byte(F6, 96, i) != 24 * 16 + i / 32) return fail("scale byte", "self-check");
    ++n;
  }
  // every f32 in [0, 7.5] in steps of 2^12 bit patterns, the ends of the word range
  const uint32_t us[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
  uint32_t prev[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t s = 0; s <= 0x40f00000u; s += 4096u) {
    uint32_t last = 0xffffffffu;
    for (int j = 0; j < 6; ++j) {
      const uint32_t c = mx_sr_e2m3(s, us[j]);
      if (mx_sr_e2m3(s | 0x80000000u, us[j]) != (c | 0x20u)) return fail("sign", "self-check");
      if (c > 31u) return fail("range", "self-check");
      if (c < prev[j]) return fail("not monotone in s", "self-check");
      if (j > 0 && c > last) return fail("not monotone in u", "self-check");
      if (j > 0 && last - c > 1u) return fail("more than one step", "self-check");
      prev[j] = c;
      last = c;
      ++n;
    }
  }
  if (mx_sr_e2m3(0x40f00000u, 0u) != 31u || mx_sr_e2m3(0x3f800000u, 0xffffffffu) != 8u) return fail("grid points", "self-check");
  printf("ok %ld\n", n);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_check();
  for (int i = 1; i < argc; ++i) {
    char kind[8] = {0};
    const char* c1 = strchr(argv[i], ':');
    if (!c1 || c1 - argv[i] >= (long)sizeof(kind)) return fail("bad query", argv[i]);
    memcpy(kind, argv[i], (size_t)(c1 - argv[i]));
    char* end = nullptr;
    unsigned long long a = strtoull(c1 + 1, &end, 16), b = 0;
    if (end == c1 + 1) return fail("bad number", argv[i]);
    const bool two = *end == ':';
    if (two) {
      const char* p = end + 1;
      b = strtoull(p, &end, 16);
      if (end == p) return fail("bad number", argv[i]);
    }
    if (*end != 0) return fail("trailing text", argv[i]);
    if (!strcmp(kind, "d") && two && b >= 1) {
      const size_t cb = mx_chunk_blocks(F6, (size_t)a, (int)b);
      printf("%zu %zu\n", cb, mx_wire_bytes(F6, cb, (size_t)b));
    } else if (!strcmp(kind, "s") && two && a >= 1 && b >= 1) {
      printf("%zu %zu\n", mx_shard_blocks(F6, (size_t)a), mx_shard_wire_bytes(F6, (size_t)a, (size_t)b));
    } else if (!strcmp(kind, "c") && !two && a >= 1) {
      printf("%zu %zu %zu %zu\n", mx_chunk_bytes(F6, (size_t)a), mx_payload_off(F6, (size_t)a - 1),
             mx_scale_off(F6, (size_t)a, 0), mx_scale_off(F6, (size_t)a, (size_t)a - 1));
    } else if (!strcmp(kind, "p") && two && a >= 1) {
      printf("%zu %zu\n", mx_shard_payload_byte(F6, (size_t)a, (size_t)b), mx_shard_scale_byte(F6, (size_t)a, (size_t)b));
    } else if (!strcmp(kind, "e2m3") && two) {
      printf("%u\n", mx_sr_e2m3((uint32_t)a, (uint32_t)b));
    } else {
      return fail("unknown query", argv[i]);
    }
  }
  printf("ok %d\n", argc - 1);
  return 0;
}
