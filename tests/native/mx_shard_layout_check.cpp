// Stand-alone check of the shard layout in csrc/kernels/mx_layout.h (built with ASan + UBSan by
// tests/test_mx_shard_cpu.py).
//
// For every (m, world) on the command line -- or a built-in list -- it walks a shard wire the way the
// kernels address it: every element of every shard marks its payload byte and (the first element of
// a block) its block's scale byte, then every padding position and padding block of every chunk does
// the same, all in a heap buffer of exactly mx_shard_wire_bytes() bytes. Every byte must be marked
// exactly once (an offset past the end is the sanitizer's to report), and no element of shard r may
// land outside chunk r. It prints one line "m world cb wire_bytes" per case, which the Python test
// compares with ops.mx_shard_blocks / ops.mx_shard_wire_bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels/mx_layout.h"

using namespace pdcc::kern;

static int fail(const char* what, size_t m, int world, size_t cb) {
  std::fprintf(stderr, "FAIL %s: m=%zu world=%d cb=%zu\n", what, m, world, cb);
  return 1;
}

static int check(size_t m, int world) {
  const size_t cb = mx_shard_blocks(m);
  const size_t bytes = mx_shard_wire_bytes(m, (size_t)world);
  if (cb != mx_chunk_blocks(m, 1)) return fail("cb is not mx_chunk_blocks(m, 1)", m, world, cb);
  if (cb % 16 || cb * kMxBlock < m) return fail("a chunk does not hold a shard", m, world, cb);
  if (bytes != (size_t)world * 33 * cb) return fail("wire bytes", m, world, cb);
  std::printf("%zu %d %zu %zu\n", m, world, cb, bytes);
  std::vector<unsigned char> seen(bytes, 0);
  for (int r = 0; r < world; ++r) {
    const size_t lo = (size_t)r * mx_chunk_bytes(cb), hi = lo + mx_chunk_bytes(cb);
    // the shard's elements, by their index in the tensor
    for (size_t i = (size_t)r * m; i < (size_t)(r + 1) * m; ++i) {
      const size_t p = mx_shard_payload_byte(m, i), s = mx_shard_scale_byte(m, i);
      if (p < lo || p >= hi || s < lo || s >= hi) return fail("an element leaves its shard's chunk", m, world, cb);
      if (p != lo + mx_payload_off((i - (size_t)r * m) / kMxBlock) + (i - (size_t)r * m) % kMxBlock)
        return fail("payload byte differs from block * 32 + position", m, world, cb);
      ++seen[p];
      if ((i - (size_t)r * m) % kMxBlock == 0) ++seen[s];
    }
    // what lies past the shard's end inside its chunk: the tail of the last block, then padding blocks
    unsigned char* chunk = seen.data() + lo;
    for (size_t e = m; e < cb * kMxBlock; ++e) {
      ++chunk[mx_payload_off(e / kMxBlock) + e % kMxBlock];
      if (e % kMxBlock == 0) ++chunk[mx_scale_off(cb, e / kMxBlock)];
    }
    if (mx_scale_off(cb, 0) % 16 || lo % 16) return fail("chunk or scale area is not 16-byte aligned", m, world, cb);
  }
  for (size_t i = 0; i < bytes; ++i)
    if (seen[i] != 1) return fail("a wire byte is not addressed exactly once", m, world, cb);
  return 0;
}

int main(int argc, char** argv) {
  int bad = 0, n = 0;
  if (argc > 1) {
    for (int i = 1; i + 1 < argc; i += 2, ++n)
      bad += check((size_t)std::strtoull(argv[i], nullptr, 10), std::atoi(argv[i + 1]));
  } else {
    const size_t sizes[] = {1, 31, 32, 33, 64, 511, 512, 513, 4113, 65553, 31776 * 32 - 1, 31776 * 32, (size_t)1 << 20};
    for (int w = 1; w <= 8; ++w)
      for (size_t s : sizes) {
        bad += check(s, w);
        ++n;
      }
  }
  if (bad) return 1;
  std::printf("ok %d\n", n);
  return 0;
}
