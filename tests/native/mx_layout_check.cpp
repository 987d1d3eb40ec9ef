// Stand-alone check of csrc/kernels/mx_layout.h (built with ASan + UBSan by tests/test_mx_cpu.py).
//
// For every (numel, world) on the command line -- or a built-in list -- it checks the chunk size
// rules and then walks the offsets: every block of every chunk marks its 32 payload bytes and its
// scale byte in a heap buffer of exactly mx_wire_bytes() bytes, and every byte must be marked
// exactly once (an offset past the end is the sanitizer's to report). It prints one line
// "numel world cb wire_bytes" per case, which the Python test compares with ops.mx_chunk_blocks.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels/mx_layout.h"

using namespace pdcc::kern;

static int fail(const char* what, size_t numel, int world, size_t cb) {
  std::fprintf(stderr, "FAIL %s: numel=%zu world=%d cb=%zu\n", what, numel, world, cb);
  return 1;
}

static int check(size_t numel, int world, bool walk) {
  const size_t cb = mx_chunk_blocks(numel, world);
  const size_t bytes = mx_wire_bytes(cb, (size_t)world);
  if (cb == 0 || cb % 16) return fail("cb is not a positive multiple of 16", numel, world, cb);
  if (cb * (size_t)world < mx_blocks(numel)) return fail("chunks do not hold the tensor", numel, world, cb);
  if (mx_chunk_bytes(cb) != 33 * cb || mx_chunk_bytes(cb) % 16) return fail("chunk bytes", numel, world, cb);
  if (mx_chunk_bytes(cb) >= (size_t(1) << 20)) {
    if (cb % 4096 || mx_chunk_bytes(cb) % 4096) return fail("a chunk of 1 MiB or more is not whole tiles", numel, world, cb);
  }
  // the documented rule, spelled out once more: the chunk's share of the blocks, up to a multiple of
  // 16 (at least 16), and up to a multiple of 4096 once 33 of those bytes reach 1 MiB
  size_t want = ((mx_blocks(numel) + (size_t)world - 1) / (size_t)world + 15) / 16 * 16;
  if (want == 0) want = 16;
  if (33 * want >= 1048576) want = (want + 4095) / 4096 * 4096;
  if (cb != want) return fail("cb differs from the documented rule", numel, world, cb);
  std::printf("%zu %d %zu %zu\n", numel, world, cb, bytes);
  if (!walk) return 0;
  std::vector<unsigned char> seen(bytes, 0);
  for (int c = 0; c < world; ++c) {
    unsigned char* chunk = seen.data() + (size_t)c * mx_chunk_bytes(cb);
    for (size_t b = 0; b < cb; ++b) {
      for (int i = 0; i < kMxBlock; ++i) ++chunk[mx_payload_off(b) + i];
      ++chunk[mx_scale_off(cb, b)];
    }
    if (mx_scale_off(cb, 0) % 16) return fail("scale area is not 16-byte aligned", numel, world, cb);
  }
  for (size_t i = 0; i < bytes; ++i)
    if (seen[i] != 1) return fail("a wire byte is not owned by exactly one block", numel, world, cb);
  return 0;
}

int main(int argc, char** argv) {
  int bad = 0, n = 0;
  if (argc > 1) {
    for (int i = 1; i + 1 < argc; i += 2, ++n)
      bad += check((size_t)std::strtoull(argv[i], nullptr, 10), std::atoi(argv[i + 1]), true);
  } else {
    for (int w = 1; w <= 8; ++w) {
      const size_t sizes[] = {0, 1, 31, 32, 33, 511, 513, 4096 + 17, 65536 + 17, 70001, (size_t)512 * w - 1,
                              (size_t)512 * w + 1, (size_t)4 << 20, ((size_t)1 << 20) * 32 / 33 * (size_t)w};
      for (size_t s : sizes) {
        bad += check(s, w, true);
        ++n;
      }
      // around the 1 MiB chunk threshold (31776 blocks of 33 bytes) and far past 2^31 elements (rules only)
      for (size_t blocks = 31744; blocks <= 31808; blocks += 16, ++n) bad += check(blocks * 32 * w, w, blocks % 32 == 0);
      bad += check(((size_t)1 << 33) + 5, w, false);
      ++n;
    }
  }
  if (bad) return 1;
  std::printf("ok %d\n", n);
  return 0;
}
