// Stand-alone check of the FP4 (`mxfp4_e2m1`) forms of csrc/kernels/mx_layout.h (built with ASan +
// UBSan by tests/test_mx4_cpu.py).
//
// Arguments are triples "d numel world" (the dealt layout) or "s m world" (the shard layout); without
// arguments a built-in list runs. For each case it checks the chunk size rules (16 payload bytes and
// one scale byte per block, cb a multiple of 16, and of 4096 once 17 cb reaches 1 MiB) and walks the
// wire the way the kernels address it, in a heap buffer of exactly the wire's size: every nibble of
// every payload byte and every scale byte must be claimed exactly once (an offset past the end is the
// sanitizer's to report). It also checks that the functions without a format argument are the FP8
// case of the ones with one. It prints one line "d|s n world cb wire_bytes" per case, which the
// Python test compares with ops.mx_chunk_blocks(..., wire="mxfp4_e2m1") and its kin.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels/mx_layout.h"

using namespace pdcc::kern;

static constexpr MxFormat F4 = MxFormat::FP4_E2M1, F8 = MxFormat::FP8_E4M3;

static int fail(const char* what, char mode, size_t n, int world, size_t cb) {
  std::fprintf(stderr, "FAIL %s: %c n=%zu world=%d cb=%zu\n", what, mode, n, world, cb);
  return 1;
}

static int rules(char mode, size_t n, int world, size_t cb, size_t per_chunk_blocks) {
  if (mx_block_payload(F4) != 16 || mx_block_wire(F4) != 17) return fail("block bytes", mode, n, world, cb);
  if (cb == 0 || cb % 16) return fail("cb is not a positive multiple of 16", mode, n, world, cb);
  if (cb < per_chunk_blocks) return fail("a chunk does not hold its blocks", mode, n, world, cb);
  if (mx_chunk_bytes(F4, cb) != 17 * cb || mx_chunk_bytes(F4, cb) % 16) return fail("chunk bytes", mode, n, world, cb);
  if (mx_scale_off(F4, cb, 0) != 16 * cb || mx_scale_off(F4, cb, 0) % 16) return fail("scale area", mode, n, world, cb);
  if (mx_chunk_bytes(F4, cb) >= (size_t(1) << 20) && (cb % 4096 || mx_chunk_bytes(F4, cb) % 4096))
    return fail("a chunk of 1 MiB or more is not whole tiles", mode, n, world, cb);
  size_t want = (per_chunk_blocks + 15) / 16 * 16;
  if (want == 0) want = 16;
  if (17 * want >= 1048576) want = (want + 4095) / 4096 * 4096;
  if (cb != want) return fail("cb differs from the documented rule", mode, n, world, cb);
  return 0;
}

// the existing names are the FP8 case of the new ones
static int fp8_forms(size_t n, int world) {
  const size_t cb = mx_chunk_blocks(n, world);
  bool ok = cb == mx_chunk_blocks(F8, n, world) && mx_chunk_bytes(cb) == mx_chunk_bytes(F8, cb) &&
            mx_wire_bytes(cb, (size_t)world) == mx_wire_bytes(F8, cb, (size_t)world) &&
            mx_payload_off(7) == mx_payload_off(F8, 7) && mx_scale_off(cb, 7) == mx_scale_off(F8, cb, 7) &&
            mx_block_payload(F8) == 32 && mx_block_wire(F8) == kMxBlockWire;
  if (n > 0)
    ok = ok && mx_shard_blocks(n) == mx_shard_blocks(F8, n) &&
         mx_shard_wire_bytes(n, (size_t)world) == mx_shard_wire_bytes(F8, n, (size_t)world) &&
         mx_shard_payload_byte(n, n - 1) == mx_shard_payload_byte(F8, n, n - 1) &&
         mx_shard_scale_byte(n, n - 1) == mx_shard_scale_byte(F8, n, n - 1);
  return ok ? 0 : fail("the FP8 names differ from the FP8 case", 'd', n, world, cb);
}

static int check_dealt(size_t numel, int world, bool walk) {
  const size_t cb = mx_chunk_blocks(F4, numel, world);
  const size_t bytes = mx_wire_bytes(F4, cb, (size_t)world);
  if (rules('d', numel, world, cb, (mx_blocks(numel) + (size_t)world - 1) / (size_t)world)) return 1;
  if (bytes != 17 * cb * (size_t)world) return fail("wire bytes", 'd', numel, world, cb);
  if (fp8_forms(numel, world)) return 1;
  std::printf("d %zu %d %zu %zu\n", numel, world, cb, bytes);
  if (!walk) return 0;
  std::vector<unsigned char> seen(bytes, 0);  // payload bytes count nibbles (2), scale bytes count 2 at once
  for (int c = 0; c < world; ++c) {
    unsigned char* chunk = seen.data() + (size_t)c * mx_chunk_bytes(F4, cb);
    for (size_t b = 0; b < cb; ++b) {
      for (int i = 0; i < kMxBlock; ++i) ++chunk[mx_payload_off(F4, b) + (size_t)i / 2];
      chunk[mx_scale_off(F4, cb, b)] += 2;
    }
  }
  for (size_t i = 0; i < bytes; ++i)
    if (seen[i] != 2) return fail("a wire byte is not owned by exactly one block", 'd', numel, world, cb);
  return 0;
}

static int check_shards(size_t m, int world, bool walk) {
  const size_t cb = mx_shard_blocks(F4, m);
  const size_t bytes = mx_shard_wire_bytes(F4, m, (size_t)world);
  if (cb != mx_chunk_blocks(F4, m, 1)) return fail("cb is not mx_chunk_blocks(m, 1)", 's', m, world, cb);
  if (rules('s', m, world, cb, mx_blocks(m))) return 1;
  if (bytes != 17 * cb * (size_t)world) return fail("wire bytes", 's', m, world, cb);
  std::printf("s %zu %d %zu %zu\n", m, world, cb, bytes);
  if (!walk) return 0;
  std::vector<unsigned char> seen(bytes, 0);
  for (int r = 0; r < world; ++r) {
    const size_t lo = (size_t)r * mx_chunk_bytes(F4, cb), hi = lo + mx_chunk_bytes(F4, cb);
    for (size_t i = (size_t)r * m; i < (size_t)(r + 1) * m; ++i) {
      const size_t k = i - (size_t)r * m;  // position in the shard
      const size_t p = mx_shard_payload_byte(F4, m, i), s = mx_shard_scale_byte(F4, m, i);
      if (p < lo || p >= hi || s < lo || s >= hi) return fail("an element leaves its shard's chunk", 's', m, world, cb);
      if (p != lo + mx_payload_off(F4, k / kMxBlock) + k % kMxBlock / 2)
        return fail("payload byte differs from block * 16 + position / 2", 's', m, world, cb);
      ++seen[p];
      if (k % kMxBlock == 0) seen[s] += 2;
    }
    // what lies past the shard's end inside its chunk: the tail of the last block, then padding blocks
    unsigned char* chunk = seen.data() + lo;
    for (size_t e = m; e < cb * kMxBlock; ++e) {
      ++chunk[mx_payload_off(F4, e / kMxBlock) + e % kMxBlock / 2];
      if (e % kMxBlock == 0) chunk[mx_scale_off(F4, cb, e / kMxBlock)] += 2;
    }
    if (lo % 16) return fail("a chunk is not 16-byte aligned", 's', m, world, cb);
  }
  for (size_t i = 0; i < bytes; ++i)
    if (seen[i] != 2) return fail("a wire byte is not addressed exactly once", 's', m, world, cb);
  return 0;
}

int main(int argc, char** argv) {
  int bad = 0, n = 0;
  if (argc > 1) {
    for (int i = 1; i + 2 < argc; i += 3, ++n) {
      const size_t v = (size_t)std::strtoull(argv[i + 1], nullptr, 10);
      const int w = std::atoi(argv[i + 2]);
      bad += argv[i][0] == 's' ? check_shards(v, w, true) : check_dealt(v, w, true);
    }
  } else {
    for (int w = 1; w <= 8; ++w) {
      const size_t sizes[] = {1, 31, 32, 33, 63, 65, 511, 513, 4113, 65553, (size_t)512 * w - 1, (size_t)512 * w + 1};
      for (size_t s : sizes) {
        bad += check_dealt(s, w, true) + check_shards(s, w, true);
        n += 2;
      }
      bad += check_dealt(0, w, true);
      ++n;
      // around the 1 MiB chunk threshold: 17 * 61680 = 2^20 - 16, 17 * 61696 = 2^20 + 256
      for (size_t blocks = 61648; blocks <= 61712; blocks += 16, n += 2) {
        bad += check_dealt(blocks * 32 * w, w, blocks % 32 == 0);
        bad += check_shards(blocks * 32 - 5, w, w <= 2 && blocks % 32 == 0);
      }
      bad += check_dealt(((size_t)1 << 33) + 5, w, false);
      ++n;
    }
  }
  if (bad) return 1;
  std::printf("ok %d\n", n);
  return 0;
}
