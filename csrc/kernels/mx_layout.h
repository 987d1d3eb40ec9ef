// Layout of the block-scaled wire formats `mxfp8_e4m3` (docs/collectives.md, "Compressed
// all-reduce"), `mxfp4_e2m1` ("The `mxfp4_e2m1` wire format") and `mxfp6_e2m3` ("The `mxfp6_e2m3` wire
// format"). Host and device, no HIP runtime call: the kernels (mx_wire.hip), the bindings and
// tests/native/mx_layout_check.cpp all read the one definition.
//
// A block is 32 consecutive elements: 32 float8_e4m3fn payload bytes and one E8M0 scale byte (FP4:
// 16 payload bytes, FP6: 24; read 16 or 24 for every 32 payload bytes below). The
// blocks of a tensor are dealt to `nchunks` chunks of `cb` blocks (one chunk per rank of an
// all-reduce); a chunk on the wire is
//     [32 * cb payload bytes][cb scale bytes]
// and a wire tensor is `nchunks` such chunks back to back. Block g of the tensor (elements
// 32 g .. 32 g + 31) is block g % cb of chunk g / cb.
//
// The shard layout ("Compressed reduce-scatter and all-gather") is the same chunks cut at shard
// boundaries: a shard wire of `world` shards of `m` elements is `world` chunks of
// cb = mx_shard_blocks(m) blocks, and block b of chunk r holds elements r m + 32 b .. r m + 32 b + 31
// of the tensor, clipped at (r + 1) m -- positions past the shard's end count as +0 and are never
// read from the next shard. Blocks are aligned to the start of each shard, not of the tensor, so for
// m % 32 != 0 the bytes differ from the dealt layout; when 32 * mx_chunk_blocks(world m, world) == m
// the two layouts are the same bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PDCC_MX_HD __host__ __device__
#else
#define PDCC_MX_HD
#endif

namespace pdcc {
namespace kern {

constexpr int kMxBlock = 32;                     // elements per block
constexpr size_t kMxBlockWire = kMxBlock + 1;    // wire bytes per block (mxfp8_e4m3)
constexpr size_t kMxScaleAlign = 16;             // cb is a multiple of this: the scale area stays 16-B aligned
constexpr size_t kMxBigChunk = size_t(1) << 20;  // from this chunk wire size on ...
constexpr size_t kMxBigAlign = 4096;             // ... cb is a multiple of 4096 blocks (whole 4-KiB tiles)

// The wire formats. They differ in the payload of a block only: 32 float8_e4m3fn bytes, or 16 bytes
// of two e2m1 nibbles each (element 2j in the low nibble of byte j, element 2j + 1 in the high one),
// or 24 bytes that are a little-endian stream of 32 e2m3 codes of 6 bits (element j in bits 6j .. 6j + 5
// of the block's 192; bit n of the stream is bit n % 8 of byte n / 8).
// The functions below without a format argument are the FP8 case of the ones that take one.
enum class MxFormat : int { FP8_E4M3 = 0, FP4_E2M1 = 1, FP6_E2M3 = 2 };

PDCC_MX_HD inline size_t mx_round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

PDCC_MX_HD inline size_t mx_blocks(size_t numel) { return (numel + kMxBlock - 1) / kMxBlock; }

// payload bytes and wire bytes (payload + one scale byte) of a block
PDCC_MX_HD constexpr size_t mx_block_payload(MxFormat f) {
  switch (f) {
    case MxFormat::FP4_E2M1: return 16;
    case MxFormat::FP6_E2M3: return 24;
    default: return 32;
  }
}
PDCC_MX_HD constexpr size_t mx_block_wire(MxFormat f) { return mx_block_payload(f) + 1; }

// blocks per chunk when `numel` elements are dealt to `world` chunks (at least one group of 16). The
// 4096 rule looks at the chunk's wire bytes, so near the threshold cb differs between the formats.
PDCC_MX_HD inline size_t mx_chunk_blocks(MxFormat f, size_t numel, int world) {
  const size_t w = world > 0 ? (size_t)world : 1;
  size_t cb = mx_round_up((mx_blocks(numel) + w - 1) / w, kMxScaleAlign);
  if (cb == 0) cb = kMxScaleAlign;
  if (mx_block_wire(f) * cb >= kMxBigChunk) cb = mx_round_up(cb, kMxBigAlign);
  return cb;
}
PDCC_MX_HD inline size_t mx_chunk_blocks(size_t numel, int world) {
  return mx_chunk_blocks(MxFormat::FP8_E4M3, numel, world);
}

PDCC_MX_HD inline size_t mx_chunk_bytes(MxFormat f, size_t cb) { return mx_block_wire(f) * cb; }
PDCC_MX_HD inline size_t mx_chunk_bytes(size_t cb) { return mx_chunk_bytes(MxFormat::FP8_E4M3, cb); }
PDCC_MX_HD inline size_t mx_wire_bytes(MxFormat f, size_t cb, size_t nchunks) { return mx_chunk_bytes(f, cb) * nchunks; }
PDCC_MX_HD inline size_t mx_wire_bytes(size_t cb, size_t nchunks) {
  return mx_wire_bytes(MxFormat::FP8_E4M3, cb, nchunks);
}

// byte offsets inside one chunk
PDCC_MX_HD inline size_t mx_payload_off(MxFormat f, size_t block) { return mx_block_payload(f) * block; }
PDCC_MX_HD inline size_t mx_payload_off(size_t block) { return mx_payload_off(MxFormat::FP8_E4M3, block); }
PDCC_MX_HD inline size_t mx_scale_off(MxFormat f, size_t cb, size_t block) { return mx_block_payload(f) * cb + block; }
PDCC_MX_HD inline size_t mx_scale_off(size_t cb, size_t block) { return mx_scale_off(MxFormat::FP8_E4M3, cb, block); }


// ---- shard layout: chunk r is shard r (elements r m .. (r + 1) m - 1), blocks counted from r m
PDCC_MX_HD inline size_t mx_shard_blocks(MxFormat f, size_t m) { return mx_chunk_blocks(f, m, 1); }
PDCC_MX_HD inline size_t mx_shard_blocks(size_t m) { return mx_shard_blocks(MxFormat::FP8_E4M3, m); }
PDCC_MX_HD inline size_t mx_shard_wire_bytes(MxFormat f, size_t m, size_t world) {
  return mx_wire_bytes(f, mx_shard_blocks(f, m), world > 0 ? world : 1);
}
PDCC_MX_HD inline size_t mx_shard_wire_bytes(size_t m, size_t world) {
  return mx_shard_wire_bytes(MxFormat::FP8_E4M3, m, world);
}
// wire byte of the payload of element i (of world * m; FP4: the byte that holds its nibble, the high
// one for an odd position in the shard; FP6: the byte that holds the lowest bit of its code) and of the
// scale of its block
PDCC_MX_HD inline size_t mx_shard_payload_byte(MxFormat f, size_t m, size_t i) {
  const size_t r = i / m;
  return r * mx_chunk_bytes(f, mx_shard_blocks(f, m)) + (i - r * m) * mx_block_payload(f) / kMxBlock;
}
PDCC_MX_HD inline size_t mx_shard_payload_byte(size_t m, size_t i) {
  return mx_shard_payload_byte(MxFormat::FP8_E4M3, m, i);
}
PDCC_MX_HD inline size_t mx_shard_scale_byte(MxFormat f, size_t m, size_t i) {
  const size_t r = i / m, cb = mx_shard_blocks(f, m);
  return r * mx_chunk_bytes(f, cb) + mx_scale_off(f, cb, (i - r * m) / kMxBlock);
}
PDCC_MX_HD inline size_t mx_shard_scale_byte(size_t m, size_t i) {
  return mx_shard_scale_byte(MxFormat::FP8_E4M3, m, i);
}

}  // namespace kern
}  // namespace pdcc
