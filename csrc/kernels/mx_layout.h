// Layout of the block-scaled FP8 wire format `mxfp8_e4m3` (docs/collectives.md, "Compressed
// all-reduce"). Host and device, no HIP runtime call: the kernels (mx_wire.hip), the bindings and
// tests/native/mx_layout_check.cpp all read the one definition.
//
// A block is 32 consecutive elements: 32 float8_e4m3fn payload bytes and one E8M0 scale byte. The
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
constexpr size_t kMxBlockWire = kMxBlock + 1;    // wire bytes per block
constexpr size_t kMxScaleAlign = 16;             // cb is a multiple of this: the scale area stays 16-B aligned
constexpr size_t kMxBigChunk = size_t(1) << 20;  // from this chunk wire size on ...
constexpr size_t kMxBigAlign = 4096;             // ... cb is a multiple of 4096 blocks (33 cb = whole 4-KiB tiles)

PDCC_MX_HD inline size_t mx_round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

PDCC_MX_HD inline size_t mx_blocks(size_t numel) { return (numel + kMxBlock - 1) / kMxBlock; }

// blocks per chunk when `numel` elements are dealt to `world` chunks (at least one group of 16)
PDCC_MX_HD inline size_t mx_chunk_blocks(size_t numel, int world) {
  const size_t w = world > 0 ? (size_t)world : 1;
  size_t cb = mx_round_up((mx_blocks(numel) + w - 1) / w, kMxScaleAlign);
  if (cb == 0) cb = kMxScaleAlign;
  if (kMxBlockWire * cb >= kMxBigChunk) cb = mx_round_up(cb, kMxBigAlign);
  return cb;
}

PDCC_MX_HD inline size_t mx_chunk_bytes(size_t cb) { return kMxBlockWire * cb; }
PDCC_MX_HD inline size_t mx_wire_bytes(size_t cb, size_t nchunks) { return mx_chunk_bytes(cb) * nchunks; }

// byte offsets inside one chunk
PDCC_MX_HD inline size_t mx_payload_off(size_t block) { return (size_t)kMxBlock * block; }
PDCC_MX_HD inline size_t mx_scale_off(size_t cb, size_t block) { return (size_t)kMxBlock * cb + block; }


// ---- shard layout: chunk r is shard r (elements r m .. (r + 1) m - 1), blocks counted from r m
PDCC_MX_HD inline size_t mx_shard_blocks(size_t m) { return mx_chunk_blocks(m, 1); }
PDCC_MX_HD inline size_t mx_shard_wire_bytes(size_t m, size_t world) {
  return mx_wire_bytes(mx_shard_blocks(m), world > 0 ? world : 1);
}
// wire byte of the payload of element i (of world * m) and of the scale of its block
PDCC_MX_HD inline size_t mx_shard_payload_byte(size_t m, size_t i) {
  const size_t r = i / m;
  return r * mx_chunk_bytes(mx_shard_blocks(m)) + (i - r * m);
}
PDCC_MX_HD inline size_t mx_shard_scale_byte(size_t m, size_t i) {
  const size_t r = i / m, cb = mx_shard_blocks(m);
  return r * mx_chunk_bytes(cb) + mx_scale_off(cb, (i - r * m) / kMxBlock);
}

}  // namespace kern
}  // namespace pdcc
