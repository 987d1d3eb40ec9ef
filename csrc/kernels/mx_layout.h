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

}  // namespace kern
}  // namespace pdcc
