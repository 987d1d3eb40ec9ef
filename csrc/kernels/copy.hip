// K2 multi-tensor pack/unpack and the copy family of the IPC collectives
// (broadcast, all-gather, gather, scatter, all-to-all, barrier), plus the
// host-side entry points that dispatch on dtype into reduce_<dt>.hip.
#include <algorithm>

#include "reduce_impl.h"

namespace pdcc {
namespace dev {

// --------------------------------------------------------------------------- K2
struct CopyArgs {
  kern::CopyDesc d[kern::kMaxCopyDescs];
  uint64_t prefix[kern::kMaxCopyDescs + 1];  // prefix sums of FULL tiles per descriptor
  int n;
  int ntail;                                  // descriptors with a partial last tile
  int tail_idx[kern::kMaxCopyDescs];
};

// Tile g of the launch lives in descriptor j with prefix[j] <= g < prefix[j+1]. A
// block visits its tiles in increasing order (and pipe_run asks for sources and
// destinations in increasing order too), so each side keeps a monotonic cursor:
// amortised O(1) uniform scalar steps per tile instead of a binary search.
struct DescMap {
  const CopyArgs* a;
  size_t first, stride, total;
  mutable int js = 0, jd = 0;  // descriptor cursors of the source and destination sides
  __device__ size_t count() const { return first < total ? (total - 1 - first) / stride + 1 : 0; }
  __device__ size_t advance(int& j, size_t i) const {
    const size_t g = first + i * stride;
    while (a->prefix[j + 1] <= g) ++j;
    return g - a->prefix[j];
  }
  __device__ const char* src(int, size_t i) const {
    const size_t lt = advance(js, i);
    return (const char*)a->d[js].src + lt * kTile;
  }
  __device__ char* dst(size_t i) const {
    const size_t lt = advance(jd, i);
    return (char*)a->d[jd].dst + lt * kTile;
  }
  __device__ size_t valid(size_t) const { return kTile; }
};

// NTL: non-temporal source loads (a pack / unpack reads each source once)
template <int D, bool NTL>
__global__ void __launch_bounds__(256) k2_multi_copy(CopyArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[PipeLds<1, D>::kBytes];
  const DescMap m{&a, blockIdx.x, gridDim.x, a.prefix[a.n]};
  pipe_run<DType::U8, RedOp::COPY, 1, D, DescMap, 1, false, NTL>(lds, m, 1);
  // partial last tiles: one block each, bounded plain loads
  for (int k = blockIdx.x; k < a.ntail; k += gridDim.x) {
    const kern::CopyDesc& d = a.d[a.tail_idx[k]];
    const size_t full = d.bytes / kTile * kTile;
    const size_t off = full + (threadIdx.x >> 6) * kWaveBytes + (threadIdx.x & 63) * 16;
    if (off < d.bytes) {
      const uint32_t lim = (uint32_t)(d.bytes - off < 16 ? d.bytes - off : 16);
      const char* s = (const char*)d.src + off;
      char* o = (char*)d.dst + off;
      if (lim == 16) *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>(s);
      else store_partial(o, load_partial(s, lim), lim);
    }
  }
}

// ----------------------------------------------------------- IPC copy family
// Dynamic zero-copy all-gather (IpcCall::dyn): items of K tiles, each pulled from every rank's
// input (owners rotated per item) into out[q]; the claim loop and departure of the dynamic
// all-reduce (reduce_impl.h).
template <int W>
__device__ __forceinline__ void ipc_allgather_dyn(const DView& v, const DCall& c, char* lds, const PhaseTrace* tr) {
  const uint32_t xb = xchg_blocks(c), G = gridDim.x - xb, b = blockIdx.x - xb;
  const size_t nt = c.bytes / kTile;
  const uint32_t K = kern::dyn_rows_per_chunk(nt, G, (uint32_t)c.dyn, (uint32_t)c.dyn_min_rows);
  const uint32_t nc = (uint32_t)((nt + K - 1) / K);
  const uint32_t dep = dyn_epoch(v, tr);
  dyn_claim_loop(v, nc, tr, b, G, [&](uint32_t it) {
    const size_t t0 = (size_t)it * K, t1 = t0 + K < nt ? t0 + K : nt;
    const PeerTileMap<W> m{&v, &c, 0, c.bytes, (uint32_t)(v.rank + it), t0, 1, t1};
    ipc_pipe<DType::U8, RedOp::COPY, 1, kCopyDepth>(lds, m, 1);
  });
  dyn_depart(v, dep, true, tr, G);
}

// Zero-copy copies (IpcCall::zc): peers' user buffers are read in place; data
// arrival barrier first, departure barrier last (see ipc_reduce_zc).
template <int W>
__device__ __forceinline__ void ipc_copy_zc(const DView& v, const DCall& c, char* lds, const PhaseTrace tr,
                                            uint32_t ep) {
  const size_t G = gridDim.x - xchg_blocks(c), b = blockIdx.x - xchg_blocks(c);  // the data blocks
  const int me = v.rank;
  const size_t nt = c.bytes / kTile;
  block_barrier(v, ep);
  tr.mark(2);
  tr.mark(4);
  if (c.coll == IpcColl::ALLGATHER && c.dyn) {
    ipc_allgather_dyn<W>(v, c, lds, &tr);
    tr.mark(5);
    return;
  }
  switch (c.coll) {
    case IpcColl::BROADCAST_2SHOT: {
      if (me != c.root) {  // phase 1: my owned tiles straight from the root's buffer into mine
        const OneSrcMap m{v.buf[c.root], v.buf[me], c.bytes, (size_t)me + W * b, W * G, nt};
        ipc_pipe<DType::U8, RedOp::COPY, 1, kCopyDepth>(lds, m, 1);
      }
      tr.mark(5);
      block_barrier(v, ep + 2u);
      tr.mark(6);
      if (me != c.root) {  // phase 2: the other owners' tiles (the root's own straight from the root)
        const PeerRowMap<W> m{&v, v.buf[me], (uint32_t)b, b, G, nt / W};
        ipc_pipe<DType::U8, RedOp::COPY, 1, kCopyDepth>(lds, m, 1);
      }
      break;
    }
    case IpcColl::ALLGATHER:
    case IpcColl::GATHER:
      if (c.coll == IpcColl::ALLGATHER || me == c.root) {
        const PeerTileMap<W> m{&v, &c, 0, c.bytes, (uint32_t)(me + b), b, G, nt};
        ipc_pipe<DType::U8, RedOp::COPY, 1, kCopyDepth>(lds, m, 1);
      }
      tr.mark(5);
      break;
    case IpcColl::ALLTOALL: {
      const PeerTileMap<W> m{&v, &c, (size_t)me * c.zstride, c.bytes, (uint32_t)(me + b), b, G, nt};
      ipc_pipe<DType::U8, RedOp::COPY, 1, kCopyDepth>(lds, m, 1);
      tr.mark(5);
      break;
    }
    case IpcColl::SCATTER: {  // my chunk straight out of the root's flat list
      const OneSrcMap m{v.buf[c.root] + (size_t)me * c.zstride, (char*)c.out[0], c.bytes, b, G, nt};
      ipc_pipe<DType::U8, RedOp::COPY, 1, kCopyDepth>(lds, m, 1);
      tr.mark(5);
      break;
    }
    default:
      break;
  }
  block_barrier<false>(v, ep + 3u);  // departure
}

template <int W>
__device__ __forceinline__ void ipc_copy_body(const DView& v, const DCall& c, char* lds, const PhaseTrace tr,
                                              uint32_t seq) {
  const size_t G = gridDim.x - xchg_blocks(c), b = blockIdx.x - xchg_blocks(c);  // the data blocks
  const int me = v.rank;
  tr.seq(seq);
  const uint32_t ep = seq * kern::kEpochsPerCall, ph0 = ep + 1u, ph1 = ep + 2u;
  if (c.coll == IpcColl::BARRIER) {  // the arrival barrier is the whole collective
    block_barrier<false>(v, ep);
    return;
  }
  if (c.zc) {
    ipc_copy_zc<W>(v, c, lds, tr, ep);
    return;
  }
  block_barrier<false>(v, ep);  // arrival: every peer's previous call is over
  tr.mark(2);
  const size_t poff = 0;        // single staging buffer (the arrival barrier guards reuse)
  char* mine = v.buf[me];
  const size_t nt = pad_tiles(c.bytes) / kTile;
  const size_t cpad = nt * kTile;

  switch (c.coll) {
    case IpcColl::BROADCAST_1SHOT: {
      if (me == c.root) stage_tiles((const char*)c.in[0], mine, c.bytes, b, G, nt);
      tr.mark(3);
      block_barrier(v, ph0);
      tr.mark(4);
      if (me == c.root) return;
      const OneSrcMap m{v.buf[c.root] + poff, (char*)c.out[0], c.bytes, b, G, nt};
      ipc_pipe<DType::U8, RedOp::COPY, 1, kCopyDepth>(lds, m, 1);
      return;
    }
    case IpcColl::BROADCAST_2SHOT: {
      // rows (t / W) belong to block row % G; tile t is owned by rank t % W
      if (me == c.root)
        for (int q = 0; q < W; ++q) stage_tiles((const char*)c.in[0], mine, c.bytes, q + W * b, W * G, nt);
      block_barrier(v, ph0);
      if (me != c.root) {  // phase 1: fetch my owned tiles from the root (one link each)
        const OneSrcMap m{v.buf[c.root] + poff, mine, cpad, me + W * b, W * G, nt};
        ipc_pipe<DType::U8, RedOp::COPY, 1, kCopyDepth>(lds, m, 1);
      }
      block_barrier(v, ph1);
      if (me == c.root) return;
      {  // phase 2: every owner's tiles, owners interleaved (all links at once)
        const OwnerRowMap<W> m{v.buf, poff, (char*)c.out[0], c.bytes, (uint32_t)(me + b), b, G, (nt + W - 1) / W};
        ipc_pipe<DType::U8, RedOp::COPY, 1, kCopyDepth>(lds, m, 1);
      }
      return;
    }
    case IpcColl::ALLGATHER:
    case IpcColl::GATHER: {
      stage_tiles((const char*)c.in[0], mine, c.bytes, b, G, nt);
      tr.mark(3);
      block_barrier(v, ph0);
      tr.mark(4);
      if (c.coll == IpcColl::GATHER && me != c.root) return;
      {
        const PeerTileMap<W> m{&v, &c, poff, c.bytes, (uint32_t)(me + b), b, G, nt};
        ipc_pipe<DType::U8, RedOp::COPY, 1, kCopyDepth>(lds, m, 1);
      }
      return;
    }
    case IpcColl::SCATTER: {
      if (me == c.root)
        for (int q = 0; q < W; ++q) stage_tiles((const char*)c.in[q], mine + q * cpad, c.bytes, b, G, nt);
      block_barrier(v, ph0);
      const OneSrcMap m{v.buf[c.root] + poff + me * cpad, (char*)c.out[0], c.bytes, b, G, nt};
      ipc_pipe<DType::U8, RedOp::COPY, 1, kCopyDepth>(lds, m, 1);
      return;
    }
    case IpcColl::ALLTOALL: {
      for (int q = 0; q < W; ++q) stage_tiles((const char*)c.in[q], mine + q * cpad, c.bytes, b, G, nt);
      block_barrier(v, ph0);
      {
        const PeerTileMap<W> m{&v, &c, poff + me * cpad, c.bytes, (uint32_t)(me + b), b, G, nt};
        ipc_pipe<DType::U8, RedOp::COPY, 1, kCopyDepth>(lds, m, 1);
      }
      return;
    }
    default:
      return;
  }
}

template <int W>
__global__ void __launch_bounds__(256) k_ipc_copy(IpcView v, IpcCall c) {
  __shared__ __attribute__((aligned(16))) char lds[PipeLds<1, kCopyDepth>::kBytes];
  __shared__ DView sv;
  __shared__ DCall sc;
  const uint32_t xb = xchg_blocks(c);
  PhaseTrace tr(v, xb);
  if (xb && blockIdx.x == 0) {  // the exchange block (see xchg_blocks)
    if (threadIdx.x < 64) zx_resolve(v, c, tr);
    tr.finish_exchange(v);
    zx_publish_verdict(c);
    return;
  }
  const uint32_t seq = block_seq(v, block_seq_load(v));  // (see k_ipc_reduce)
  stage_args(v, c, sv, sc, tr);  // (a gated zero-copy launch waits for its buffers here)
  if (c.gate) tr.mark(3);    // gate passed (zero-copy calls do not stage: [3] is free there)
  ipc_copy_body<W>(sv, sc, lds, tr, seq);
  tr.finish(v);
}

}  // namespace dev

// =============================================================== host entry points
namespace kern {

static hipError_t k1_dispatch(const void* const* srcs, int nsrc, void* out, size_t count, DType t, RedOp op,
                              int avg_div, hipStream_t stream, int max_blocks, int lds) {
  if (nsrc < 1 || nsrc > kMaxRanks || op == RedOp::COPY || !supports(t, op)) return hipErrorInvalidValue;
  canon(t, op);
  const size_t nbytes = count * dtype_size(t);
  if (nbytes == 0) return hipSuccess;
  const size_t tiles = nbytes / kTileBytes;
  // one workgroup per CU streams fastest with the strided tile map (measured: 256 > 512 > 1024)
  int grid = (int)std::min<size_t>(std::max<size_t>(tiles, 1), max_blocks > 0 ? (size_t)max_blocks : 256);
  using namespace dev;
  switch (t) {
#define PDCC_DT(DT) \
  case DType::DT: return k1_dispatch_##DT(srcs, nsrc, out, nbytes, op, avg_div, stream, grid, lds);
    PDCC_FOR_DTYPES(PDCC_DT)
#undef PDCC_DT
    default: return hipErrorInvalidValue;
  }
}

hipError_t reduce_nway(const void* const* srcs, int nsrc, void* out, size_t count, DType t, RedOp op, int avg_div,
                       hipStream_t stream, int max_blocks, bool nt) {
  return k1_dispatch(srcs, nsrc, out, count, t, op, avg_div, stream, max_blocks, 1 | (nt ? 2 : 0));
}
hipError_t reduce_nway_regs(const void* const* srcs, int nsrc, void* out, size_t count, DType t, RedOp op,
                            int avg_div, hipStream_t stream, int max_blocks, bool nt) {
  return k1_dispatch(srcs, nsrc, out, count, t, op, avg_div, stream, max_blocks, nt ? 2 : 0);
}
hipError_t reduce_nway_mode(const void* const* srcs, int nsrc, void* out, size_t count, DType t, RedOp op,
                            int avg_div, hipStream_t stream, int max_blocks, int mode) {
  if (mode < 0 || mode > 15) return hipErrorInvalidValue;
  return k1_dispatch(srcs, nsrc, out, count, t, op, avg_div, stream, max_blocks, mode);
}

// Default K2 grid from the launch's shape (scripts/k2_sweep.py on MI355X, profiles/README.md):
// small lists are latency-bound and want one tile per workgroup; big streams want few,
// long-running workgroups, and the fewer the larger the descriptors (each workgroup's
// strided tiles then stay within one DRAM-friendly window): 256 workgroups from 16 MiB
// per descriptor (8 x 32 MiB: 5.9 TB/s vs 4.9 at 1024), 512 below (64 x 4 MiB: 5.6 vs 5.1).
static int k2_grid(uint64_t tiles, int ndesc, size_t bytes) {
  if (tiles <= 4096) return (int)std::max<uint64_t>(1, std::min<uint64_t>(tiles, 2048));
  const size_t avg = bytes / (size_t)std::max(1, ndesc);
  return avg >= (16u << 20) ? 256 : 512;
}

// Non-temporal source loads by default for big lists of mid-size tensors (scripts/k2_sweep.py on
// MI355X, profiles/r3/k2_sweep_ntl_r3.json: 64 x 4 MiB 5.90 vs 5.45 TB/s, 8 x 32 MiB 5.85 vs 5.80);
// a wash or slightly worse for 128-256 MiB descriptors and for small lists.
static bool k2_ntl(size_t bytes, int ndesc) {
  return bytes >= (64u << 20) && bytes / (size_t)std::max(1, ndesc) <= (32u << 20);
}

hipError_t multi_copy(const CopyDesc* descs, int n, hipStream_t stream, int max_blocks, int depth, int ntl_mode) {
  if (depth <= 0) depth = kK2Depth;
  auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  for (int base = 0; base < n; base += kMaxCopyDescs) {
    dev::CopyArgs a{};
    const int m = std::min(kMaxCopyDescs, n - base);
    uint64_t acc = 0;
    size_t bytes = 0;
    for (int k = 0; k < m; ++k) {
      a.d[a.n] = descs[base + k];
      if (a.d[a.n].bytes == 0) continue;
      if (!aligned(a.d[a.n].src) || !aligned(a.d[a.n].dst)) {
        // the 16-B vector / LDS-DMA path needs aligned endpoints: DMA engine copy instead
        hipError_t e = hipMemcpyAsync(a.d[a.n].dst, a.d[a.n].src, a.d[a.n].bytes, hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
        continue;
      }
      a.prefix[a.n] = acc;
      acc += a.d[a.n].bytes / kTileBytes;
      if (a.d[a.n].bytes % kTileBytes) a.tail_idx[a.ntail++] = a.n;
      bytes += a.d[a.n].bytes;
      ++a.n;
    }
    if (a.n == 0) continue;
    a.prefix[a.n] = acc;
    const int cap = max_blocks > 0 ? max_blocks : k2_grid(acc, a.n, bytes);
    const bool ntl = ntl_mode < 0 ? k2_ntl(bytes, a.n) : ntl_mode > 0;
    const int grid =
        (int)std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint64_t>(acc, (uint64_t)a.ntail), (uint64_t)cap));
    if (depth >= 8) {
      if (ntl) hipLaunchKernelGGL((dev::k2_multi_copy<8, true>), dim3(grid), dim3(256), 0, stream, a);
      else hipLaunchKernelGGL((dev::k2_multi_copy<8, false>), dim3(grid), dim3(256), 0, stream, a);
    } else {
      if (ntl) hipLaunchKernelGGL((dev::k2_multi_copy<4, true>), dim3(grid), dim3(256), 0, stream, a);
      else hipLaunchKernelGGL((dev::k2_multi_copy<4, false>), dim3(grid), dim3(256), 0, stream, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// block-pairwise flags, the per-block call counters, the LL control words and LL slots
size_t ipc_signal_bytes() { return kDynOffset + kDynBytes; }

// plan (ipc_plan.h: every rejection, the grid, the canonical dtype and op), then one dispatch on
// (family, world[, dtype, op])
hipError_t ipc_launch(const IpcView& v, const IpcCall& call, hipStream_t stream) {
  const IpcPlan p = ipc_plan(v.world, call);
  if (p.err != hipSuccess) return p.err;
  IpcCall c = call;
  c.dtype = p.dtype;
  c.op = p.op;
  using namespace dev;
  if (coll_traits(c.coll).reducing) switch (p.dtype) {
#define PDCC_DT(DT) \
  case DType::DT: return ipc_dispatch_##DT(v, c, stream, p);
      PDCC_FOR_DTYPES(PDCC_DT)
#undef PDCC_DT
      default: return hipErrorInvalidValue;
    }
  return by_world(v.world, [&](auto w) {
    constexpr int W = decltype(w)::value;
    switch (p.family) {
      case Family::LL_ALLGATHER: return ipc_go(k_ll_allgather<W>, p.grid, stream, v, c);
      case Family::LL_ALLTOALL: return ipc_go(k_ll_alltoall<W>, p.grid, stream, v, c);
      case Family::LL_ROOTED: return ipc_go(k_ll_rooted<W>, p.grid, stream, v, c);
      default: return ipc_go(k_ipc_copy<W>, p.grid, stream, v, c);
    }
  });
}

}  // namespace kern
}  // namespace pdcc
