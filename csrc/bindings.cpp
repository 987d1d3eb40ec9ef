// Python bindings of the native library (module `_C` of the package).
//  * ProcessGroupMI355X  -- the c10d backend (subclass of torch's Backend type)
//  * kernel ops           -- K1 reduce_nway (LDS-DMA and register variants) and
//                            K2 multi_copy on torch tensors, on the current stream
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <pybind11/chrono.h>
#include <pybind11/stl.h>
#include <torch/csrc/utils/pybind.h>
#include <torch/python.h>

#include "backend/process_group.h"
#include "device/comm_util.h"
#include "kernels/kernel_api.h"
#include "kernels/mx_layout.h"
#include "kernels/mx_rot.h"

namespace py = pybind11;

namespace {

pdcc::kern::DType kdtype(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return pdcc::kern::DType::F32;
    case at::kHalf: return pdcc::kern::DType::F16;
    case at::kBFloat16: return pdcc::kern::DType::BF16;
    case at::kDouble: return pdcc::kern::DType::F64;
    case at::kChar: return pdcc::kern::DType::I8;
    case at::kByte: return pdcc::kern::DType::U8;
    case at::kInt: return pdcc::kern::DType::I32;
    case at::kLong: return pdcc::kern::DType::I64;
    case at::kBool: return pdcc::kern::DType::BOOL;
    case at::kFloat8_e4m3fn: return pdcc::kern::DType::F8E4M3;
    case at::kFloat8_e5m2: return pdcc::kern::DType::F8E5M2;
    default: TORCH_CHECK(false, "pdcc.ops: unsupported dtype ", t);
  }
}

pdcc::kern::RedOp kop(const std::string& s) {
  if (s == "sum") return pdcc::kern::RedOp::SUM;
  if (s == "avg") return pdcc::kern::RedOp::AVG;
  if (s == "prod" || s == "product") return pdcc::kern::RedOp::PROD;
  if (s == "min") return pdcc::kern::RedOp::MIN;
  if (s == "max") return pdcc::kern::RedOp::MAX;
  if (s == "band") return pdcc::kern::RedOp::BAND;
  if (s == "bor") return pdcc::kern::RedOp::BOR;
  if (s == "bxor") return pdcc::kern::RedOp::BXOR;
  TORCH_CHECK(false, "pdcc.ops: unknown reduce op '", s, "'");
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// mode: OR of kern::K1Mode bits (LDS-DMA engine, non-temporal stores, streaming kernel, non-temporal loads)
void reduce_nway(const std::vector<at::Tensor>& srcs, at::Tensor& out, const std::string& op, int mode,
                 int max_blocks) {
  TORCH_CHECK(!srcs.empty() && (int)srcs.size() <= pdcc::kern::kMaxRanks, "reduce_nway: 1..8 sources");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && al16(out.data_ptr()), "reduce_nway: out must be a contiguous, "
              "16-byte aligned GPU tensor");
  std::vector<const void*> p;
  for (const auto& s : srcs) {
    TORCH_CHECK(s.device() == out.device() && s.scalar_type() == out.scalar_type() && s.numel() == out.numel() &&
                    s.is_contiguous() && al16(s.data_ptr()),
                "reduce_nway: sources must match out (device, dtype, numel) and be contiguous + 16-byte aligned");
    p.push_back(s.data_ptr());
  }
  const auto k = kop(op);
  const auto d = kdtype(out.scalar_type());
  TORCH_CHECK(pdcc::kern::supports(d, k), "reduce_nway: op '", op, "' unsupported for ", out.scalar_type());
  c10::hip::HIPGuardMasqueradingAsCUDA g(out.device());
  hipStream_t s = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(out.device().index()).stream();
  hipError_t e = pdcc::kern::reduce_nway_mode(p.data(), (int)p.size(), out.data_ptr(), out.numel(), d, k,
                                               (int)srcs.size(), s, max_blocks, mode);
  TORCH_CHECK(e == hipSuccess, "reduce_nway launch failed: ", hipGetErrorString(e));
}

void multi_copy(const std::vector<at::Tensor>& srcs, const std::vector<at::Tensor>& dsts, int max_blocks, int depth,
                int ntl) {
  TORCH_CHECK(srcs.size() == dsts.size(), "multi_copy: list length mismatch");
  if (srcs.empty()) return;
  std::vector<pdcc::kern::CopyDesc> d;
  for (size_t i = 0; i < srcs.size(); ++i) {
    const auto& a = srcs[i];
    const auto& b = dsts[i];
    TORCH_CHECK(a.is_cuda() && b.device() == a.device(), "multi_copy: tensors must be on one GPU");
    TORCH_CHECK(a.nbytes() == b.nbytes(), "multi_copy: pair ", i, " size mismatch");
    TORCH_CHECK(a.is_contiguous() && b.is_contiguous(), "multi_copy: tensors must be contiguous");
    d.push_back({a.data_ptr(), b.data_ptr(), a.nbytes()});
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(srcs[0].device());
  hipStream_t s = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(srcs[0].device().index()).stream();
  hipError_t e = pdcc::kern::multi_copy(d.data(), (int)d.size(), s, max_blocks, depth, ntl);
  TORCH_CHECK(e == hipSuccess, "multi_copy launch failed: ", hipGetErrorString(e));
}

// ---- block-scaled wires, mxfp8_e4m3, mxfp4_e2m1 and mxfp6_e2m3 (kernels/mx_wire.hip). The kernels want contiguous, 16-byte aligned
// buffers: any other tensor goes through a contiguous copy (inputs) or is filled from one (outputs).
at::Tensor mx_in(const at::Tensor& t) {
  if (t.is_contiguous() && al16(t.data_ptr())) return t;
  at::Tensor c = at::empty_like(t, at::MemoryFormat::Contiguous);
  c.copy_(t);
  return c;
}
at::Tensor mx_out(const at::Tensor& t) {
  if (t.is_contiguous() && al16(t.data_ptr())) return t;
  return at::empty_like(t, at::MemoryFormat::Contiguous);
}
pdcc::kern::DType mx_dtype(const at::Tensor& t, const char* who) {
  TORCH_CHECK_TYPE(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf,
                   who, ": float32, bfloat16 or float16 tensors only, got ", t.scalar_type());
  return kdtype(t.scalar_type());
}
void mx_check_wire(const at::Tensor& w, const char* who) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kByte && w.dim() == 1, who, ": the wire is a 1-d uint8 GPU tensor");
}
// An error-feedback residual (docs/collectives.md "Error feedback") is updated in place, so it cannot
// go through a copy: float32, `numel` elements, contiguous, 16-byte aligned, on the data's GPU.
float* mx_residual(const c10::optional<at::Tensor>& r, int64_t numel, const at::Device& dev, const char* who) {
  if (!r) return nullptr;
  TORCH_CHECK_TYPE(r->scalar_type() == at::kFloat, who, ": the residual must be float32, got ", r->scalar_type());
  TORCH_CHECK_VALUE(r->numel() == numel, who, ": the residual has ", r->numel(), " elements, ", numel, " expected");
  TORCH_CHECK_VALUE(r->device() == dev, who, ": the residual is on ", r->device(), ", the data on ", dev);
  TORCH_CHECK_VALUE(r->is_contiguous(), who, ": the residual must be contiguous");
  TORCH_CHECK_VALUE(al16(r->data_ptr()), who, ": the residual must be 16-byte aligned");
  return r->data_ptr<float>();
}
// Stochastic rounding (docs/collectives.md "Stochastic rounding"): `sr` selects the kernels that round by the
// words of (seed, stream, element index); with a residual it is refused (the two are alternatives).
void mx_check_sr(bool sr, bool residual, int64_t stream, const char* who) {
  TORCH_CHECK_VALUE(!(sr && residual), who, ": stochastic rounding and a residual are alternatives");
  TORCH_CHECK_VALUE(stream >= 0 && stream <= 0xffffffffll, who, ": stream must be in [0, 2^32)");
}
// Hadamard rotation (docs/collectives.md "Hadamard rotation"): the sign word of `seed`, or none
struct MxRot {
  uint32_t signs = 0;
  bool on = false;
  MxRot(bool rot, uint64_t seed) : signs(rot ? pdcc::kern::mx_rot_signs(seed) : 0u), on(rot) {}
  const uint32_t* ptr() const { return on ? &signs : nullptr; }
};
using pdcc::kern::MxFormat;
MxFormat mx_format(const std::string& wire, const char* who) {
  if (wire == "mxfp8_e4m3") return MxFormat::FP8_E4M3;
  if (wire == "mxfp4_e2m1") return MxFormat::FP4_E2M1;
  if (wire == "mxfp6_e2m3") return MxFormat::FP6_E2M3;
  TORCH_CHECK_VALUE(false, who, ": unknown wire format '", wire, "' (supported: mxfp8_e4m3, mxfp4_e2m1, mxfp6_e2m3)");
  return MxFormat::FP8_E4M3;
}

at::Tensor mx_quantize(const at::Tensor& x, int world, const c10::optional<at::Tensor>& out, const std::string& fmt,
                       const c10::optional<at::Tensor>& residual, bool sr, uint64_t seed, int64_t sr_stream,
                       uint64_t index_offset, bool rot, uint64_t rot_seed) {
  const MxFormat f = mx_format(fmt, "mx_quantize");
  const MxRot rt(rot, rot_seed);
  mx_check_sr(sr, residual.has_value(), sr_stream, "mx_quantize");
  TORCH_CHECK(x.is_cuda(), "mx_quantize: GPU tensors only");
  TORCH_CHECK(world >= 1, "mx_quantize: world must be >= 1");
  const auto d = mx_dtype(x, "mx_quantize");
  const size_t numel = (size_t)x.numel();
  const size_t cb = pdcc::kern::mx_chunk_blocks(f, numel, world);
  const int64_t bytes = (int64_t)pdcc::kern::mx_wire_bytes(f, cb, (size_t)world);
  float* res = mx_residual(residual, x.numel(), x.device(), "mx_quantize");
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  at::Tensor wire = out ? *out : at::empty({bytes}, x.options().dtype(at::kByte));
  mx_check_wire(wire, "mx_quantize");
  TORCH_CHECK(wire.device() == x.device() && wire.numel() == bytes, "mx_quantize: out must hold ", bytes, " bytes on ",
              x.device());
  at::Tensor src = mx_in(x), w = mx_out(wire);
  hipStream_t s = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(x.device().index()).stream();
  hipError_t e = sr    ? pdcc::kern::mx_quantize_sr(src.data_ptr(), numel, d, w.data_ptr(), cb, (size_t)world, seed,
                                                    (uint32_t)sr_stream, index_offset, s, f, rt.ptr())
                 : res ? pdcc::kern::mx_quantize_ef(src.data_ptr(), numel, d, res, w.data_ptr(), cb, (size_t)world, s, f,
                                                    rt.ptr())
                       : pdcc::kern::mx_quantize(src.data_ptr(), numel, d, w.data_ptr(), cb, (size_t)world, s, f, rt.ptr());
  TORCH_CHECK(e == hipSuccess, "mx_quantize launch failed: ", hipGetErrorString(e));
  if (!w.is_same(wire)) wire.copy_(w);
  return wire;
}

at::Tensor mx_reduce(const at::Tensor& wire, int nsrc, const std::string& op, const c10::optional<at::Tensor>& out,
                     const std::string& fmt, const c10::optional<at::Tensor>& residual, bool sr, uint64_t seed,
                     int64_t sr_stream) {
  const MxFormat f = mx_format(fmt, "mx_reduce");
  mx_check_sr(sr, residual.has_value(), sr_stream, "mx_reduce");
  mx_check_wire(wire, "mx_reduce");
  TORCH_CHECK(nsrc >= 1 && nsrc <= pdcc::kern::kMaxRanks, "mx_reduce: 1..8 sources");
  TORCH_CHECK_VALUE(op == "sum" || op == "avg", "mx_reduce: op must be 'sum' or 'avg', got '", op, "'");
  const int64_t chunk = wire.numel() / nsrc;
  const int64_t bw = (int64_t)pdcc::kern::mx_block_wire(f);  // 33, 17 or 25
  TORCH_CHECK(chunk > 0 && chunk * nsrc == wire.numel() && chunk % (bw * 16) == 0, "mx_reduce: ", wire.numel(),
              " bytes are not ", nsrc, " chunk wires (", bw, " bytes per block, blocks in groups of 16)");
  const size_t cb = (size_t)(chunk / bw);
  float* r = mx_residual(residual, (int64_t)cb * pdcc::kern::kMxBlock, wire.device(), "mx_reduce");
  c10::hip::HIPGuardMasqueradingAsCUDA g(wire.device());
  at::Tensor res = out ? *out : at::empty({chunk}, wire.options());
  mx_check_wire(res, "mx_reduce");
  TORCH_CHECK(res.device() == wire.device() && res.numel() == chunk, "mx_reduce: out must hold ", chunk, " bytes");
  at::Tensor in = mx_in(wire), o = mx_out(res);
  hipStream_t s = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(wire.device().index()).stream();
  hipError_t e = sr  ? pdcc::kern::mx_reduce_sr(in.data_ptr(), nsrc, cb, kop(op), nsrc, o.data_ptr(), seed,
                                                (uint32_t)sr_stream, s, f)
                 : r ? pdcc::kern::mx_reduce_ef(in.data_ptr(), nsrc, cb, kop(op), nsrc, r, o.data_ptr(), s, f)
                     : pdcc::kern::mx_reduce(in.data_ptr(), nsrc, cb, kop(op), nsrc, o.data_ptr(), s, f);
  TORCH_CHECK(e == hipSuccess, "mx_reduce launch failed: ", hipGetErrorString(e));
  if (!o.is_same(res)) res.copy_(o);
  return res;
}

void mx_dequantize(const at::Tensor& wire, int world, at::Tensor& out, const std::string& fmt, bool rot,
                   uint64_t rot_seed) {
  const MxFormat f = mx_format(fmt, "mx_dequantize");
  const MxRot rt(rot, rot_seed);
  mx_check_wire(wire, "mx_dequantize");
  TORCH_CHECK(world >= 1, "mx_dequantize: world must be >= 1");
  TORCH_CHECK(out.is_cuda() && out.device() == wire.device(), "mx_dequantize: out must be on the wire's GPU");
  const auto d = mx_dtype(out, "mx_dequantize");
  const size_t numel = (size_t)out.numel();
  const size_t cb = pdcc::kern::mx_chunk_blocks(f, numel, world);
  TORCH_CHECK((size_t)wire.numel() == pdcc::kern::mx_wire_bytes(f, cb, (size_t)world), "mx_dequantize: the wire of ",
              numel, " elements in ", world, " chunks has ", pdcc::kern::mx_wire_bytes(f, cb, (size_t)world),
              " bytes, got ", wire.numel());
  c10::hip::HIPGuardMasqueradingAsCUDA g(wire.device());
  at::Tensor w = mx_in(wire), o = mx_out(out);
  hipStream_t s = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(wire.device().index()).stream();
  hipError_t e = pdcc::kern::mx_dequantize(w.data_ptr(), cb, (size_t)world, o.data_ptr(), numel, d, s, f, rt.ptr());
  TORCH_CHECK(e == hipSuccess, "mx_dequantize launch failed: ", hipGetErrorString(e));
  if (!o.is_same(out)) out.copy_(o);
}

// ---- the shard layout (kernels/mx_layout.h): chunk r is shard r of `numel / world` elements
at::Tensor mx_quantize_shards(const at::Tensor& x, int world, const c10::optional<at::Tensor>& out,
                              const std::string& fmt, const c10::optional<at::Tensor>& residual, bool sr, uint64_t seed,
                              int64_t sr_stream, uint64_t index_offset, bool rot, uint64_t rot_seed) {
  const MxFormat f = mx_format(fmt, "mx_quantize_shards");
  const MxRot rt(rot, rot_seed);
  mx_check_sr(sr, residual.has_value(), sr_stream, "mx_quantize_shards");
  TORCH_CHECK(x.is_cuda(), "mx_quantize_shards: GPU tensors only");
  TORCH_CHECK(world >= 1 && world <= 65535, "mx_quantize_shards: world must be 1..65535");
  const auto d = mx_dtype(x, "mx_quantize_shards");
  TORCH_CHECK_VALUE(x.numel() > 0 && x.numel() % world == 0, "mx_quantize_shards: ", x.numel(),
                    " elements are not ", world, " shards of one or more elements");
  const size_t m = (size_t)x.numel() / (size_t)world;
  const size_t cb = pdcc::kern::mx_shard_blocks(f, m);
  const int64_t bytes = (int64_t)pdcc::kern::mx_shard_wire_bytes(f, m, (size_t)world);
  float* res = mx_residual(residual, x.numel(), x.device(), "mx_quantize_shards");
  c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
  at::Tensor wire = out ? *out : at::empty({bytes}, x.options().dtype(at::kByte));
  mx_check_wire(wire, "mx_quantize_shards");
  TORCH_CHECK(wire.device() == x.device() && wire.numel() == bytes, "mx_quantize_shards: out must hold ", bytes,
              " bytes on ", x.device());
  at::Tensor src = mx_in(x), w = mx_out(wire);
  hipStream_t s = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(x.device().index()).stream();
  hipError_t e = sr    ? pdcc::kern::mx_quantize_shards_sr(src.data_ptr(), m, d, w.data_ptr(), cb, (size_t)world, seed,
                                                           (uint32_t)sr_stream, index_offset, s, f, rt.ptr())
                 : res ? pdcc::kern::mx_quantize_shards_ef(src.data_ptr(), m, d, res, w.data_ptr(), cb, (size_t)world, s, f,
                                                           rt.ptr())
                       : pdcc::kern::mx_quantize_shards(src.data_ptr(), m, d, w.data_ptr(), cb, (size_t)world, s, f,
                                                        rt.ptr());
  TORCH_CHECK(e == hipSuccess, "mx_quantize_shards launch failed: ", hipGetErrorString(e));
  if (!w.is_same(wire)) wire.copy_(w);
  return wire;
}

void mx_dequantize_shards(const at::Tensor& wire, int world, at::Tensor& out, const std::string& fmt, bool rot,
                          uint64_t rot_seed) {
  const MxFormat f = mx_format(fmt, "mx_dequantize_shards");
  const MxRot rt(rot, rot_seed);
  mx_check_wire(wire, "mx_dequantize_shards");
  TORCH_CHECK(world >= 1 && world <= 65535, "mx_dequantize_shards: world must be 1..65535");
  TORCH_CHECK(out.is_cuda() && out.device() == wire.device(), "mx_dequantize_shards: out must be on the wire's GPU");
  const auto d = mx_dtype(out, "mx_dequantize_shards");
  TORCH_CHECK_VALUE(out.numel() > 0 && out.numel() % world == 0, "mx_dequantize_shards: ", out.numel(),
                    " elements are not ", world, " shards of one or more elements");
  const size_t m = (size_t)out.numel() / (size_t)world;
  const size_t cb = pdcc::kern::mx_shard_blocks(f, m);
  const size_t bytes = pdcc::kern::mx_shard_wire_bytes(f, m, (size_t)world);
  TORCH_CHECK((size_t)wire.numel() == bytes, "mx_dequantize_shards: the wire of ", world, " shards of ", m,
              " elements has ", bytes, " bytes, got ", wire.numel());
  c10::hip::HIPGuardMasqueradingAsCUDA g(wire.device());
  at::Tensor w = mx_in(wire), o = mx_out(out);
  hipStream_t s = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(wire.device().index()).stream();
  hipError_t e = pdcc::kern::mx_dequantize_shards(w.data_ptr(), cb, (size_t)world, o.data_ptr(), m, d, s, f, rt.ptr());
  TORCH_CHECK(e == hipSuccess, "mx_dequantize_shards launch failed: ", hipGetErrorString(e));
  if (!o.is_same(out)) out.copy_(o);
}

void mx_fold(const at::Tensor& wire, int nsrc, const std::string& op, at::Tensor& out, const std::string& fmt, bool rot,
             uint64_t rot_seed) {
  const MxFormat f = mx_format(fmt, "mx_fold");
  const MxRot rt(rot, rot_seed);
  mx_check_wire(wire, "mx_fold");
  TORCH_CHECK(nsrc >= 1 && nsrc <= pdcc::kern::kMaxRanks, "mx_fold: 1..8 sources");
  TORCH_CHECK_VALUE(op == "sum" || op == "avg", "mx_fold: op must be 'sum' or 'avg', got '", op, "'");
  TORCH_CHECK(out.is_cuda() && out.device() == wire.device(), "mx_fold: out must be on the wire's GPU");
  const auto d = mx_dtype(out, "mx_fold");
  TORCH_CHECK_VALUE(out.numel() > 0, "mx_fold: out has no elements");
  const size_t numel = (size_t)out.numel();
  const size_t cb = pdcc::kern::mx_shard_blocks(f, numel);
  const size_t bytes = pdcc::kern::mx_wire_bytes(f, cb, (size_t)nsrc);
  TORCH_CHECK((size_t)wire.numel() == bytes, "mx_fold: ", nsrc, " chunk wires of ", numel, " elements have ", bytes,
              " bytes, got ", wire.numel());
  c10::hip::HIPGuardMasqueradingAsCUDA g(wire.device());
  at::Tensor w = mx_in(wire), o = mx_out(out);
  hipStream_t s = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(wire.device().index()).stream();
  hipError_t e = pdcc::kern::mx_fold(w.data_ptr(), nsrc, cb, kop(op), nsrc, o.data_ptr(), numel, d, s, f, rt.ptr());
  TORCH_CHECK(e == hipSuccess, "mx_fold launch failed: ", hipGetErrorString(e));
  if (!o.is_same(out)) out.copy_(o);
}

// Peer links between every pair of visible GPUs, as the runtime reports them: HSA link
// type (xGMI on an MI355X node, PCIe otherwise), hop count, P2P access / atomics and
// the runtime's relative performance rank. Local queries only (no collective).
py::list device_links() {
  static const char* kLink[] = {"hypertransport", "qpi", "pcie", "infiniband", "xgmi"};
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  py::list out;
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) {
      if (a == b) continue;
      py::dict d;
      d["src"] = a;
      d["dst"] = b;
      uint32_t type = 0, hops = 0;
      if (hipExtGetLinkTypeAndHopCount(a, b, &type, &hops) == hipSuccess) {
        d["link"] = type < 5 ? std::string(kLink[type]) : std::to_string(type);
        d["hops"] = hops;
      } else {
        (void)hipGetLastError();
        d["link"] = "unknown";
      }
      int v = 0;
      if (hipDeviceGetP2PAttribute(&v, hipDevP2PAttrAccessSupported, a, b) == hipSuccess) d["p2p"] = v;
      if (hipDeviceGetP2PAttribute(&v, hipDevP2PAttrNativeAtomicSupported, a, b) == hipSuccess) d["atomics"] = v;
      if (hipDeviceGetP2PAttribute(&v, hipDevP2PAttrPerformanceRank, a, b) == hipSuccess) d["perf_rank"] = v;
      (void)hipGetLastError();
      out.append(d);
    }
  return out;
}

}  // namespace

PYBIND11_MODULE(_C, m) {
  m.doc() = "MI355X-native collective communication backend (c10d) and gfx950 kernels";
  py::module::import("torch.distributed");  // registers c10d::Backend / Store with pybind

  py::class_<pdcc::ProcessGroupMI355X, c10d::Backend, c10::intrusive_ptr<pdcc::ProcessGroupMI355X>>(
      m, "ProcessGroupMI355X")
      .def(py::init([](const c10::intrusive_ptr<c10d::Store>& store, int rank, int size,
                       std::chrono::milliseconds timeout, std::vector<int64_t> ranks, std::string name) {
             return c10::make_intrusive<pdcc::ProcessGroupMI355X>(store, rank, size, timeout, std::move(ranks),
                                                                  std::move(name));
           }),
           py::arg("store"), py::arg("rank"), py::arg("size"), py::arg("timeout"),
           py::arg("global_ranks") = std::vector<int64_t>{}, py::arg("group_name") = std::string(""),
           py::call_guard<py::gil_scoped_release>())
      .def("stats",
           [](pdcc::ProcessGroupMI355X& pg) {
             std::map<std::string, pdcc::OpStats> st;
             {  // (may wait for pending zero-copy outcomes)
               py::gil_scoped_release nogil;
               st = pg.stats();
             }
             py::dict d;
             for (const auto& kv : st)
               d[py::str(kv.first)] = py::make_tuple(kv.second.calls, kv.second.bytes, kv.second.host_ms);
             return d;
           })
      .def("autotune_table",
           [](pdcc::ProcessGroupMI355X& pg) {
             py::list l;
             for (const auto& r : pg.autotune_table()) {
               py::dict d;
               d["coll"] = r.coll;
               d["dtype"] = r.dtype;
               d["op"] = r.op;
               d["lo"] = r.lo;
               d["hi"] = r.hi;
               d["ref"] = r.ref;
               d["ref_us"] = r.rccl_us;
               d["ipc_us"] = r.ipc_us;
               d["push_us"] = r.push_us;
               d["dyn_us"] = r.dyn_us;
               d["sdma_us"] = r.sdma_us;
               d["wide_us"] = r.wide_us;
               d["ipc_wide_us"] = r.ipc_wide_us;
               d["staged_us"] = r.staged_us;
               d["ipc_valid"] = r.valid;
               d["algo"] = r.algo;
               d["iters"] = r.iters;
               d["async_capped"] = r.async_capped;
               l.append(d);
             }
             return l;
           })
      .def("flight_recorder",
           [](pdcc::ProcessGroupMI355X& pg) {
             py::list l;
             for (const auto& r : pg.flight_recorder()) {
               py::dict d;
               d["seq"] = r.seq;
               d["op"] = r.what;
               d["bytes"] = r.bytes;
               d["t_ms"] = r.t_ms;
               d["state"] = r.state;
               l.append(d);
             }
             return l;
           })
      .def("flight_recorder_dump", &pdcc::ProcessGroupMI355X::flight_recorder_dump, py::arg("last") = 16)
      .def("reset_stats", &pdcc::ProcessGroupMI355X::reset_stats)
      .def("describe", &pdcc::ProcessGroupMI355X::describe)
      .def("timeout_ms", &pdcc::ProcessGroupMI355X::timeout_ms)
      .def("last_algo", &pdcc::ProcessGroupMI355X::last_algo, py::call_guard<py::gil_scoped_release>())
      .def("zc_counters", &pdcc::ProcessGroupMI355X::zc_counters, py::call_guard<py::gil_scoped_release>())
      .def("healthy", &pdcc::ProcessGroupMI355X::healthy)
      .def("health_message", &pdcc::ProcessGroupMI355X::health_message)
      .def("set_algo", &pdcc::ProcessGroupMI355X::set_algo)
      .def("host_profile",
           [](pdcc::ProcessGroupMI355X& pg) {
             py::dict d;
             for (const auto& r : pg.host_profile())
               d[py::str(std::get<0>(r))] = py::make_tuple(std::get<1>(r), std::get<2>(r));
             return d;
           },
           "PDCC_HOST_PROF / set_host_profile(True): {stage: (calls, total_us)} of the GPU all_reduce host path")
      .def("set_host_profile", &pdcc::ProcessGroupMI355X::set_host_profile, py::arg("on"))
      .def("set_ipc_thresholds", &pdcc::ProcessGroupMI355X::set_ipc_thresholds, py::arg("one_shot_max") = -1,
           py::arg("two_shot_max") = -1, py::arg("copy_max") = -1)
      .def("abort_group", &pdcc::ProcessGroupMI355X::abort_group, py::call_guard<py::gil_scoped_release>())
      .def("ipc_trace", &pdcc::ProcessGroupMI355X::ipc_trace,
           "PDCC_IPC_TRACE records: [seq, t_entry, t_seq, t_staged, t_barrier0, t_phase1, t_barrier1, t_exit] "
           "in 100 MHz device ticks, block 0 of each IPC kernel (words 8-11: zero-copy exchange, 12-15: call number "
           "and zero-copy arrival barrier), then per block b < 256: [16 + b] phase 1 done, [272 + b] exit")
      .def("eager_init", &pdcc::ProcessGroupMI355X::eager_init, py::arg("device"),
           py::call_guard<py::gil_scoped_release>())
      // torch calls this on non-member ranks of a new group when the default group is bound
      // to a device (see supportsSplitting in process_group.h): nothing to do here
      .def("perform_nocolor_split", [](pdcc::ProcessGroupMI355X&, const at::Device&) {});

  // the cross-stream issue order of one RCCL communicator (csrc/device/issue_order.h), exposed
  // for tests: dry=True logs the stream operations instead of issuing them (no GPU needed)
  py::class_<pdcc::IssueOrder>(m, "IssueOrder")
      .def(py::init<bool>(), py::arg("dry") = false)
      .def("enter", [](pdcc::IssueOrder& o, uintptr_t s) { o.enter(reinterpret_cast<hipStream_t>(s)); })
      .def("leave", [](pdcc::IssueOrder& o, uintptr_t s) { o.leave(reinterpret_cast<hipStream_t>(s)); })
      .def("add_user", &pdcc::IssueOrder::add_user)
      .def("users", &pdcc::IssueOrder::users)
      .def("ticks", &pdcc::IssueOrder::ticks)
      .def("waits", &pdcc::IssueOrder::waits)
      .def("log", &pdcc::IssueOrder::log);

  m.def("reduce_nway", &reduce_nway, py::arg("srcs"), py::arg("out"), py::arg("op") = "sum",
        py::arg("mode") = 1, py::arg("max_blocks") = 0,
        "K1: out = op(srcs...) on the current stream (mode: 1 LDS-DMA engine | 2 non-temporal stores | "
        "4 streaming kernel | 8 non-temporal loads)");
  m.def("multi_copy", &multi_copy, py::arg("srcs"), py::arg("dsts"), py::arg("max_blocks") = 0, py::arg("depth") = 0,
        py::arg("ntl") = -1,
        "K2: one-launch multi-tensor copy (max_blocks/depth 0 = defaults)");
  m.def("mx_quantize", &mx_quantize, py::arg("x"), py::arg("world") = 1, py::arg("out") = py::none(),
        py::arg("fmt") = "mxfp8_e4m3", py::arg("residual") = py::none(), py::arg("sr") = false, py::arg("seed") = 0,
        py::arg("stream") = 0, py::arg("index_offset") = 0, py::arg("rot") = false, py::arg("rot_seed") = 0,
        "tensor (f32 / bf16 / f16) -> mxfp8_e4m3 / mxfp4_e2m1 / mxfp6_e2m3 wire of `world` chunks, on the current stream; "
        "`residual`: one float per element of error feedback, added before and updated in place; `sr`: stochastic "
        "rounding by the words of (seed, stream, index_offset + element index); `rot`: every block rotated with the "
        "sign word of `rot_seed` first (Hadamard rotation)");
  m.def("mx_reduce", &mx_reduce, py::arg("wire"), py::arg("nsrc"), py::arg("op") = "sum", py::arg("out") = py::none(),
        py::arg("fmt") = "mxfp8_e4m3", py::arg("residual") = py::none(), py::arg("sr") = false, py::arg("seed") = 0,
        py::arg("stream") = 0,
        "nsrc chunk wires back to back -> one chunk wire (dequantize, fold in f32 in source order, requantize); "
        "`residual`: 32 cb floats of error feedback, updated in place; `sr`: stochastic requantization by the "
        "words of (seed, stream, index in the chunk)");
  m.def("mx_dequantize", &mx_dequantize, py::arg("wire"), py::arg("world"), py::arg("out"),
        py::arg("fmt") = "mxfp8_e4m3", py::arg("rot") = false, py::arg("rot_seed") = 0,
        "mxfp8_e4m3 / mxfp4_e2m1 / mxfp6_e2m3 wire of `world` chunks -> out (f32 / bf16 / f16), exactly out.numel() elements; "
        "`rot`: every block rotated back with the sign word of `rot_seed`");
  m.def("mx_quantize_shards", &mx_quantize_shards, py::arg("x"), py::arg("world"), py::arg("out") = py::none(),
        py::arg("fmt") = "mxfp8_e4m3", py::arg("residual") = py::none(), py::arg("sr") = false, py::arg("seed") = 0,
        py::arg("stream") = 0, py::arg("index_offset") = 0, py::arg("rot") = false, py::arg("rot_seed") = 0,
        "tensor of `world` shards -> shard wire: chunk r is the wire of shard r alone; `residual`, `sr` and `rot` as in "
        "mx_quantize");
  m.def("mx_dequantize_shards", &mx_dequantize_shards, py::arg("wire"), py::arg("world"), py::arg("out"),
        py::arg("fmt") = "mxfp8_e4m3", py::arg("rot") = false, py::arg("rot_seed") = 0,
        "shard wire of `world` chunks -> out: chunk r fills out[r m, (r + 1) m), m = out.numel() / world; `rot` as in "
        "mx_dequantize");
  m.def("mx_fold", &mx_fold, py::arg("wire"), py::arg("nsrc"), py::arg("op"), py::arg("out"),
        py::arg("fmt") = "mxfp8_e4m3", py::arg("rot") = false, py::arg("rot_seed") = 0,
        "nsrc chunk wires of out.numel() elements -> out (dequantize, fold in f32 in source order, round once); `rot`: "
        "the fold rotated back before it is rounded");
  m.def("mx_rotation_signs", [](uint64_t seed) { return pdcc::kern::mx_rot_signs(seed); }, py::arg("seed"),
        "the sign word of a Hadamard rotation seed (kernels/mx_rot.h)");
  m.def("mx_shard_blocks", [](int64_t m, const std::string& fmt) {
    return (int64_t)pdcc::kern::mx_shard_blocks(mx_format(fmt, "mx_shard_blocks"), (size_t)m);
  }, py::arg("m"), py::arg("fmt") = "mxfp8_e4m3");
  m.def("mx_chunk_blocks", [](int64_t numel, int world, const std::string& fmt) {
    return (int64_t)pdcc::kern::mx_chunk_blocks(mx_format(fmt, "mx_chunk_blocks"), (size_t)numel, world);
  }, py::arg("numel"), py::arg("world"), py::arg("fmt") = "mxfp8_e4m3");
  m.def("ipc_signal_bytes", &pdcc::kern::ipc_signal_bytes);
  m.def("device_links", &device_links,
        "peer links between every pair of visible GPUs: link type (xgmi/pcie), hops, p2p, atomics, perf_rank");
  m.def("forwarded_rccl_env", &pdcc::forward_rccl_env,
        "NCCL_* variables set from PDCC_RCCL_* before the first communicator (once per process)");
  m.attr("MAX_RANKS_IPC") = pdcc::kern::kMaxRanks;
  m.attr("TILE_BYTES") = pdcc::kern::kTileBytes;
}
