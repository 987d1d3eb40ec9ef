// GPU data paths of ProcessGroupMI355X.
//
// Every collective runs on the caller's stream (synchronous ops) or on a
// per-device comm stream that first waits for the caller's stream (async ops),
// exactly like the reference's sync `dist.*` calls appear to the user
// (main.py:14-83) but without blocking the host. Per call one of three engines:
//   IPC  -- csrc/kernels: stage into own registered buffer, flag peers, pull or
//           reduce straight from every peer's buffer over xGMI (1-/2-shot)
//   RCCL -- ncclAllReduce/Reduce/Broadcast/AllGather/ReduceScatter/AllToAll and
//           grouped ncclSend/Recv (gather/scatter/list all-gather/uneven
//           all-to-all straight into the caller's list tensors)
//   HOST -- D2H, the shared-memory host transport, H2D (fallback only)
// Which one: a static size threshold (config.h) until the online autotuner has
// timed both feasible engines for the call's (collective, dtype, op, size
// bucket) on this very node; from then on the measured winner.
#include "gpu_util.h"

namespace pdcc {

using namespace gpu;

// a call whose IPC engine is an LL kernel (whatever engine the autotuner then picks, every one of them
// takes buffers at any alignment: LL, RCCL, the host path)
bool ProcessGroupMI355X::ll_call(const DeviceState& ds, size_t bytes) const {
  return ds.ipc_ok && ll_size(ds, bytes);
}

bool ProcessGroupMI355X::bytes_in_ll_range(size_t bytes) const {
  return bytes > 0 && bytes <= std::min(cfg_.ipc_ll_max, kern::kLLMaxBytes);
}

Algo ProcessGroupMI355X::choose(Coll c, size_t bytes, DeviceState& ds, bool rccl_can, bool ipc_can) {
  const Algo a = [&] {
    if (cfg_.force_algo == Algo::HOST) return Algo::HOST;
    if (cfg_.force_algo == Algo::RCCL && rccl_can) return Algo::RCCL;
    if (cfg_.force_algo == Algo::RCCL_WIDE && rccl_can)  // only all_reduce races the wide communicator
      return c == Coll::ALLREDUCE ? Algo::RCCL_WIDE : Algo::RCCL;
    if (cfg_.force_algo == Algo::IPC && ipc_can) return Algo::IPC;
    if (cfg_.force_algo == Algo::IPC_PUSH && ipc_can)  // only all_reduce has a push protocol
      return c == Coll::ALLREDUCE && ds.zc_ok ? Algo::IPC_PUSH : Algo::IPC;
    if (cfg_.force_algo == Algo::IPC_WIDE && ipc_can)  // only all_reduce races the wide grid
      return c == Coll::ALLREDUCE ? Algo::IPC_WIDE : Algo::IPC;
    if (cfg_.force_algo == Algo::IPC_DYN && ipc_can)  // the zero-copy all_reduce / all_gather / reduce_scatter
      return (c == Coll::ALLREDUCE || c == Coll::ALLGATHER || c == Coll::REDUCE_SCATTER) && ds.zc_ok
                 ? Algo::IPC_DYN
                 : Algo::IPC;
    if (cfg_.force_algo == Algo::IPC_STAGED && ipc_can) return Algo::IPC_STAGED;
    if (cfg_.force_algo == Algo::IPC_SDMA && ipc_can)  // the copy collectives (the others: the IPC kernels)
      return (c == Coll::BROADCAST || c == Coll::ALLGATHER || c == Coll::GATHER || c == Coll::SCATTER ||
              c == Coll::ALLTOALL) && ds.zc_ok
                 ? Algo::IPC_SDMA
                 : Algo::IPC;
    if (ipc_can) {
      size_t lim = cfg_.ipc_copy_max;
      if (c == Coll::ALLREDUCE || c == Coll::REDUCE || c == Coll::BROADCAST) lim = cfg_.ipc_2shot_max;
      if (bytes <= lim) return Algo::IPC;
    }
    if (rccl_can) return Algo::RCCL;
    if (ipc_can) return Algo::IPC;
    return Algo::HOST;
  }();
  TORCH_CHECK(a != Algo::HOST || !capturing_on(ds.device), "pdcc: this ", coll_name(c), " (", bytes,
              " B) would run on the host-staged engine, which cannot be captured into a graph");
  return a;
}

void ProcessGroupMI355X::ipc_chunked(IpcComm& ic, kern::IpcCall call, size_t per_call_max, hipStream_t s) {
  // whole rows of `size_` tiles per chunk: 2-shot staging is sized to whole rows
  const size_t row = (size_t)size_ * kern::kTileBytes;
  size_t chunk = per_call_max / row * row;
  if (chunk == 0) chunk = row;
  const size_t total = call.bytes;
  if (total <= chunk) {
    ic.launch(call, s);
    return;
  }
  for (size_t off = 0; off < total; off += chunk) {
    kern::IpcCall c = call;
    c.bytes = std::min(chunk, total - off);
    for (int k = 0; k < kern::kMaxRanks; ++k) {
      if (call.in[k]) c.in[k] = static_cast<const char*>(call.in[k]) + off;
      if (call.out[k]) c.out[k] = static_cast<char*>(call.out[k]) + off;
    }
    ic.launch(c, s);
  }
}

// Zero-copy IPC. Every step depends on group-wide facts or on the exchanged records
// only, so all ranks take the same branch: the records go round the host transport
// (a few us), a second round only when some rank exported an allocation its peers
// have not mapped yet (agreeing that every mapping worked).
bool ProcessGroupMI355X::zc_map(DeviceState& ds, const void* zbuf, size_t zlen, bool cap, const char* selftest,
                                std::vector<char*>& ptrs) {
  IpcComm& ic = ds.ipc ? *ds.ipc : ipc(ds);
  const IpcComm::ZcRec mine = ic.zc_export(zbuf, zlen, cap);
  std::vector<IpcComm::ZcRec> all(size_);
  if (selftest) {  // init_mu_ is held: exchange through the store, not the host transport
    const auto v = store_allgather(store_, std::string(selftest) + "/rec", rank_, size_,
                                   std::vector<uint8_t>(reinterpret_cast<const uint8_t*>(&mine),
                                                        reinterpret_cast<const uint8_t*>(&mine) + sizeof(mine)));
    for (int r = 0; r < size_; ++r) {
      TORCH_CHECK(v[r].size() == sizeof(IpcComm::ZcRec), "pdcc: malformed zero-copy record");
      std::memcpy(&all[r], v[r].data(), sizeof(IpcComm::ZcRec));
    }
  } else {  // (a launcher job exchanges on the launcher's own channel)
    std::vector<void*> outs;
    for (auto& r : all) outs.push_back(&r);
    (cfg_.ipc_zc_async ? exchange_channel(ds) : shm()).allgather(&mine, outs, sizeof(mine), timeout_);
  }
  bool all_ok = true, fresh = false;
  for (const auto& r : all) {
    all_ok = all_ok && r.ok;
    fresh = fresh || r.fresh;
  }
  bool ok = ic.zc_import(all, zbuf, all_ok, ptrs);
  if (all_ok && fresh) {
    if (selftest) {
      const auto v = store_allgather(store_, std::string(selftest) + "/mapped", rank_, size_,
                                     std::vector<uint8_t>{(uint8_t)ok});
      for (const auto& x : v) ok = ok && !x.empty() && x[0] == 1;
    } else {
      double f = ok ? 1.0 : 0.0;
      (cfg_.ipc_zc_async ? exchange_channel(ds) : shm()).allreduce(&f, 1, at::kDouble, RedOpType::MIN, timeout_);
      ok = f > 0.0;
    }
  }
  ok = ok && all_ok;
  ic.zc_settle(mine, ok);
  return ok;
}

size_t ProcessGroupMI355X::ipc_zero_copy(DeviceState& ds, kern::IpcCall call, const void* zbuf, size_t zlen,
                                         size_t unit, hipStream_t s, const char* selftest) {
  if (!selftest && (staged_only_ || !ds.zc_ok || !cfg_.ipc_zc || call.bytes < cfg_.ipc_zc_min)) return 0;
  const size_t body = call.bytes / unit * unit;
  if (body == 0) return 0;
  IpcComm& ic = ds.ipc ? *ds.ipc : ipc(ds);
  std::vector<char*> ptrs;
  if (!zc_map(ds, zbuf, zlen, capturing(s), selftest, ptrs)) return 0;
  if (kern::coll_traits(call.coll).zc_stages) {
    // the rooted reduce stages its reduced tiles, the push all-reduce receives its owned
    // tiles in staging: chunks of at most the staging cap
    const size_t chunk = std::max(unit, ic.chunk_cap() / unit * unit);
    for (size_t off = 0; off < body; off += chunk) {
      kern::IpcCall c = call;
      c.bytes = std::min(chunk, body - off);
      std::vector<char*> p = ptrs;
      for (auto& q : p)
        if (q) q += off;
      ic.launch_zc(c, p, s);
    }
    return body;
  }
  call.bytes = body;
  ic.launch_zc(call, ptrs, s);
  return body;
}

void ProcessGroupMI355X::ipc_run(DeviceState& ds, kern::IpcCall call, const void* zbuf, size_t zlen, size_t unit,
                                 size_t per_call_max, hipStream_t s, const char* selftest) {
  size_t body = 0;
  // (the same conditions ipc_zero_copy applies: a call below them is staged by design, not a fallback)
  const bool attempt = !selftest && !staged_only_ && ds.zc_ok && cfg_.ipc_zc && call.bytes >= cfg_.ipc_zc_min &&
                       call.bytes / unit > 0;
  ZcPart part;
  if (attempt && cfg_.ipc_zc_async && !capturing(s)) {
    // gated launches now, the exchange on the exchange thread (launcher.cpp); whether they ran
    // zero-copy or staged is known once the exchange has run (the part stays pending until then)
    body = call.bytes / unit * unit;
    part.ticket = ipc_gated(ds, call, zbuf, zlen, unit, body, per_call_max, s);
    part.launcher = ds.launcher.get();
  } else {
    if (!selftest) launcher_quiesce(ds);  // inline exchange: the channel is this thread's now
    body = ipc_zero_copy(ds, call, zbuf, zlen, unit, s, selftest);
    part.state = body > 0 ? 1 : 0;
  }
  if (attempt) {  // the op's engine label is settled from the outcome (record())
    std::lock_guard<std::mutex> lk(stats_mu_);
    zc_parts_.push_back(part);
  }
  if (body == call.bytes) return;
  kern::IpcCall rest = call;
  rest.coll = kern::staged_twin(rest.coll);  // (a zero-copy-only protocol)
  rest.dyn = 0;                              // (likewise)
  rest.bytes = call.bytes - body;
  for (int k = 0; k < kern::kMaxRanks; ++k) {
    if (call.in[k]) rest.in[k] = static_cast<const char*>(call.in[k]) + body;
    if (call.out[k]) rest.out[k] = static_cast<char*>(call.out[k]) + body;
  }
  const kern::IpcColl one_shot = kern::coll_traits(rest.coll).one_shot;
  if (body && rest.bytes <= cfg_.ipc_1shot_max && one_shot != kern::IpcColl::kCount)
    rest.coll = one_shot;  // the rest of a zero-copy 2-shot is short
  ipc_chunked(ipc(ds), rest, per_call_max, s);
}

// Copy-engine engine (verdict r5 Next #4, SURVEY §2.4 K3 "compare with hipMemcpyPeerAsync"). The copy
// collectives (reference main.py:37,52,68,81; the ZeRO parameter gather README.md:254 motivates) move
// their bytes with hipMemcpyAsync between IPC-mapped user buffers: the runtime's copy engines do the
// work, so a gather overlapped with GEMMs leaves every CU to them. Pull only -- every byte lands in
// memory of the GPU that issued its copy, which HIP's stream semantics then make visible to this
// rank's later kernels (no cross-GPU cache maintenance of remote writes to reason about). Order:
// the exchange (this thread, like an inline zero-copy call), a flags-only barrier launch (every
// peer's earlier kernels -- the writes of what is read here -- have finished), the pulls fanned out
// over up to PDCC_SDMA_STREAMS side streams (one stream's copies run in order), a second barrier
// launch (no peer reads this rank's buffer any more once it passes), the mappings kept open until
// that launch is done. Both barriers are single-workgroup IPC launches: every rank issues the same
// IPC sequence, so the per-block call numbers stay in step with the other engines.
bool ProcessGroupMI355X::sdma_run(
    DeviceState& ds, const void* zbuf, size_t zlen, hipStream_t s,
    const std::function<void(const std::vector<char*>&, std::vector<kern::CopyDesc>&)>& plan) {
  if (!ds.zc_ok || !cfg_.ipc_zc || capturing(s)) return false;  // (group-wide facts: every rank alike)
  launcher_quiesce(ds);  // inline exchange: the channel is this thread's now
  IpcComm& ic = ipc(ds);
  std::vector<char*> ptrs;
  const bool ok = zc_map(ds, zbuf, zlen, false, nullptr, ptrs);
  {
    std::lock_guard<std::mutex> lk(stats_mu_);
    ZcPart part;
    part.state = ok ? 1 : 0;
    zc_parts_.push_back(part);
  }
  if (!ok) return false;
  std::vector<kern::CopyDesc> copies;
  plan(ptrs, copies);
  copies.erase(std::remove_if(copies.begin(), copies.end(),
                              [](const kern::CopyDesc& d) { return d.bytes == 0 || d.src == d.dst; }),
               copies.end());
  // (one pull stays one copy: splitting a 64 MiB broadcast pull over three streams took 296 us against
  // 129 us whole, ranks sharing one MI355X -- profiles/r6/sdma/)
  const kern::IpcCall bar = copy_call(kern::IpcColl::BARRIER, 0);
  ic.launch(bar, s);  // arrival
  const int nside = std::min<int>(cfg_.sdma_streams, (int)copies.size() - 1);
  if (nside <= 0) {
    for (const auto& d : copies) PDCC_HIP(hipMemcpyAsync(d.dst, d.src, d.bytes, hipMemcpyDeviceToDevice, s));
  } else {
    while ((int)ds.sdma_side.size() < nside) {
      hipStream_t x = nullptr;
      PDCC_HIP(hipStreamCreateWithFlags(&x, hipStreamNonBlocking));
      ds.sdma_side.push_back(x);
    }
    hipEvent_t fork = ds.events->get();
    PDCC_HIP(hipEventRecord(fork, s));
    for (int k = 0; k < nside; ++k) PDCC_HIP(hipStreamWaitEvent(ds.sdma_side[k], fork, 0));
    ds.events->put(fork);
    for (size_t i = 0; i < copies.size(); ++i) {  // round-robin: copy i on stream i % (1 + nside)
      const int k = (int)(i % (size_t)(1 + nside));
      const auto& d = copies[i];
      PDCC_HIP(hipMemcpyAsync(d.dst, d.src, d.bytes, hipMemcpyDeviceToDevice, k == 0 ? s : ds.sdma_side[k - 1]));
    }
    for (int k = 0; k < nside; ++k) {
      hipEvent_t join = ds.events->get();
      PDCC_HIP(hipEventRecord(join, ds.sdma_side[k]));
      PDCC_HIP(hipStreamWaitEvent(s, join, 0));
      ds.events->put(join);
    }
  }
  ic.launch(bar, s);  // departure
  ic.zc_note_launch(ic.new_launch_event(s));  // (the mappings stay open until the pulls are done)
  return true;
}

c10::intrusive_ptr<c10d::Work> ProcessGroupMI355X::gpu_run(Coll c, DeviceState& ds,
                                                           const std::vector<at::Tensor>& keep_alive,
                                                           std::vector<at::Tensor> outputs,
                                                           std::chrono::milliseconds timeout,
                                                           const std::function<void(hipStream_t)>& fn,
                                                           std::shared_ptr<IpcComm> ipcp,
                                                           const c10::hip::HIPStreamMasqueradingAsCUDA* stream,
                                                           bool self_timed) {
  c10::hip::HIPGuardMasqueradingAsCUDA g((c10::DeviceIndex)ds.device);
  auto cur = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA((c10::DeviceIndex)ds.device);
  // synchronous collectives (and PDCC_STREAM=current) run on the caller's stream: no
  // cross-stream event hand-off, which costs far more than the launch on this runtime
  // (and graph capture always: the capturing stream is the only one the graph sees);
  // point-to-point runs on its pair's own stream (`stream`)
  const bool cap = capturing(cur.stream());
  const bool on_current = cap || (!stream && (cfg_.stream_mode == 3 || (cfg_.stream_mode != 2 && !op_async_)));
  const c10::hip::HIPStreamMasqueradingAsCUDA comm = on_current ? cur : (stream ? *stream : ds.stream);
  StreamSync& sy = *ds.sync;
  bool use_sig = false;
  // a synchronous collective after async ones that may still be running on the group's
  // comm stream: order it behind them (two collectives of one group never overlap)
  if (comm == cur && !cap && !stream) order_after_async(ds, cur.stream());
  SignalWord* done_word = nullptr;
  if (comm != cur) {
    {
      std::lock_guard<std::mutex> lk(sy.mu);  // tick + enqueue under one lock: words only ever grow
      if (sy.ok) {
        done_word = &sy.comm_done[comm.stream()];  // (std::map: the reference stays valid)
        if (!done_word->ptr) done_word->ptr = sy.alloc();
        if (!done_word->ptr) done_word = nullptr;
      }
      if (sy.ok && done_word) {
        SignalWord& w = sy.user_ready[cur.stream()];
        if (!w.ptr) w.ptr = sy.alloc();
        if (w.ptr) {
          const uint64_t t = ++w.next;
          PDCC_HIP(hipStreamWriteValue64(cur.stream(), w.ptr, t, 0));
          PDCC_HIP(hipStreamWaitValue64(comm.stream(), w.ptr, t, hipStreamWaitValueGte, ~0ull));
          use_sig = true;
        } else {
          sy.user_ready.erase(cur.stream());
        }
      }
    }
    if (!use_sig) {
      hipEvent_t pre = ds.events->get();
      PDCC_HIP(hipEventRecord(pre, cur.stream()));
      PDCC_HIP(hipStreamWaitEvent(comm.stream(), pre, 0));
      ds.events->put(pre);
    }
  }
  const bool rx = cfg_.roctx && roctx_push_;
  if (rx) roctx_push_((std::string("pdcc:") + coll_name(c)).c_str());
  {
    c10::hip::HIPStreamGuardMasqueradingAsCUDA sg(comm);  // temporaries + copy-backs run on the comm stream
    // an async collective (comm stream) runs next to the caller's compute: its IPC launches
    // take at most PDCC_IPC_ASYNC_GRID workgroups (async_op=True only: PDCC_STREAM=comm puts
    // synchronous calls on the comm stream too, and those keep the full grid)
    IpcComm::AsyncScope as(ipcp.get(), !stream && runs_capped(ds.device));  // (the autotuner keys on the same)
    fn(comm.stream());
  }
  if (rx && roctx_pop_) roctx_pop_();
  // graph capture: the graph node is the completion -- no event, nothing for the watchdog
  if (cap) return cpu_done(c, std::move(outputs));
  if (comm != cur) {  // the caching allocator must not recycle these before the comm stream is done
    for (const auto& t : keep_alive)
      if (t.defined() && t.is_cuda())
        c10::hip::HIPCachingAllocatorMasqueradingAsCUDA::recordStreamMasqueradingAsCUDA(t.storage().data_ptr(), comm);
    for (const auto& t : outputs)
      if (t.defined() && t.is_cuda())
        c10::hip::HIPCachingAllocatorMasqueradingAsCUDA::recordStreamMasqueradingAsCUDA(t.storage().data_ptr(), comm);
  }
  hipEvent_t ev = nullptr;
  uint64_t done_tick = 0;
  // A synchronous collective on the caller's stream whose kernels bound their own spins
  // (IPC: a stuck peer sets the error word the watchdog polls) needs no completion marker:
  // its Work is done as far as the caller's stream goes (no event record, ~1 us per call)
  const bool marker = !(self_timed && comm == cur && !cfg_.blocking_wait);
  if (use_sig) {
    std::lock_guard<std::mutex> lk(sy.mu);
    done_tick = ++done_word->next;
    PDCC_HIP(hipStreamWriteValue64(comm.stream(), done_word->ptr, done_tick, 0));
  } else if (marker) {
    ev = ds.events->get();
    PDCC_HIP(hipEventRecord(ev, comm.stream()));
  }
  auto w = c10::make_intrusive<WorkMI355X>(rank_, op_type(c), op_seq_.load(), std::move(outputs),
                                           c10::Device(c10::kCUDA, (c10::DeviceIndex)ds.device), ev, comm,
                                           health_, cfg_.blocking_wait, timeout, std::move(ipcp), ds.events);
  if (use_sig) w->set_signal(ds.sync, done_word->ptr, done_tick);
  if (cfg_.watchdog_ms > 0 && (marker || use_sig)) {
    std::lock_guard<std::mutex> lk(wd_mu_);
    inflight_.emplace_back(w);
  }
  {
    std::lock_guard<std::mutex> lk(stats_mu_);
    fr_last_work_ = w;  // picked up by record() for the flight recorder
  }
  return w;
}

// Make stream `s` wait (stream memory op, no host block) for every async collective of
// this group issued so far on the group's comm stream. p2p pair streams are not waited
// for: their peers may post the matching op later.
void ProcessGroupMI355X::order_after_async(DeviceState& ds, hipStream_t s) {
  StreamSync& sy = *ds.sync;
  std::lock_guard<std::mutex> lk(sy.mu);
  auto it = sy.comm_done.find(ds.stream.stream());
  if (it == sy.comm_done.end() || !it->second.ptr) return;
  uint64_t& seen = sy.comm_seen[s];
  if (seen < it->second.next) {
    PDCC_HIP(hipStreamWaitValue64(s, it->second.ptr, it->second.next, hipStreamWaitValueGte, ~0ull));
    seen = it->second.next;
  }
}

bool ProcessGroupMI355X::runs_capped(int device) const {
  return op_async_ && cfg_.ipc_async_grid > 0 && cfg_.stream_mode != 3 && !capturing_on(device);
}

c10d::OpType ProcessGroupMI355X::op_type(Coll c) {
  switch (c) {
    case Coll::ALLREDUCE: return c10d::OpType::ALLREDUCE;
    case Coll::REDUCE: return c10d::OpType::REDUCE;
    case Coll::BROADCAST: return c10d::OpType::BROADCAST;
    case Coll::ALLGATHER: return c10d::OpType::ALLGATHER;
    case Coll::GATHER: return c10d::OpType::GATHER;
    case Coll::SCATTER: return c10d::OpType::SCATTER;
    case Coll::REDUCE_SCATTER: return c10d::OpType::REDUCE_SCATTER;
    case Coll::ALLTOALL: return c10d::OpType::ALLTOALL;
    case Coll::SEND: return c10d::OpType::SEND;
    case Coll::RECV: return c10d::OpType::RECV;
    default: return c10d::OpType::BARRIER;
  }
}

c10::intrusive_ptr<c10d::Work> ProcessGroupMI355X::gpu_issue(Coll c, DeviceState& ds, Algo a,
                                                             const std::vector<at::Tensor>& keep_alive,
                                                             std::vector<at::Tensor> outputs,
                                                             std::chrono::milliseconds timeout,
                                                             std::function<void(hipStream_t)> job,
                                                             std::shared_ptr<IpcComm> ipcp) {
  hp_.lap(HostStage::CHOOSE);
  {  // (zero-copy attempts of the autotuner's scratch runs do not label this call)
    std::lock_guard<std::mutex> lk(stats_mu_);
    zc_parts_.clear();
  }
  auto w = gpu_run(c, ds, keep_alive, std::move(outputs), timeout, [&](hipStream_t s) {
    hp_.lap(HostStage::PRE);
    job(s);
    hp_.lap(HostStage::ENQUEUE);
  }, std::move(ipcp), nullptr, /*self_timed=*/is_ipc(a));
  hp_.lap(HostStage::WORK);
  return w;
}

// =================================================================== engines
const char* ProcessGroupMI355X::enqueue_allreduce(Algo a, const at::Tensor& w, const RedSpec& red, int root,
                                                  bool rooted, DeviceState& ds, hipStream_t s,
                                                  std::chrono::milliseconds to) {
  const StagedOnly staged_only(staged_only_, a == Algo::IPC_STAGED);  // (read by ipc_run)
  if (is_ipc(a)) {
    IpcComm& ic = ipc(ds);
    const bool one_shot = w.nbytes() <= cfg_.ipc_1shot_max;
    const char* label = one_shot ? "ipc_1shot" : a == Algo::IPC_WIDE ? "ipc_2shot_wide" : "ipc_2shot";
    kern::IpcCall c = reduce_call(
        rooted ? (one_shot ? kern::IpcColl::REDUCE_1SHOT : kern::IpcColl::REDUCE_2SHOT)
               : (one_shot ? kern::IpcColl::ALLREDUCE_1SHOT : kern::IpcColl::ALLREDUCE_2SHOT),
        red.kd, red.ko, size_, w.nbytes());
    c.root = root;
    if (a == Algo::IPC_WIDE) c.grid_cap = cfg_.ipc_wide_grid;  // (shared devices: capped in launch_view)
    if (a == Algo::IPC_PUSH && c.coll == kern::IpcColl::ALLREDUCE_2SHOT) {
      c.coll = kern::IpcColl::ALLREDUCE_PUSH;
      label = "ipc_push";
    }
    if (a == Algo::IPC_DYN && c.coll == kern::IpcColl::ALLREDUCE_2SHOT) {  // (zero-copy runs only)
      c.dyn = std::max(1, cfg_.ipc_dyn);  // chunks per workgroup
      label = "ipc_2shot_dyn";
    }
    c.dyn_min_rows = cfg_.ipc_dyn_min_rows;
    if (ll_size(ds, w.nbytes())) {  // small (all-)reduce: flag-tagged pushes, no staging copy, no barrier
      c.coll = kern::coll_traits(c.coll).ll_twin;
      label = "ipc_ll";
    }
    c.in[0] = w.data_ptr();
    c.out[0] = w.data_ptr();
    // 2-shot reads the peers' tensors in place (all-reduce: reduced in place too;
    // rooted reduce: into staging, so non-root tensors stay untouched)
    if (kern::coll_traits(c.coll).zc_unit == kern::ZcUnit::ROW)
      ipc_run(ds, c, w.data_ptr(), w.nbytes(), (size_t)size_ * kern::kTileBytes, ic.chunk_cap(), s);
    else
      ipc_chunked(ic, c, ic.chunk_cap(), s);
    return label;
  } else if (is_rccl(a)) {
    TORCH_CHECK(red.nok, "pdcc: RCCL has no reduction for ", op_name(red.op), " on ", w.scalar_type());
    RcclComm& rc = a == Algo::RCCL_WIDE ? rccl_wide(ds) : rccl(ds);
    RcclComm::Issue og(rc, s, capturing(s));
    if (rooted)
      PDCC_NCCLC(rc.get(), ncclReduce(w.data_ptr(), w.data_ptr(), w.numel(), red.nd, red.no, root, rc.get(), s));
    else
      PDCC_NCCLC(rc.get(), ncclAllReduce(w.data_ptr(), w.data_ptr(), w.numel(), red.nd, red.no, rc.get(), s));
    return a == Algo::RCCL_WIDE ? "rccl_wide" : "rccl";
  } else {  // HOST, synchronous
    PDCC_HIP(hipStreamSynchronize(s));
    at::Tensor h = w.cpu();
    if (rooted) shm().reduce(h.data_ptr(), h.numel(), h.scalar_type(), red.op, root, to);
    else shm().allreduce(h.data_ptr(), h.numel(), h.scalar_type(), red.op, to);
    if (!rooted || rank_ == root) const_cast<at::Tensor&>(w).copy_(h);
    return "host";
  }
}

const char* ProcessGroupMI355X::enqueue_broadcast(Algo a, const at::Tensor& w, int root, DeviceState& ds,
                                                  hipStream_t s, std::chrono::milliseconds to) {
  const StagedOnly staged_only(staged_only_, a == Algo::IPC_STAGED);  // (read by ipc_run)
  const size_t bytes = w.nbytes();
  if (a == Algo::IPC_SDMA && bytes >= cfg_.ipc_zc_min) {  // every non-root pulls the root's tensor
    const bool is_root = rank_ == root;
    if (sdma_run(ds, is_root ? w.data_ptr() : nullptr, is_root ? bytes : 0, s,
                 [&](const std::vector<char*>& p, std::vector<kern::CopyDesc>& d) {
                   if (!is_root) d.push_back({p[root], w.data_ptr(), bytes});
                 }))
      return "ipc_sdma";
  }
  if (is_ipc(a)) {
    IpcComm& ic = ipc(ds);
    kern::IpcCall c = copy_call(
        bytes <= cfg_.ipc_1shot_max ? kern::IpcColl::BROADCAST_1SHOT : kern::IpcColl::BROADCAST_2SHOT, bytes, root);
    c.in[0] = w.data_ptr();
    c.out[0] = w.data_ptr();
    if (ll_size(ds, bytes)) {  // small: the root pushes flag-tagged words
      c.coll = kern::coll_traits(c.coll).ll_twin;
      ic.launch(c, s);
      return "ipc_ll";
    }
    if (c.coll == kern::IpcColl::BROADCAST_2SHOT)
      ipc_run(ds, c, w.data_ptr(), bytes, (size_t)size_ * kern::kTileBytes, ic.chunk_cap(), s);
    else
      ipc_chunked(ic, c, ic.chunk_cap(), s);
    return c.coll == kern::IpcColl::BROADCAST_2SHOT ? "ipc_2shot" : "ipc_1shot";
  } else if (a == Algo::RCCL) {
    RcclComm& rc = rccl(ds);
    RcclComm::Issue og(rc, s, capturing(s));
    PDCC_NCCLC(rc.get(), ncclBroadcast(w.data_ptr(), w.data_ptr(), bytes, ncclUint8, root, rc.get(), s));
    return "rccl";
  } else {
    PDCC_HIP(hipStreamSynchronize(s));
    at::Tensor h = w.cpu();
    shm().broadcast(h.data_ptr(), bytes, root, to);
    if (rank_ != root) const_cast<at::Tensor&>(w).copy_(h);
    return "host";
  }
}

const char* ProcessGroupMI355X::enqueue_allgather(Algo a, const at::Tensor& wi, const std::vector<at::Tensor>& wo,
                                                  int root, bool rooted, DeviceState& ds, hipStream_t s,
                                                  std::chrono::milliseconds to) {
  const StagedOnly staged_only(staged_only_, a == Algo::IPC_STAGED);  // (read by ipc_run)
  const size_t bytes = wi.nbytes();
  const bool receiver = !rooted || rank_ == root;
  if (a == Algo::IPC_SDMA && bytes >= cfg_.ipc_zc_min) {  // every receiver pulls each rank's input
    if (sdma_run(ds, wi.data_ptr(), bytes, s, [&](const std::vector<char*>& p, std::vector<kern::CopyDesc>& d) {
          if (!receiver) return;
          for (int k = 1; k <= size_; ++k) {  // peers rotated from this rank: the first pulls spread over links
            const int r = (rank_ + k) % size_;
            d.push_back({r == rank_ ? wi.data_ptr() : p[r], wo[r].data_ptr(), bytes});
          }
        }))
      return "ipc_sdma";
  }
  if (is_ipc(a)) {
    IpcComm& ic = ipc(ds);
    kern::IpcCall c = copy_call(rooted ? kern::IpcColl::GATHER : kern::IpcColl::ALLGATHER, bytes, root);
    c.in[0] = wi.data_ptr();
    if (receiver)
      for (int r = 0; r < size_; ++r) c.out[r] = wo[r].data_ptr();
    if (ll_size(ds, bytes)) {  // small: flag-tagged pushes, no staging copy, no barrier
      c.coll = kern::coll_traits(c.coll).ll_twin;
      ic.launch(c, s);
      return "ipc_ll";
    }
    if (a == Algo::IPC_DYN && !rooted) c.dyn = std::max(1, cfg_.ipc_dyn);  // (zero-copy runs only)
    c.dyn_min_rows = cfg_.ipc_dyn_min_rows;
    ipc_run(ds, c, wi.data_ptr(), bytes, kern::kTileBytes, ic.chunk_cap(), s);
    return c.dyn ? "ipc_dyn" : "ipc";
  } else if (a == Algo::RCCL) {
    RcclComm& rc = rccl(ds);
    RcclComm::Issue og(rc, s, capturing(s));
    if (!rooted && is_flat(wo, bytes)) {
      PDCC_NCCLC(rc.get(), ncclAllGather(wi.data_ptr(), wo[0].data_ptr(), bytes, ncclUint8, rc.get(), s));
      return "rccl";
    } else if (!rooted && !cfg_.list_gather_p2p) {
      // staged: one ring all-gather into a staging buffer, then K2 unpacks into the list
      at::Tensor stg = at::empty({(int64_t)(bytes * size_)}, wi.options().dtype(at::kByte));
      PDCC_NCCLC(rc.get(), ncclAllGather(wi.data_ptr(), stg.data_ptr(), bytes, ncclUint8, rc.get(), s));
      std::vector<kern::CopyDesc> d;
      for (int r = 0; r < size_; ++r)
        d.push_back({static_cast<char*>(stg.data_ptr()) + r * bytes, wo[r].data_ptr(), bytes});
      multi_copy_or_memcpy(d, s);
      return "rccl_staged";
    } else {
      // zero copy: every receiver posts one recv per peer straight into its list entry;
      // over a fully connected xGMI node the W-1 transfers of a rank use W-1 links at once
      PDCC_NCCL(ncclGroupStart());
      for (int r = 0; r < size_; ++r) {
        if (r == rank_) continue;
        if (!rooted || r == root) PDCC_NCCL(ncclSend(wi.data_ptr(), bytes, ncclUint8, r, rc.get(), s));
        if (receiver) PDCC_NCCL(ncclRecv(wo[r].data_ptr(), bytes, ncclUint8, r, rc.get(), s));
      }
      PDCC_NCCLC(rc.get(), ncclGroupEnd());
      if (receiver && bytes)
        PDCC_HIP(hipMemcpyAsync(wo[rank_].data_ptr(), wi.data_ptr(), bytes, hipMemcpyDeviceToDevice, s));
      return rooted ? "rccl" : "rccl_p2p";
    }
  } else {
    PDCC_HIP(hipStreamSynchronize(s));
    at::Tensor h = wi.cpu();
    std::vector<at::Tensor> ho;
    std::vector<void*> ptrs(size_, nullptr);
    if (receiver)
      for (int r = 0; r < size_; ++r) {
        ho.push_back(at::empty_like(h));
        ptrs[r] = ho.back().data_ptr();
      }
    if (rooted) shm().gather(h.data_ptr(), ptrs, bytes, root, to);
    else shm().allgather(h.data_ptr(), ptrs, bytes, to);
    if (receiver)
      for (int r = 0; r < size_; ++r) const_cast<at::Tensor&>(wo[r]).copy_(ho[r]);
    return "host";
  }
}

const char* ProcessGroupMI355X::enqueue_scatter(Algo a, const std::vector<at::Tensor>& wi, const at::Tensor& wo,
                                                int root, DeviceState& ds, hipStream_t s,
                                                std::chrono::milliseconds to) {
  const StagedOnly staged_only(staged_only_, a == Algo::IPC_STAGED);  // (read by ipc_run)
  const size_t bytes = wo.nbytes();
  if (a == Algo::IPC_SDMA && bytes >= cfg_.ipc_zc_min) {
    // every rank pulls its chunk from the root's flat list (a list that is not one buffer is not
    // exportable: the record says so on every rank and the IPC kernels run instead)
    const bool is_root = rank_ == root;
    const void* z = is_root ? (is_flat(wi, bytes) ? wi[0].data_ptr() : nullptr) : nullptr;
    if (sdma_run(ds, z, is_root ? bytes * size_ : 0, s, [&](const std::vector<char*>& p, std::vector<kern::CopyDesc>& d) {
          d.push_back({is_root ? wi[root].data_ptr() : p[root] + (size_t)rank_ * bytes, wo.data_ptr(), bytes});
        }))
      return "ipc_sdma";
  }
  if (is_ipc(a)) {
    IpcComm& ic = ipc(ds);
    kern::IpcCall c = copy_call(kern::IpcColl::SCATTER, bytes, root);
    c.zstride = bytes;
    if (rank_ == root)
      for (int r = 0; r < size_; ++r) c.in[r] = wi[r].data_ptr();
    c.out[0] = wo.data_ptr();
    if (ll_size(ds, bytes)) {  // small: the root pushes chunk q to rank q
      c.coll = kern::coll_traits(c.coll).ll_twin;
      ic.launch(c, s);
      return "ipc_ll";
    }
    // a flat root list (e.g. x.chunk(W)) is read in place; the other ranks share nothing
    const void* z = rank_ == root ? (is_flat(wi, bytes) ? wi[0].data_ptr() : nullptr) : nullptr;
    ipc_run(ds, c, z, rank_ == root ? bytes * size_ : 0, kern::kTileBytes, ic.chunk_cap() / size_, s);
    return "ipc";
  } else if (a == Algo::RCCL) {
    RcclComm& rc = rccl(ds);
    RcclComm::Issue og(rc, s, capturing(s));
    PDCC_NCCL(ncclGroupStart());
    if (rank_ == root) {
      for (int r = 0; r < size_; ++r)
        if (r != root) PDCC_NCCL(ncclSend(wi[r].data_ptr(), bytes, ncclUint8, r, rc.get(), s));
    } else {
      PDCC_NCCL(ncclRecv(wo.data_ptr(), bytes, ncclUint8, root, rc.get(), s));
    }
    PDCC_NCCLC(rc.get(), ncclGroupEnd());
    if (rank_ == root && bytes)
      PDCC_HIP(hipMemcpyAsync(wo.data_ptr(), wi[root].data_ptr(), bytes, hipMemcpyDeviceToDevice, s));
    return "rccl";
  } else {
    PDCC_HIP(hipStreamSynchronize(s));
    std::vector<at::Tensor> hi;
    std::vector<const void*> ptrs(size_, nullptr);
    if (rank_ == root)
      for (int r = 0; r < size_; ++r) {
        hi.push_back(wi[r].cpu().contiguous());
        ptrs[r] = hi.back().data_ptr();
      }
    at::Tensor h = at::empty(wo.sizes(), wo.options().device(at::kCPU));
    shm().scatter(ptrs, h.data_ptr(), bytes, root, to);
    const_cast<at::Tensor&>(wo).copy_(h);
    return "host";
  }
}

const char* ProcessGroupMI355X::enqueue_reduce_scatter(Algo a, const std::vector<at::Tensor>& wi,
                                                       const at::Tensor& wo, const RedSpec& red, DeviceState& ds,
                                                       hipStream_t s, std::chrono::milliseconds to) {
  const StagedOnly staged_only(staged_only_, a == Algo::IPC_STAGED);  // (read by ipc_run)
  const size_t bytes = wo.nbytes();
  if (is_ipc(a)) {
    IpcComm& ic = ipc(ds);
    kern::IpcCall c = reduce_call(kern::IpcColl::REDUCE_SCATTER, red.kd, red.ko, size_, bytes);
    c.zstride = bytes;
    for (int r = 0; r < size_; ++r) c.in[r] = wi[r].data_ptr();
    c.out[0] = wo.data_ptr();
    if (ll_size(ds, bytes)) {  // small: chunk q pushed to rank q, reduced there
      c.coll = kern::coll_traits(c.coll).ll_twin;
      ic.launch(c, s);
      return "ipc_ll";
    }
    if (a == Algo::IPC_DYN) c.dyn = std::max(1, cfg_.ipc_dyn);  // (zero-copy runs only)
    c.dyn_min_rows = cfg_.ipc_dyn_min_rows;
    // a flat input (reduce_scatter_tensor) is read in place by every peer
    ipc_run(ds, c, is_flat(wi, bytes) ? wi[0].data_ptr() : nullptr, bytes * size_, kern::kTileBytes,
            ic.chunk_cap() / size_, s);
    return c.dyn ? "ipc_dyn" : "ipc";
  } else if (a == Algo::RCCL) {
    TORCH_CHECK(red.nok, "pdcc: RCCL has no reduction for ", op_name(red.op), " on ", wo.scalar_type());
    RcclComm& rc = rccl(ds);
    const void* src;
    at::Tensor stg;
    if (is_flat(wi, bytes)) {
      src = wi[0].data_ptr();
    } else {  // K2 pack into one staging buffer
      stg = at::empty({(int64_t)(bytes * size_)}, wo.options().dtype(at::kByte));
      std::vector<kern::CopyDesc> d;
      for (int r = 0; r < size_; ++r)
        d.push_back({wi[r].data_ptr(), static_cast<char*>(stg.data_ptr()) + r * bytes, bytes});
      multi_copy_or_memcpy(d, s);
      src = stg.data_ptr();
    }
    RcclComm::Issue og(rc, s, capturing(s));
    PDCC_NCCLC(rc.get(), ncclReduceScatter(src, wo.data_ptr(), wo.numel(), red.nd, red.no, rc.get(), s));
    return "rccl";
  } else {
    PDCC_HIP(hipStreamSynchronize(s));
    std::vector<at::Tensor> hi;
    std::vector<const void*> ptrs;
    for (const auto& i : wi) {
      hi.push_back(i.cpu().contiguous());
      ptrs.push_back(hi.back().data_ptr());
    }
    at::Tensor h = at::empty(wo.sizes(), wo.options().device(at::kCPU));
    shm().reduce_scatter(ptrs, h.data_ptr(), wo.numel(), wo.scalar_type(), red.op, to);
    const_cast<at::Tensor&>(wo).copy_(h);
    return "host";
  }
}

const char* ProcessGroupMI355X::enqueue_alltoall(Algo a, const std::vector<at::Tensor>& wi,
                                                 const std::vector<at::Tensor>& wo, bool equal, DeviceState& ds,
                                                 hipStream_t s, std::chrono::milliseconds to) {
  const StagedOnly staged_only(staged_only_, a == Algo::IPC_STAGED);  // (read by ipc_run)
  if (a == Algo::IPC_SDMA && equal && wi[0].nbytes() >= cfg_.ipc_zc_min) {
    // rank r pulls block r of every rank's flat input into its out[q] (a non-flat input: the IPC kernels)
    const size_t chunk = wi[0].nbytes();
    const void* z = is_flat(wi, chunk) ? wi[0].data_ptr() : nullptr;
    if (sdma_run(ds, z, chunk * size_, s, [&](const std::vector<char*>& p, std::vector<kern::CopyDesc>& d) {
          for (int k = 1; k <= size_; ++k) {
            const int q = (rank_ + k) % size_;
            d.push_back({q == rank_ ? wi[rank_].data_ptr() : p[q] + (size_t)rank_ * chunk, wo[q].data_ptr(), chunk});
          }
        }))
      return "ipc_sdma";
  }
  if (is_ipc(a)) {
    TORCH_CHECK(equal, "pdcc: the IPC all-to-all needs equal splits");
    IpcComm& ic = ipc(ds);
    kern::IpcCall c = copy_call(kern::IpcColl::ALLTOALL, wi[0].nbytes());
    c.zstride = c.bytes;
    for (int r = 0; r < size_; ++r) {
      c.in[r] = wi[r].data_ptr();
      c.out[r] = wo[r].data_ptr();
    }
    if (ll_size(ds, c.bytes)) {  // small: chunk q pushed straight to rank q
      c.coll = kern::coll_traits(c.coll).ll_twin;
      ic.launch(c, s);
      return "ipc_ll";
    }
    ipc_run(ds, c, is_flat(wi, c.bytes) ? wi[0].data_ptr() : nullptr, c.bytes * size_, kern::kTileBytes,
            ic.chunk_cap() / size_, s);
    return "ipc";
  } else if (a == Algo::RCCL) {
    RcclComm& rc = rccl(ds);
    RcclComm::Issue og(rc, s, capturing(s));
    const size_t chunk = wi[0].nbytes();
    if (equal && is_flat(wi, chunk) && is_flat(wo, chunk)) {
      PDCC_NCCLC(rc.get(), ncclAllToAll(wi[0].data_ptr(), wo[0].data_ptr(), chunk, ncclUint8, rc.get(), s));
    } else {
      PDCC_NCCL(ncclGroupStart());
      for (int r = 0; r < size_; ++r) {
        if (r == rank_) continue;
        if (wi[r].nbytes()) PDCC_NCCL(ncclSend(wi[r].data_ptr(), wi[r].nbytes(), ncclUint8, r, rc.get(), s));
        if (wo[r].nbytes()) PDCC_NCCL(ncclRecv(wo[r].data_ptr(), wo[r].nbytes(), ncclUint8, r, rc.get(), s));
      }
      PDCC_NCCLC(rc.get(), ncclGroupEnd());
      if (wi[rank_].nbytes())
        PDCC_HIP(hipMemcpyAsync(wo[rank_].data_ptr(), wi[rank_].data_ptr(), wi[rank_].nbytes(),
                                hipMemcpyDeviceToDevice, s));
    }
    return "rccl";
  } else {
    PDCC_HIP(hipStreamSynchronize(s));
    std::vector<at::Tensor> hi, ho;
    std::vector<const void*> ip;
    std::vector<void*> op;
    std::vector<size_t> sb, rb;
    for (const auto& i : wi) {
      hi.push_back(i.cpu().contiguous());
      ip.push_back(hi.back().data_ptr());
      sb.push_back(hi.back().nbytes());
    }
    for (const auto& o : wo) {
      ho.push_back(at::empty(o.sizes(), o.options().device(at::kCPU)));
      op.push_back(ho.back().data_ptr());
      rb.push_back(ho.back().nbytes());
    }
    shm().alltoall(ip, sb, op, rb, to);
    for (size_t i = 0; i < wo.size(); ++i) const_cast<at::Tensor&>(wo[i]).copy_(ho[i]);
    return "host";
  }
}

// =================================================================== one issue path
// What every GPU collective does once its front-end (below) has taken the local shortcut and prepared
// the buffers. The front-end hands over what differs: the tune-key slots (`c`), the race on scratch
// buffers (`tune`), its engine (`enqueue(algo, stream)`: returns the label of the protocol it ran), the
// copy from prepared temporaries back into the caller's tensors, what to keep alive and what the Work
// holds. A coalesced call (`co`) unpacks its members behind the collective, on the same stream.
template <class Tune, class Enqueue, class CopyBack>
c10::intrusive_ptr<c10d::Work> ProcessGroupMI355X::issue_collective(const Issue& c, DeviceState& ds, Tune&& tune,
                                                                    Enqueue&& enqueue, CopyBack&& copy_back,
                                                                    std::vector<at::Tensor> keep_alive,
                                                                    std::vector<at::Tensor> outputs,
                                                                    const std::shared_ptr<const Coalesced>& co) {
  const Algo a = decide(c.coll, c.key_dtype, c.key_op, c.bytes, ds, c.a0, c.rccl_can, c.ipc_can, tune);
  if (co) {
    keep_alive.insert(keep_alive.end(), co->members.begin(), co->members.end());
    outputs = co->members;
  }
  const char* label = nullptr;
  auto job = [&](hipStream_t s) {
    label = enqueue(a, s);
    copy_back();
    if (co) co->run(s);
  };
  c10::intrusive_ptr<c10d::Work> work;
  if (a == Algo::HOST) {  // synchronous, on the caller's stream
    job(current_stream(ds.device));
    work = cpu_done(c.coll, std::move(outputs));
  } else {  // (gpu_issue runs the job before it returns)
    std::shared_ptr<IpcComm> icp;
    if (is_ipc(a)) {
      ipc(ds);
      icp = ds.ipc;
    }
    work = gpu_issue(c.coll, ds, a, keep_alive, std::move(outputs), c.to, job, std::move(icp));
  }
  record(c.coll, label, c.stat_bytes, c.t0);
  if (a != Algo::HOST) hp_.lap(HostStage::RECORD);  // (the stage profile follows GPU engines only)
  return work;
}

// =================================================================== all-reduce / reduce
c10::intrusive_ptr<c10d::Work> ProcessGroupMI355X::gpu_allreduce(at::Tensor& t, RedOpType op, int root, bool rooted,
                                                                 std::chrono::milliseconds to,
                                                                 std::shared_ptr<const Coalesced> co) {
  const Coll cname = rooted ? Coll::REDUCE : Coll::ALLREDUCE;
  TORCH_CHECK(op != RedOpType::PREMUL_SUM, "ProcessGroupMI355X: PREMUL_SUM is not supported");
  const auto t0 = std::chrono::steady_clock::now();
  const size_t bytes = t.nbytes();
  if ((size_ == 1 && cfg_.world1_local) || bytes == 0) {
    record(cname, "local", bytes, t0);
    return cpu_done(cname, {t});
  }
  DeviceState& ds = dev_state(t);
  hp_.lap(HostStage::DEV_STATE);
  const RedSpec red = red_spec(t.scalar_type(), op);
  const bool rccl_can = ds.rccl_ok && red.nok, ipc_can = ds.ipc_ok && red.kok;
  const Algo a0 = choose(cname, bytes, ds, rccl_can, ipc_can);
  at::Tensor w = prep_in(t, ipc_can && ll_call(ds, bytes));  // (an LL call: any alignment, see prep_in)
  auto enqueue = [&](Algo a, const at::Tensor& x, hipStream_t s) {
    return enqueue_allreduce(a, x, red, root, rooted, ds, s, to);
  };
  auto tune = [&](const TuneKey& key, const std::vector<Algo>& cands) {
    const int64_t n = sample_numel(w.numel(), w.element_size(), cfg_.autotune_sample);
    std::vector<at::Tensor> sc;
    for (size_t k = 0; k < cands.size(); ++k) sc.push_back(w.reshape({-1}).narrow(0, 0, n).clone());
    const hipStream_t cs = current_stream(ds.device);
    return autotune(
        key, bytes, ds, cands, [&](size_t k) { enqueue(cands[k], sc[k], cs); },
        [&](size_t r, size_t k) { return results_match(sc[r], sc[k], op, size_); },
        [&] {  // IPC as the reference: itself vs the host transport on a prefix
          const int64_t m = sample_numel(w.numel(), w.element_size(), kHostTuneMax);
          at::Tensor h = w.reshape({-1}).narrow(0, 0, m).clone(), g = h.clone();
          enqueue(Algo::HOST, h, cs);
          enqueue(cands[0], g, cs);
          PDCC_HIP(hipStreamSynchronize(cs));
          // (a partial sanity check: the prefix runs the protocol of its own size, not the key's -- the
          // raced variants are then checked against the full-size reference run, results_match above)
          return results_match(h, g, op, size_);
        });
  };
  return issue_collective(
      {cname, (int)t.scalar_type(), (int)op, bytes, bytes, a0, rccl_can, ipc_can, t0, to}, ds, tune,
      [&](Algo a, hipStream_t s) { return enqueue(a, w, s); },
      [&] { if (!w.is_same(t) && (!rooted || rank_ == root)) t.copy_(w); },
      {t, w}, {t}, co);
}

// =================================================================== broadcast
c10::intrusive_ptr<c10d::Work> ProcessGroupMI355X::gpu_broadcast(at::Tensor& t, int root,
                                                                 std::chrono::milliseconds to) {
  const auto t0 = std::chrono::steady_clock::now();
  const size_t bytes = t.nbytes();
  if ((size_ == 1 && cfg_.world1_local) || bytes == 0) {
    record(Coll::BROADCAST, "local", bytes, t0);
    return cpu_done(Coll::BROADCAST, {t});
  }
  DeviceState& ds = dev_state(t);
  const Algo a0 = choose(Coll::BROADCAST, bytes, ds, ds.rccl_ok, ds.ipc_ok);
  at::Tensor w = prep_in(t, ll_call(ds, bytes));  // (an LL call: any alignment, see prep_in)
  auto tune = [&](const TuneKey& key, const std::vector<Algo>& cands) {
    const int64_t n = sample_numel(w.numel(), w.element_size(), cfg_.autotune_sample);
    std::vector<at::Tensor> sc;
    for (size_t k = 0; k < cands.size(); ++k) sc.push_back(w.reshape({-1}).narrow(0, 0, n).clone());
    const hipStream_t cs = current_stream(ds.device);
    return autotune(
        key, bytes, ds, cands, [&](size_t k) { enqueue_broadcast(cands[k], sc[k], root, ds, cs, to); },
        [&](size_t r, size_t k) { return at::equal(sc[r], sc[k]); },
        [&] {  // IPC as the reference: itself vs the host transport on a <= kHostTuneMax prefix (a
               // partial sanity check: the prefix takes the protocol of its own size)
          const int64_t m = sample_numel(w.numel(), w.element_size(), kHostTuneMax);
          at::Tensor h = w.reshape({-1}).narrow(0, 0, m).clone(), g = h.clone();
          enqueue_broadcast(Algo::HOST, h, root, ds, cs, to);
          enqueue_broadcast(cands[0], g, root, ds, cs, to);
          PDCC_HIP(hipStreamSynchronize(cs));
          return at::equal(h, g);
        });
  };
  return issue_collective(
      {Coll::BROADCAST, -1, -1, bytes, bytes, a0, ds.rccl_ok, ds.ipc_ok, t0, to}, ds, tune,
      [&](Algo a, hipStream_t s) { return enqueue_broadcast(a, w, root, ds, s, to); },
      [&] { if (!w.is_same(t) && rank_ != root) t.copy_(w); },
      {t, w}, {t});
}

// =================================================================== all-gather / gather
c10::intrusive_ptr<c10d::Work> ProcessGroupMI355X::gpu_allgather(std::vector<at::Tensor>& outs, at::Tensor& in,
                                                                 int root, bool rooted,
                                                                 std::chrono::milliseconds to,
                                                                 std::shared_ptr<const Coalesced> co) {
  const Coll cname = rooted ? Coll::GATHER : Coll::ALLGATHER;
  const auto t0 = std::chrono::steady_clock::now();
  const size_t bytes = in.nbytes();
  const bool receiver = !rooted || rank_ == root;
  if ((size_ == 1 && cfg_.world1_local) || bytes == 0) {
    if (!outs.empty()) outs[0].copy_(in);
    record(cname, "local", bytes, t0);
    return cpu_done(cname, outs);
  }
  DeviceState& ds = dev_state(in);
  const Algo a0 = choose(cname, bytes, ds, ds.rccl_ok, ds.ipc_ok);
  const bool any_align = ll_call(ds, bytes);  // (see prep_in)
  at::Tensor wi = prep_in(in, any_align);
  std::vector<at::Tensor> wo;
  if (receiver)
    for (auto& o : outs) wo.push_back(prep_out(o, any_align));
  // the layout is part of the key (RCCL takes a different path for a flat output);
  // on gather only the root has outputs, so the key cannot depend on them there
  const bool flat = !rooted && is_flat(wo, bytes);
  auto tune = [&](const TuneKey& key, const std::vector<Algo>& cands) {
    const int64_t n = sample_numel(wi.numel(), wi.element_size(), cfg_.autotune_sample, size_);
    const at::Tensor si = wi.reshape({-1}).narrow(0, 0, n);
    std::vector<std::vector<at::Tensor>> sc(cands.size());
    if (receiver)
      for (size_t k = 0; k < cands.size(); ++k) sc[k] = scratch_outputs(wi.options(), size_, n, flat);
    const hipStream_t cs = current_stream(ds.device);
    return autotune(
        key, bytes, ds, cands, [&](size_t k) { enqueue_allgather(cands[k], si, sc[k], root, rooted, ds, cs, to); },
        [&](size_t r, size_t k) { return lists_equal(sc[r], sc[k]); },
        [&] {  // IPC as the reference: exact against the host transport on a <= kHostTuneMax prefix
          const int64_t m = sample_numel(wi.numel(), wi.element_size(), kHostTuneMax, size_);
          const at::Tensor pi = wi.reshape({-1}).narrow(0, 0, m);
          std::vector<at::Tensor> h, g;
          if (receiver) {
            h = scratch_outputs(wi.options(), size_, m, flat);
            g = scratch_outputs(wi.options(), size_, m, flat);
          }
          enqueue_allgather(Algo::HOST, pi, h, root, rooted, ds, cs, to);
          enqueue_allgather(cands[0], pi, g, root, rooted, ds, cs, to);
          PDCC_HIP(hipStreamSynchronize(cs));
          return lists_equal(h, g);
        });
  };
  std::vector<at::Tensor> keep{in, wi};
  keep.insert(keep.end(), wo.begin(), wo.end());
  return issue_collective(
      {cname, -1, rooted ? -1 : (flat ? kLayoutFlat : kLayoutList), bytes, bytes, a0, ds.rccl_ok, ds.ipc_ok, t0, to},
      ds, tune, [&](Algo a, hipStream_t s) { return enqueue_allgather(a, wi, wo, root, rooted, ds, s, to); },
      [&] {
        if (receiver)
          for (int r = 0; r < size_; ++r)
            if (!wo[r].is_same(outs[r])) outs[r].copy_(wo[r]);
      },
      std::move(keep), outs, co);
}

// =================================================================== scatter
c10::intrusive_ptr<c10d::Work> ProcessGroupMI355X::gpu_scatter(at::Tensor& out, std::vector<at::Tensor>& ins,
                                                               int root, std::chrono::milliseconds to) {
  const auto t0 = std::chrono::steady_clock::now();
  const size_t bytes = out.nbytes();
  if ((size_ == 1 && cfg_.world1_local) || bytes == 0) {
    if (!ins.empty()) out.copy_(ins[0]);
    record(Coll::SCATTER, "local", bytes, t0);
    return cpu_done(Coll::SCATTER, {out});
  }
  DeviceState& ds = dev_state(out);
  const Algo a0 = choose(Coll::SCATTER, bytes, ds, ds.rccl_ok, ds.ipc_ok);
  const bool any_align = ll_call(ds, bytes);  // (see prep_in)
  std::vector<at::Tensor> wi;
  if (rank_ == root)
    for (auto& i : ins) wi.push_back(prep_in(i, any_align));
  at::Tensor wo = prep_out(out, any_align);
  auto tune = [&](const TuneKey& key, const std::vector<Algo>& cands) {
    const int64_t n = sample_numel(wo.numel(), wo.element_size(), cfg_.autotune_sample, size_);
    const std::vector<at::Tensor> si = sample_inputs(wi, n, false);
    std::vector<at::Tensor> sc;
    for (size_t k = 0; k < cands.size(); ++k) sc.push_back(at::empty({n}, wo.options()));
    const hipStream_t cs = current_stream(ds.device);
    return autotune(
        key, bytes, ds, cands, [&](size_t k) { enqueue_scatter(cands[k], si, sc[k], root, ds, cs, to); },
        [&](size_t r, size_t k) { return at::equal(sc[r], sc[k]); });
  };
  std::vector<at::Tensor> keep{out, wo};
  keep.insert(keep.end(), wi.begin(), wi.end());
  return issue_collective(
      {Coll::SCATTER, -1, -1, bytes, bytes, a0, ds.rccl_ok, ds.ipc_ok, t0, to}, ds, tune,
      [&](Algo a, hipStream_t s) { return enqueue_scatter(a, wi, wo, root, ds, s, to); },
      [&] { if (!wo.is_same(out)) out.copy_(wo); },
      std::move(keep), {out});
}

// =================================================================== reduce-scatter
c10::intrusive_ptr<c10d::Work> ProcessGroupMI355X::gpu_reduce_scatter(at::Tensor& out, std::vector<at::Tensor>& ins,
                                                                      RedOpType op, std::chrono::milliseconds to,
                                                                      std::shared_ptr<const Coalesced> co) {
  TORCH_CHECK(op != RedOpType::PREMUL_SUM, "ProcessGroupMI355X: PREMUL_SUM is not supported");
  const auto t0 = std::chrono::steady_clock::now();
  const size_t bytes = out.nbytes();
  if ((size_ == 1 && cfg_.world1_local) || bytes == 0) {
    if (!ins.empty()) out.copy_(ins[0]);
    record(Coll::REDUCE_SCATTER, "local", bytes, t0);
    return cpu_done(Coll::REDUCE_SCATTER, {out});
  }
  DeviceState& ds = dev_state(out);
  const RedSpec red = red_spec(out.scalar_type(), op);
  const bool rccl_can = ds.rccl_ok && red.nok, ipc_can = ds.ipc_ok && red.kok;
  const Algo a0 = choose(Coll::REDUCE_SCATTER, bytes, ds, rccl_can, ipc_can);
  const bool any_align = ll_call(ds, bytes);  // (see prep_in)
  std::vector<at::Tensor> wi;
  for (auto& i : ins) wi.push_back(prep_in(i, any_align));
  at::Tensor wo = prep_out(out, any_align);
  auto tune = [&](const TuneKey& key, const std::vector<Algo>& cands) {
    const int64_t n = sample_numel(wo.numel(), wo.element_size(), cfg_.autotune_sample, size_);
    const std::vector<at::Tensor> si = sample_inputs(wi, n, is_flat(wi, bytes));
    std::vector<at::Tensor> sc;
    for (size_t k = 0; k < cands.size(); ++k) sc.push_back(at::empty({n}, wo.options()));
    const hipStream_t cs = current_stream(ds.device);
    return autotune(
        key, bytes, ds, cands, [&](size_t k) { enqueue_reduce_scatter(cands[k], si, sc[k], red, ds, cs, to); },
        [&](size_t r, size_t k) { return results_match(sc[r], sc[k], op, size_); },
        [&] {  // IPC as the reference: itself vs the host transport on a prefix of every chunk
          const int64_t m = sample_numel(wo.numel(), wo.element_size(), kHostTuneMax, size_);
          const std::vector<at::Tensor> pi = sample_inputs(wi, m, false);
          at::Tensor h = at::empty({m}, wo.options()), g = at::empty({m}, wo.options());
          enqueue_reduce_scatter(Algo::HOST, pi, h, red, ds, cs, to);
          enqueue_reduce_scatter(cands[0], pi, g, red, ds, cs, to);
          PDCC_HIP(hipStreamSynchronize(cs));
          return results_match(h, g, op, size_);
        });
  };
  std::vector<at::Tensor> keep{out, wo};
  keep.insert(keep.end(), wi.begin(), wi.end());
  return issue_collective(
      {Coll::REDUCE_SCATTER, (int)out.scalar_type(), (int)op, bytes, bytes, a0, rccl_can, ipc_can, t0, to}, ds, tune,
      [&](Algo a, hipStream_t s) { return enqueue_reduce_scatter(a, wi, wo, red, ds, s, to); },
      [&] { if (!wo.is_same(out)) out.copy_(wo); },
      std::move(keep), {out}, co);
}

// =================================================================== all-to-all
c10::intrusive_ptr<c10d::Work> ProcessGroupMI355X::gpu_alltoall(std::vector<at::Tensor>& outs,
                                                                std::vector<at::Tensor>& ins, bool equal,
                                                                std::chrono::milliseconds to) {
  const auto t0 = std::chrono::steady_clock::now();
  size_t total = 0;
  for (auto& i : ins) total += i.nbytes();
  if (size_ == 1 && cfg_.world1_local) {
    outs[0].copy_(ins[0]);
    record(Coll::ALLTOALL, "local", total, t0);
    return cpu_done(Coll::ALLTOALL, outs);
  }
  DeviceState& ds = dev_state(ins[0]);
  const size_t chunk = ins[0].nbytes();
  // uneven splits take the same path: without the IPC engine (`ipc_can`) decide() has no candidates to
  // race and keeps the static choice, RCCL's grouped send/recv or the host transport
  const bool ipc_can = ds.ipc_ok && equal;
  const Algo a0 = choose(Coll::ALLTOALL, equal ? chunk : SIZE_MAX, ds, ds.rccl_ok, ipc_can);
  const bool any_align = equal && ll_call(ds, chunk);  // (see prep_in)
  std::vector<at::Tensor> wi, wo;
  for (auto& i : ins) wi.push_back(prep_in(i, any_align));
  for (auto& o : outs) wo.push_back(prep_out(o, any_align));
  const bool flat = equal && is_flat(wi, chunk) && is_flat(wo, chunk);
  auto tune = [&](const TuneKey& key, const std::vector<Algo>& cands) {
    const int64_t n = sample_numel(wi[0].numel(), wi[0].element_size(), cfg_.autotune_sample, size_);
    const std::vector<at::Tensor> si = sample_inputs(wi, n, flat);
    std::vector<std::vector<at::Tensor>> sc;
    for (size_t k = 0; k < cands.size(); ++k) sc.push_back(scratch_outputs(wo[0].options(), size_, n, flat));
    const hipStream_t cs = current_stream(ds.device);
    return autotune(
        key, chunk, ds, cands, [&](size_t k) { enqueue_alltoall(cands[k], si, sc[k], true, ds, cs, to); },
        [&](size_t r, size_t k) { return lists_equal(sc[r], sc[k]); });
  };
  std::vector<at::Tensor> keep = wi;
  keep.insert(keep.end(), wo.begin(), wo.end());
  return issue_collective(
      {Coll::ALLTOALL, -1, flat ? kLayoutFlat : kLayoutList, chunk, total, a0, ds.rccl_ok, ipc_can, t0, to}, ds, tune,
      [&](Algo a, hipStream_t s) { return enqueue_alltoall(a, wi, wo, equal, ds, s, to); },
      [&] {
        for (size_t i = 0; i < outs.size(); ++i)
          if (!wo[i].is_same(outs[i])) outs[i].copy_(wo[i]);
      },
      std::move(keep), outs);
}

}  // namespace pdcc
