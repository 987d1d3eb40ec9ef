// Point-to-point of ProcessGroupMI355X on GPU tensors (2-rank pair channels on their own streams, the
// host-staged fallback) and batch_isend_irecv coalescing: nothing here uses the engines of gpu_ops.cpp.
#include "gpu_util.h"

namespace pdcc {

using namespace gpu;

// Host-staged point-to-point (ranks sharing a GPU, or PDCC_ALGO=host): the copy to
// the host happens now, on the caller's stream; the transfer runs on the backend's
// send/recv threads over the pair's shared-memory channel, so isend/irecv pairs
// and rings never deadlock; the copy back to the GPU happens on the recv thread.
c10::intrusive_ptr<c10d::Work> ProcessGroupMI355X::host_p2p(at::Tensor& t, int peer, bool is_send,
                                                            std::chrono::milliseconds to) {
  TORCH_CHECK(!capturing_on(t.device().index()), "pdcc: ", is_send ? "send" : "recv",
              " runs on the host transport here, which cannot be captured into a graph");
  const auto t0 = std::chrono::steady_clock::now();
  const Coll cname = is_send ? Coll::SEND : Coll::RECV;
  auto work = c10::make_intrusive<WorkMI355X>(rank_, is_send ? c10d::OpType::SEND : c10d::OpType::RECV,
                                              op_seq_.load(), std::vector<at::Tensor>{t});
  const int pi = peer < rank_ ? 0 : 1;  // the peer's rank inside the pair channel
  if (is_send) {
    at::Tensor h = t.cpu().contiguous();
    p2p_submit(true, Job{[this, h, peer, pi, to] { shm_pair(peer).send(h.data_ptr(), h.nbytes(), pi, to); }, work});
  } else {
    p2p_submit(false, Job{[this, t, peer, pi, to]() mutable {
                            at::Tensor h = at::empty(t.sizes(), t.options().device(at::kCPU));
                            shm_pair(peer).recv(h.data_ptr(), h.nbytes(), pi, to);
                            c10::hip::HIPGuardMasqueradingAsCUDA g(t.device());
                            t.copy_(h);
                            PDCC_HIP(hipStreamSynchronize(current_stream(t.device().index())));
                          },
                          work});
  }
  if (coalescing_) coalesced_cpu_.push_back(work);
  record(cname, "host", t.nbytes(), t0);
  return work;
}

c10::intrusive_ptr<c10d::Work> ProcessGroupMI355X::gpu_p2p(at::Tensor& t, int peer, bool is_send,
                                                           std::chrono::milliseconds to) {
  const auto t0 = std::chrono::steady_clock::now();
  const Coll cname = is_send ? Coll::SEND : Coll::RECV;
  if (coalescing_) {
    // batch_isend_irecv: one group call on the group's communicator (like ProcessGroupNCCL,
    // every rank of the group takes part in the batch that first uses it)
    DeviceState& ds = dev_state(t);
    if (!ds.rccl_ok || cfg_.force_algo == Algo::HOST) return host_p2p(t, peer, is_send, to);
    RcclComm& rc = rccl(ds);
    at::Tensor w = is_send ? prep_in(t) : prep_out(t);
    coalesced_.push_back([w, peer, is_send, comm = rc.get()](hipStream_t s) mutable {
      if (is_send) PDCC_NCCL(ncclSend(w.data_ptr(), w.nbytes(), ncclUint8, peer, comm, s));
      else PDCC_NCCL(ncclRecv(w.data_ptr(), w.nbytes(), ncclUint8, peer, comm, s));
    });
    coalesced_tensors_.push_back(t);
    coalesced_tensors_.push_back(w);
    coalesced_ds_ = &ds;
    record(cname, "rccl_coalesced", t.nbytes(), t0);
    return cpu_done(cname, {t});
  }
  // single send/recv: only this pair of ranks takes part
  DeviceState& ds = dev_local(t);
  if (cfg_.force_algo == Algo::HOST || !pair_on_distinct_devices(ds, peer)) return host_p2p(t, peer, is_send, to);
  auto pc = pair_chan(ds, peer);
  const int pi = peer < rank_ ? 0 : 1;  // the peer's rank in the pair communicator
  at::Tensor w = is_send ? prep_in(t) : prep_out(t);
  {
    std::unique_lock<std::mutex> lk(pc->mu);
    if (!pc->error.empty()) throw std::runtime_error("pdcc: point-to-point channel to rank " + std::to_string(peer) +
                                                     " failed: " + pc->error);
    if (!(pc->ready && pc->q.empty())) {
      // the channel's communicator is still being built: queue behind it, in order
      TORCH_CHECK(!capturing_on(ds.device), "pdcc: the first send/recv between two ranks cannot be captured into a "
                  "graph (it builds their communicator): run one exchange before capturing");
      c10::hip::HIPGuardMasqueradingAsCUDA g((c10::DeviceIndex)ds.device);
      auto gate = std::make_shared<Gate>();
      PDCC_HIP(hipEventCreateWithFlags(&gate->ev, hipEventDisableTiming));
      hipEvent_t after = nullptr;
      PDCC_HIP(hipEventCreateWithFlags(&after, hipEventDisableTiming));
      PDCC_HIP(hipEventRecord(after, current_stream(ds.device)));
      pc->q.push_back({is_send, t, w, after, gate});
      auto work = c10::make_intrusive<WorkMI355X>(
          rank_, is_send ? c10d::OpType::SEND : c10d::OpType::RECV, op_seq_.load(), std::vector<at::Tensor>{t},
          c10::Device(c10::kCUDA, (c10::DeviceIndex)ds.device), gate->ev, pc->stream, health_, cfg_.blocking_wait,
          to, nullptr, nullptr);
      work->set_gate(gate);
      if (!pc->started) {
        pc->started = true;
        // self-contained (copies only): the thread may outlive a group destroyed meanwhile
        const int lo = std::min(rank_, peer), hi = std::max(rank_, peer);
        std::thread([pc, store = store_, key = "pdcc/p2p/" + std::to_string(lo) + ":" + std::to_string(hi),
                     prank = rank_ == lo ? 0 : 1, dev = ds.device, pi,
                     init_ms = cfg_.rccl_nonblocking ? rccl_opts().init_timeout_ms : int64_t{0}] {
          pair_builder(pc, store, key, prank, dev, pi, init_ms);
        }).detach();
      }
      if (cfg_.watchdog_ms > 0) {
        std::lock_guard<std::mutex> wl(wd_mu_);
        inflight_.emplace_back(work);
      }
      record(cname, "rccl_pair_deferred", t.nbytes(), t0);
      return work;
    }
  }
  auto work = gpu_run(cname, ds, {t, w}, {t}, to, [&](hipStream_t s) {
    if (is_send) PDCC_NCCLC(pc->comm->get(), ncclSend(w.data_ptr(), w.nbytes(), ncclUint8, pi, pc->comm->get(), s));
    else PDCC_NCCLC(pc->comm->get(), ncclRecv(w.data_ptr(), w.nbytes(), ncclUint8, pi, pc->comm->get(), s));
    if (!is_send && !w.is_same(t)) t.copy_(w);
  }, nullptr, &pc->stream);
  record(cname, "rccl_pair", t.nbytes(), t0);
  return work;
}

// Builder thread of a PairChan: create the 2-rank communicator (blocking on the peer),
// then enqueue the ops that queued up meanwhile, in order, each after its caller's
// stream point, and open their gates; then mark the channel ready.
void ProcessGroupMI355X::pair_builder(std::shared_ptr<PairChan> pc, c10::intrusive_ptr<c10d::Store> store,
                                      std::string key, int prank, int dev, int pi, int64_t init_ms) {
  std::string err;
  try {
    PDCC_HIP(hipSetDevice(dev));
    const auto t0 = std::chrono::steady_clock::now();
    RcclOpts o;
    o.init_timeout_ms = init_ms;  // the peer may never post its side: bounded
    o.nonblocking = init_ms > 0;
    auto c = std::make_shared<RcclComm>(store, key, prank, 2, dev, o);
    std::lock_guard<std::mutex> lk(pc->mu);
    pc->comm = c;
    pc->init_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  } catch (const std::exception& e) {
    err = e.what();
  }
  for (;;) {
    PairChan::Op op;
    {
      std::lock_guard<std::mutex> lk(pc->mu);
      if (!err.empty()) pc->error = err;
      if (pc->q.empty()) {
        pc->ready = pc->error.empty();
        return;
      }
      op = std::move(pc->q.front());
      pc->q.pop_front();
    }
    try {
      if (!err.empty()) throw std::runtime_error(err);
      c10::hip::HIPStreamGuardMasqueradingAsCUDA sg(pc->stream);
      const hipStream_t s = pc->stream.stream();
      PDCC_HIP(hipStreamWaitEvent(s, op.after, 0));
      if (op.is_send) PDCC_NCCLC(pc->comm->get(), ncclSend(op.w.data_ptr(), op.w.nbytes(), ncclUint8, pi, pc->comm->get(), s));
      else PDCC_NCCLC(pc->comm->get(), ncclRecv(op.w.data_ptr(), op.w.nbytes(), ncclUint8, pi, pc->comm->get(), s));
      if (!op.is_send && !op.w.is_same(op.t)) op.t.copy_(op.w);
      for (const at::Tensor* x : {&op.t, &op.w})
        c10::hip::HIPCachingAllocatorMasqueradingAsCUDA::recordStreamMasqueradingAsCUDA(x->storage().data_ptr(),
                                                                                         pc->stream);
      PDCC_HIP(hipEventRecord(op.gate->ev, s));
      op.gate->state.store(1, std::memory_order_release);
    } catch (const std::exception& e) {
      if (err.empty()) err = e.what();
      std::lock_guard<std::mutex> lk(op.gate->mu);
      op.gate->error = std::string("send/recv channel setup failed: ") + e.what();
      op.gate->state.store(-1, std::memory_order_release);
    }
    (void)hipEventDestroy(op.after);
  }
}

void ProcessGroupMI355X::startCoalescing() {
  coalescing_ = true;
  coalesced_cpu_.clear();
  coalesced_.clear();
  coalesced_tensors_.clear();
  coalesced_ds_ = nullptr;
}

c10::intrusive_ptr<c10d::Work> ProcessGroupMI355X::endCoalescing() {
  coalescing_ = false;
  DeviceState* ds = coalesced_ds_;
  if (!ds) {
    std::lock_guard<std::mutex> lk(init_mu_);
    if (devs_.size() == 1) ds = devs_.begin()->second.get();
  }
  // CPU p2p posted inside the batch runs on the worker threads: wait for all of
  // it so the returned work really covers the batch (all ops are already posted,
  // so this cannot deadlock the exchange)
  auto cpu_works = std::move(coalesced_cpu_);
  coalesced_cpu_.clear();
  for (auto& w : cpu_works) w->wait();
  if (!ds) return cpu_done(Coll::SEND, {});
  // nothing was batched (torch's fast path issued one coalesced collective instead): a synchronous
  // one already ran on the caller's stream, so there is nothing to order -- an async one ran on the
  // comm stream and the returned work must cover it (below)
  if (coalesced_.empty() && !op_async_) {
    coalesced_tensors_.clear();
    coalesced_ds_ = nullptr;
    return cpu_done(Coll::SEND, {});
  }
  auto fns = std::move(coalesced_);
  auto keep = std::move(coalesced_tensors_);
  coalesced_.clear();
  coalesced_tensors_.clear();
  coalesced_ds_ = nullptr;
  return gpu_run(Coll::SEND, *ds, keep, {}, timeout_, [&](hipStream_t s) {
    if (fns.empty()) return;
    // the batch runs on the group's communicator (rccl() made it when the first op was posted)
    RcclComm::Issue og(*ds->rccl, s, capturing(s));
    PDCC_NCCL(ncclGroupStart());
    for (auto& f : fns) f(s);
    PDCC_NCCLC(ds->rccl->get(), ncclGroupEnd());
    for (size_t i = 0; i + 1 < keep.size(); i += 2)
      if (!keep[i].is_same(keep[i + 1])) keep[i].copy_(keep[i + 1]);
  });
}

}  // namespace pdcc
