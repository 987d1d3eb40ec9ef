"""Rank functions of the `mxfp4_e2m1` tests (tests/test_mx4_cpu.py, tests/test_mx4_gpu.py). The
reference is always tests/_mx4_ref.py; results must equal it as values (rtol = atol = 0, NaN where
it has NaN) and be the same bytes on every rank. Inputs are those of the FP8 tests
(tests/_workers_mx.py, _workers_mx_shard.py): large / negated / small blocks that tell fold orders apart."""
import torch

from tests import _mx4_ref as R4
from tests import _mx_shard_ref as SR8
from tests._workers_mx import _dev, digest, rank_inputs
from tests._workers_mx_shard import shard_inputs

WIRE = R4.WIRE


def _seed(n):
    return 4000 + n % 9973


def collective_cases(rank, size, device="cpu", numels=(1, 33), dtypes=("float32",), ops=("sum", "avg"),
                     async_op=False):
    """For every (dtype, n): all_reduce_compressed of n elements (every op), reduce_scatter_compressed
    into n elements (every op) and all_gather_compressed of n elements per rank, all over the FP4 wire,
    against _mx4_ref. Returns {case: [equals the reference, digest of the result bytes]}."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd import distributed as pd

    d = _dev(device)

    def finish(w, t, want, dt):
        # the call ran on a side stream; a multiply queued on the current stream after wait() must see it
        w.wait()
        t.mul_(2.0)
        if d.type == "cuda":
            torch.cuda.synchronize()
        assert w.is_completed()
        return (want.to(torch.float32) * 2.0).to(dt)

    out = {}
    for dtn in dtypes:
        dt = R4.DTYPES[dtn]
        for n in numels:
            xs = rank_inputs(n, size, _seed(n), dt)
            ss = shard_inputs(n, size, _seed(n) + 17, dt)
            for op in ops:
                rop = dist.ReduceOp.SUM if op == "sum" else dist.ReduceOp.AVG
                want = R4.all_reduce(xs, op, dt)
                t = xs[rank].clone().to(d)
                if async_op:
                    want = finish(pd.all_reduce_compressed(t, rop, wire=WIRE, async_op=True), t, want, dt)
                else:
                    assert pd.all_reduce_compressed(t, rop, wire=WIRE) is None
                out[f"ar/{dtn}/{n}/{op}"] = [R4.same(t, want), digest(t)]
                want = R4.reduce_scatter(ss, rank, op, dt)
                x = ss[rank].clone().to(d)
                t = torch.full((n,), -7.5, dtype=dt, device=d)
                if async_op:
                    want = finish(pd.reduce_scatter_compressed(t, x, rop, wire=WIRE, async_op=True), t, want, dt)
                else:
                    assert pd.reduce_scatter_compressed(t, x, rop, wire=WIRE) is None
                out[f"rs/{dtn}/{n}/{op}"] = [R4.same(t, want) and torch.equal(x.cpu(), ss[rank]), digest(t)]
            shards = [v[:n] for v in ss]
            want = R4.all_gather(shards, dt)
            t = torch.full((n * size,), -7.5, dtype=dt, device=d)
            mine = shards[rank].clone().to(d)
            if async_op:
                want = finish(pd.all_gather_compressed(t, mine, wire=WIRE, async_op=True), t, want, dt)
            else:
                assert pd.all_gather_compressed(t, mine, wire=WIRE) is None
            out[f"ag/{dtn}/{n}"] = [R4.same(t, want), digest(t)]
    dist.barrier()
    return out


def world1_and_errors(rank, size, device="cpu"):
    """World 1 leaves the data bit for bit; every error case, raised before any communication."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd import distributed as pd

    d = _dev(device)
    ar = lambda t, *a, **k: pd.all_reduce_compressed(t, *a, wire=WIRE, **k)  # noqa: E731
    rs = lambda o, i, *a, **k: pd.reduce_scatter_compressed(o, i, *a, wire=WIRE, **k)  # noqa: E731
    ag = lambda o, i, **k: pd.all_gather_compressed(o, i, wire=WIRE, **k)  # noqa: E731
    out = {}
    if size == 1:
        g1 = dist.new_group([rank])
        x = torch.from_numpy(R4.edge_tensor()[0])[:777].clone()
        for dtn, dt in R4.DTYPES.items():
            src = x.to(dt).to(d)
            t = src.clone()
            ar(t, dist.ReduceOp.AVG, group=g1)
            w = ar(t, async_op=True)
            out[f"unchanged/{dtn}"] = bool(torch.equal(t.view(torch.uint8), src.view(torch.uint8))
                                           and w.is_completed() and w.wait())
            for name, fn in (("rs", lambda o, i, **k: rs(o, i, dist.ReduceOp.AVG, **k)), ("ag", ag)):
                dst = torch.zeros_like(src)
                fn(dst, src, group=g1)
                w = fn(dst, src, async_op=True)
                out[f"copied/{name}/{dtn}"] = bool(torch.equal(dst.view(torch.uint8), src.view(torch.uint8))
                                                   and w.is_completed() and w.wait())
    big, small = torch.ones(64 * size, device=d), torch.ones(64, device=d)

    def raises(kind, fn, *needles):
        try:
            fn()
            return False
        except kind as e:
            return all(n in str(e) for n in needles)

    out["ar_op"] = raises(ValueError, lambda: ar(small, dist.ReduceOp.MAX), "MAX")
    out["rs_op"] = raises(ValueError, lambda: rs(small, big, dist.ReduceOp.PRODUCT), "PRODUCT")
    out["ar_dtype"] = raises(TypeError, lambda: ar(small.double()), "float64")
    out["rs_dtype"] = raises(TypeError, lambda: rs(small.double(), big.double()), "float64")
    out["ag_dtype"] = raises(TypeError, lambda: ag(big.to(torch.int32), small.to(torch.int32)), "int32")
    out["rs_dtypes_differ"] = raises(TypeError, lambda: rs(small.to(torch.bfloat16), big), "float32", "bfloat16")
    out["rs_numel"] = raises(ValueError, lambda: rs(small[:63], big), str(64 * size), str(63 * size))
    out["ag_numel"] = raises(ValueError, lambda: ag(big, small[:63]), str(64 * size), str(63 * size))
    wide = torch.ones(64 * size, 2, device=d)
    out["rs_strided_output"] = raises(ValueError, lambda: rs(torch.ones(64, 2, device=d)[:, 0], big), "contiguous")
    out["ag_strided_output"] = raises(ValueError, lambda: ag(wide[:, 0], small), "contiguous")
    for bad in ("mxfp4", "mxfp6"):  # still unknown; the message lists the supported names
        out[f"ar_{bad}"] = raises(ValueError, lambda: pd.all_reduce_compressed(small, wire=bad), repr(bad), WIRE)
        out[f"rs_{bad}"] = raises(ValueError, lambda: pd.reduce_scatter_compressed(small, big, wire=bad), repr(bad))
        out[f"ag_{bad}"] = raises(ValueError, lambda: pd.all_gather_compressed(big, small, wire=bad), repr(bad))
    out["untouched"] = bool((big == 1).all() and (small == 1).all())
    dist.barrier()
    return out


def bucketer(rank, size, device="cuda", bucket_bytes=2048):
    """GradBucketer(wire="mxfp4_e2m1") on the in-tree MLP: one backward, one finish(); every bucket
    must equal _mx4_ref's AVG all-reduce of the ranks' raw gradients (exchanged uncompressed)."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd.models import MLP, synthetic_batch
    from pytorch_distributed_collective_communication_amd.parallel import ddp

    d = _dev(device)
    torch.manual_seed(100)
    model = MLP().to(d)
    raw = {}
    params = [p for p in model.parameters() if p.requires_grad]
    hooks = [p.register_post_accumulate_grad_hook(lambda p: raw.__setitem__(id(p), p.grad.detach().clone()))
             for p in params]
    buck = ddp.GradBucketer(model, bucket_bytes=bucket_bytes, wire=WIRE)
    x, y = synthetic_batch(64, device=d)
    shard = 64 // size
    xs, ys = x[rank * shard:(rank + 1) * shard], y[rank * shard:(rank + 1) * shard]
    torch.nn.functional.mse_loss(model(xs), ys).backward()
    handles = [type(b.work).__name__ for b in buck.buckets]
    buck.finish()
    out = {"buckets": len(buck.buckets), "handles": sorted(set(handles))}
    for i, b in enumerate(buck.buckets):
        mine = torch.cat([raw[id(p)].reshape(-1) for p in b.params])
        every = [torch.empty_like(mine) for _ in range(size)]
        dist.all_gather(every, mine)
        want = R4.all_reduce([e.cpu() for e in every], "avg", mine.dtype)
        got = torch.cat([p.grad.reshape(-1) for p in b.params])
        out[i] = [R4.same(got, want) and R4.same(b.flat, want), digest(got), b.numel]
    for h in hooks:
        h.remove()
    buck.remove()
    dist.barrier()
    return out


def zero(rank, size, device="cuda", grad_wire=WIRE, param_wire=WIRE, bucket_bytes=2048):
    """ShardedOptimizer with the given wires (FP4, FP8 or None each) on the in-tree MLP: one backward,
    one step(). Every bucket's grad_shard must equal the reference AVG reduce-scatter of the ranks' raw
    flat gradients in `grad_wire`, and `flat` after the step the reference all-gather of the ranks'
    param_shards in `param_wire` (both exchanged uncompressed; an uncompressed wire is not compared)."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd.models import MLP, synthetic_batch
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    ref = {WIRE: R4, "mxfp8_e4m3": SR8}
    d = _dev(device)
    torch.manual_seed(100)
    model = MLP().to(d)
    raw = {}
    params = [p for p in model.parameters() if p.requires_grad]
    hooks = [p.register_post_accumulate_grad_hook(lambda p: raw.__setitem__(id(p), p.grad.detach().clone()))
             for p in params]
    opt = ShardedOptimizer(model.parameters(), torch.optim.SGD, lr=0.05, bucket_bytes=bucket_bytes,
                           grad_wire=grad_wire, param_wire=param_wire)
    x, y = synthetic_batch(64, device=d)
    shard = 64 // size
    xs, ys = x[rank * shard:(rank + 1) * shard], y[rank * shard:(rank + 1) * shard]
    torch.nn.functional.mse_loss(model(xs), ys).backward()
    (s,) = opt.spaces
    handles = sorted({type(b.work).__name__ for b in s.buckets})
    every = []
    for b in s.buckets:  # (the exchange below must not overlap the side stream's reduce-scatters)
        if b.work is not None:
            b.work.wait()
    for b in s.buckets:
        flat = torch.zeros(b.padded, dtype=s.dtype, device=d)
        for i in b.idx:
            p, o = s.params[i], s.offsets[i] - b.off
            flat[o:o + p.numel()] = raw[id(p)].reshape(-1)
        got = [torch.empty_like(flat) for _ in range(size)]
        dist.all_gather(got, flat)
        every.append([g.cpu() for g in got])
    opt.step()
    out = {"buckets": len(s.buckets), "handles": handles}
    shards = [torch.empty_like(s.param_shard) for _ in range(size)]
    dist.all_gather(shards, s.param_shard)
    shards = [t.cpu() for t in shards]
    for i, b in enumerate(s.buckets):
        ok_g = ok_p = True
        if grad_wire is not None:
            want_g = ref[grad_wire].reduce_scatter(every[i], rank, "avg", s.dtype)
            ok_g = R4.same(s.grad_shard[b.soff:b.soff + b.shard], want_g)
        if param_wire is not None:
            want_p = ref[param_wire].all_gather([t[b.soff:b.soff + b.shard] for t in shards], s.dtype)
            ok_p = R4.same(s.flat[b.off:b.off + b.padded], want_p)
        out[i] = [ok_g, ok_p, b.padded]
    out["digest"] = digest(s.flat)
    for h in hooks:
        h.remove()
    opt.remove_hooks()
    dist.barrier()
    return out
