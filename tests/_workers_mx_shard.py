"""Rank functions and inputs of the compressed reduce-scatter / all-gather tests
(tests/test_mx_shard_cpu.py, tests/test_mx_shard_gpu.py). The reference is always
tests/_mx_shard_ref.py; results must equal it as values (rtol = atol = 0, NaN where it has NaN)."""
import torch

from tests import _mx_ref as R
from tests import _mx_shard_ref as SR
from tests._workers_mx import _dev, digest, rank_inputs


def shard_inputs(m, world, seed, dtype=torch.float32):
    """One CPU tensor of world * m elements per rank, built shard by shard (rank_inputs(m, world,
    seed + shard)), so the large / negated / small pairing stays block-aligned inside every shard."""
    per_shard = [rank_inputs(m, world, seed + k, dtype) for k in range(world)]
    return [torch.cat([per_shard[k][r] for k in range(world)]) for r in range(world)]


def _seed(m):
    return 2000 + m % 9973


def collective_cases(rank, size, device="cpu", ms=(1, 33), dtypes=("float32",), ops=("sum", "avg"), async_op=False):
    """reduce_scatter_compressed of every (dtype, m, op) and all_gather_compressed of every (dtype, m)
    against _mx_shard_ref. Returns {case: [equals the reference, digest of the result, engine label]}."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd import distributed as pd

    d = _dev(device)
    label = lambda: ""  # noqa: E731
    if d.type == "cuda":
        from pytorch_distributed_collective_communication_amd.parallel import backend as be

        label = be.native_backend(None, "cuda").last_algo

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
        dt = R.DTYPES[dtn]
        for m in ms:
            xs = shard_inputs(m, size, _seed(m), dt)
            x = xs[rank].clone().to(d)
            for op in ops:
                want = SR.reduce_scatter(xs, rank, op, dt)
                t = torch.full((m,), -7.5, dtype=dt, device=d)
                rop = dist.ReduceOp.SUM if op == "sum" else dist.ReduceOp.AVG
                if async_op:
                    want = finish(pd.reduce_scatter_compressed(t, x, rop, async_op=True), t, want, dt)
                else:
                    assert pd.reduce_scatter_compressed(t, x, rop) is None
                out[f"rs/{dtn}/{m}/{op}"] = [R.same(t, want) and torch.equal(x.cpu(), xs[rank]), digest(t), label()]
            # the gather: rank r contributes the first shard of its input
            shards = [v[:m] for v in xs]
            want = SR.all_gather(shards, dt)
            mine = shards[rank].clone().to(d)
            t = torch.full((m * size,), -7.5, dtype=dt, device=d)
            if async_op:
                want = finish(pd.all_gather_compressed(t, mine, async_op=True), t, want, dt)
            else:
                assert pd.all_gather_compressed(t, mine) is None
            out[f"ag/{dtn}/{m}"] = [R.same(t, want), digest(t), label()]
    dist.barrier()
    return out


def world1_and_errors(rank, size, device="cpu"):
    """World 1 copies input to output bit for bit; every error case, raised before any communication."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd import distributed as pd

    d = _dev(device)
    out = {}
    if size == 1:
        g1 = dist.new_group([rank])
        x = torch.from_numpy(R.edge_tensor()[0])[:777].clone()
        for dt in R.DTYPES.values():
            src = x.to(dt).to(d)
            for fn in (lambda o, i, **k: pd.reduce_scatter_compressed(o, i, dist.ReduceOp.AVG, **k),
                       pd.all_gather_compressed):
                dst = torch.zeros_like(src)
                fn(dst, src, group=g1)
                w = fn(dst, src, async_op=True)
                out[f"copied/{dt}/{len(out)}"] = bool(torch.equal(dst.view(torch.uint8), src.view(torch.uint8))
                                                      and w.is_completed() and w.wait())
        empty = torch.empty(0, device=d)
        out["empty"] = pd.reduce_scatter_compressed(empty, empty) is None and pd.all_gather_compressed(empty, empty) is None
    big, small = torch.ones(64 * size, device=d), torch.ones(64, device=d)

    def raises(kind, fn, *needles):
        try:
            fn()
            return False
        except kind as e:
            return all(n in str(e) for n in needles)

    rs, ag = pd.reduce_scatter_compressed, pd.all_gather_compressed
    out["op"] = raises(ValueError, lambda: rs(small, big, dist.ReduceOp.MAX), "MAX")
    out["op_prod"] = raises(ValueError, lambda: rs(small, big, dist.ReduceOp.PRODUCT), "PRODUCT")
    out["rs_wire"] = raises(ValueError, lambda: rs(small, big, wire="mxfp4"), "mxfp4")
    out["ag_wire"] = raises(ValueError, lambda: ag(big, small, wire="mxfp4"), "mxfp4")
    out["rs_dtype"] = raises(TypeError, lambda: rs(small.double(), big.double()), "float64")
    out["ag_dtype"] = raises(TypeError, lambda: ag(big.to(torch.int32), small.to(torch.int32)), "int32")
    out["rs_dtypes_differ"] = raises(TypeError, lambda: rs(small.to(torch.bfloat16), big), "float32", "bfloat16")
    out["ag_dtypes_differ"] = raises(TypeError, lambda: ag(big, small.to(torch.float16)), "float32", "float16")
    out["rs_numel"] = raises(ValueError, lambda: rs(small[:63], big), str(64 * size), str(63 * size))
    out["ag_numel"] = raises(ValueError, lambda: ag(big, small[:63]), str(64 * size), str(63 * size))
    out["rs_swapped"] = size == 1 or raises(ValueError, lambda: rs(big, small), "64")
    wide = torch.ones(64 * size, 2, device=d)
    out["rs_strided_output"] = raises(ValueError, lambda: rs(torch.ones(64, 2, device=d)[:, 0], big), "contiguous")
    out["ag_strided_output"] = raises(ValueError, lambda: ag(wide[:, 0], small), "contiguous")
    out["untouched"] = bool((big == 1).all() and (small == 1).all())
    dist.barrier()
    return out


def zero(rank, size, device="cuda", bucket_bytes=2048):
    """ShardedOptimizer(grad_wire, param_wire = mxfp8_e4m3) on the in-tree MLP: one backward, one
    step(). A hook records every raw gradient; the ranks' flat bucket gradients (padding as zeros) are
    exchanged uncompressed, and every bucket's grad_shard must equal _mx_shard_ref's AVG
    reduce-scatter of them. After the step the ranks' param_shards are exchanged uncompressed and
    `flat` must equal the reference all-gather of them. No optimizer arithmetic is compared."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd.models import MLP, synthetic_batch
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    d = _dev(device)
    torch.manual_seed(100)
    model = MLP().to(d)
    raw = {}
    params = [p for p in model.parameters() if p.requires_grad]
    hooks = [p.register_post_accumulate_grad_hook(lambda p: raw.__setitem__(id(p), p.grad.detach().clone()))
             for p in params]
    opt = ShardedOptimizer(model.parameters(), torch.optim.SGD, lr=0.05, bucket_bytes=bucket_bytes,
                           grad_wire="mxfp8_e4m3", param_wire="mxfp8_e4m3")
    x, y = synthetic_batch(64, device=d)
    shard = 64 // size
    xs, ys = x[rank * shard:(rank + 1) * shard], y[rank * shard:(rank + 1) * shard]
    torch.nn.functional.mse_loss(model(xs), ys).backward()
    (s,) = opt.spaces
    handles = sorted({type(b.work).__name__ for b in s.buckets})
    every = []
    # the reduce-scatters run on a side stream: the exchange below, other collectives of the same group
    # on the current stream, must not overlap any of them -- wait() orders the current stream
    for b in s.buckets:
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
    out = {"buckets": len(s.buckets), "handles": handles, "overlapped": opt.overlapped}
    shards = [torch.empty_like(s.param_shard) for _ in range(size)]
    dist.all_gather(shards, s.param_shard)
    shards = [t.cpu() for t in shards]
    for i, b in enumerate(s.buckets):
        want_g = SR.reduce_scatter(every[i], rank, "avg", s.dtype)
        want_p = SR.all_gather([t[b.soff:b.soff + b.shard] for t in shards], s.dtype)
        out[i] = [R.same(s.grad_shard[b.soff:b.soff + b.shard], want_g), R.same(s.flat[b.off:b.off + b.padded], want_p),
                  b.padded]
    # the master weights are not the dequantized wire: exact f32 of the optimizer's own arithmetic
    out["master_is_param_shard"] = bool(torch.equal(s.master.to(s.dtype), s.param_shard))
    out["digest"] = digest(s.flat)
    for h in hooks:
        h.remove()
    opt.remove_hooks()
    dist.barrier()
    return out
