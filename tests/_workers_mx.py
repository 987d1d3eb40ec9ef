"""Rank functions and inputs of the compressed all-reduce tests (tests/test_mx_cpu.py,
tests/test_mx_gpu.py). The reference is always tests/_mx_ref.py; results must equal it as values
(rtol = atol = 0, NaN where it has NaN) and be the same bytes on every rank."""
import hashlib

import numpy as np
import torch

from tests import _mx_ref as R


def _dev(device: str):
    if device == "cpu":
        return torch.device("cpu")
    return torch.device("cuda", torch.cuda.current_device())


def rank_inputs(n, world, seed, dtype=torch.float32):
    """One CPU tensor per rank. Random values over a few binades; in every third block one rank holds
    large values, another their negatives and the rest small ones (the pairing of tests/_exact.py), so
    any fold order but 0, 1, .., W-1 gives other values -- which rank is which rotates with the block."""
    rng = np.random.default_rng(seed)
    blocks = -(-n // R.BLOCK)
    xs = []
    # (2^14 against 2^-14: 28 binades apart, more than an f32 sum keeps, and inside f16's range)
    big = (rng.uniform(1.0, 2.0, (blocks, R.BLOCK)) * 2.0 ** 14).astype(np.float32)
    for r in range(world):
        x = (rng.standard_normal((blocks, R.BLOCK)) * np.ldexp(1.0, -rng.integers(0, 6, (blocks, R.BLOCK))))
        x = x.astype(np.float32)
        if world >= 2:
            for b in range(0, blocks, 3):
                pos, neg = (b // 3) % world, (b // 3 + 1 + (b // 3) // world % (world - 1)) % world
                if r == pos:
                    x[b] = big[b]
                elif r == neg:
                    x[b] = -big[b]
                else:
                    x[b] *= np.float32(2.0 ** -14)
        xs.append(torch.from_numpy(x.reshape(-1)[:n].copy()).to(dtype))
    return xs


def digest(t):
    return hashlib.sha1(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def all_reduce_cases(rank, size, device="cpu", numels=(1, 33), dtypes=("float32",), ops=("sum", "avg"),
                     async_op=False):
    """all_reduce_compressed of every (dtype, numel, op) against _mx_ref's fold.
    Returns {case: [equals the reference, digest of the result bytes, engine label]}."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd import distributed as pd

    d = _dev(device)
    label = lambda: ""  # noqa: E731
    if d.type == "cuda":
        from pytorch_distributed_collective_communication_amd.parallel import backend as be

        label = be.native_backend(None, "cuda").last_algo
    out = {}
    for dtn in dtypes:
        dt = R.DTYPES[dtn]
        for n in numels:
            xs = rank_inputs(n, size, 1000 + n % 9973, dt)
            for op in ops:
                want = R.all_reduce(xs, op, dt)
                t = xs[rank].clone().to(d)
                rop = dist.ReduceOp.SUM if op == "sum" else dist.ReduceOp.AVG
                if async_op:
                    # the call runs on a side stream; a multiply queued on the current stream after
                    # wait() must see the reduced values
                    w = pd.all_reduce_compressed(t, rop, async_op=True)
                    w.wait()
                    t.mul_(2.0)
                    want = (want.to(torch.float32) * 2.0).to(dt)
                    if d.type == "cuda":
                        torch.cuda.synchronize()
                    assert w.is_completed()
                else:
                    pd.all_reduce_compressed(t, rop)
                assert t.dtype == dt and t.numel() == n
                out[f"{dtn}/{n}/{op}"] = [R.same(t, want), digest(t), label()]
    dist.barrier()
    return out


def world1_and_errors(rank, size, device="cpu"):
    """World 1 leaves the tensor alone; the three error cases."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd import distributed as pd

    d = _dev(device)
    out = {}
    g1 = dist.new_group([rank]) if size == 1 else None
    if size == 1:
        x = torch.from_numpy(R.edge_tensor()[0])[:777].clone()
        for dt in R.DTYPES.values():
            t = x.to(dt).to(d)
            keep = t.clone()
            pd.all_reduce_compressed(t, dist.ReduceOp.AVG, group=g1)
            w = pd.all_reduce_compressed(t, async_op=True)
            out[f"unchanged/{dt}"] = bool(torch.equal(t.view(torch.uint8), keep.view(torch.uint8))
                                          and w.is_completed() and w.wait())
    t = torch.ones(64, device=d)

    def raises(kind, fn, needle):
        try:
            fn()
            return False
        except kind as e:
            return needle in str(e)

    out["op"] = raises(ValueError, lambda: pd.all_reduce_compressed(t, dist.ReduceOp.MAX), "MAX")
    out["op_prod"] = raises(ValueError, lambda: pd.all_reduce_compressed(t, dist.ReduceOp.PRODUCT), "PRODUCT")
    out["dtype"] = raises(TypeError, lambda: pd.all_reduce_compressed(t.to(torch.float64)), "float64")
    out["dtype_int"] = raises(TypeError, lambda: pd.all_reduce_compressed(t.to(torch.int32)), "int32")
    out["wire"] = raises(ValueError, lambda: pd.all_reduce_compressed(t, wire="mxfp4"), "mxfp4")
    out["untouched"] = bool((t == 1).all())
    dist.barrier()
    return out


def bucketer(rank, size, device="cuda", bucket_bytes=2048):
    """GradBucketer(wire="mxfp8_e4m3") on the in-tree MLP: one backward, one finish(). A hook
    registered before the bucketer's records every gradient as the bucketer packs it; the flat
    gradients of all ranks are exchanged uncompressed, and every bucket must equal _mx_ref's AVG fold
    of them. Returns {bucket index: [equal, digest]} and the bucket count."""
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
    buck = ddp.GradBucketer(model, bucket_bytes=bucket_bytes, wire="mxfp8_e4m3")
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
        want = R.all_reduce([e.cpu() for e in every], "avg", mine.dtype)
        got = torch.cat([p.grad.reshape(-1) for p in b.params])
        out[i] = [R.same(got, want) and R.same(b.flat, want), digest(got), b.numel]
    for h in hooks:
        h.remove()
    buck.remove()
    dist.barrier()
    return out
