"""Shared by tests/test_mx_list_cpu.py and tests/test_mx_list_gpu.py (docs/collectives.md "Tensor-list layout"):
the pad-and-concatenate function that turns a list into the tensor the numpy references are applied to, the
references' quantize under one signature, and the rank functions. Values must equal the references exactly
(rtol = atol = 0) and be the same bytes on every rank."""
import numpy as np
import torch

from tests import _mx_ef_ref as EF
from tests import _mx_rot_ref as R
from tests import _mx_sr_ref as SR
from tests._workers_mx import _dev, digest, rank_inputs
from tests._workers_mx6 import _batch, _mlp, _sync

R6 = R.R6
LISTS = {"one": (1,), "ragged": (31, 33), "empty": (32, 0, 1, 4097), "many": (5,) * 70,
         # a span is 1024 vectors, 4096 f32 or 8192 16-bit elements of the padded concatenation: the long tensor
         # of "cross" runs over both boundaries, tensors of "exact" end on them
         "cross": (100, 8300), "exact": (33, 4032, 4096, 7)}


def pad_cat(xs):
    """The padded concatenation: every tensor zero-padded to a multiple of 32 elements."""
    return torch.cat([torch.nn.functional.pad(x.reshape(-1), (0, -x.numel() % 32)) for x in xs])


def ref_quantize(x, world, wire, res=None, sr=None, rot=None):
    """The numpy references' dealt quantize of flat f32 `x`: res -> (wire, new residual); sr = (seed, stream)."""
    if rot is not None:
        return R.quantize(x, world, wire, rot, res, None if sr is None else (sr[0], sr[1], 0))
    if res is not None:
        return R6.quantize_ef(x, res, world) if wire == R6.WIRE else EF.quantize(x, res, world, wire)
    if sr is not None:
        return R6.quantize(x, world, (sr[0], sr[1], 0)) if wire == R6.WIRE else SR.quantize(x, world, wire, sr[0], sr[1], 0)
    return R.WIRES[wire].quantize(x, world)


def collective(rank, size, device="cpu", async_op=False, names=("ragged", "empty")):
    """all_reduce_compressed of a list, for every wire: equals the reference all-reduce of the ranks' padded
    concatenations, slice by slice, and all_reduce_compressed of this rank's padded concatenation.
    Returns {case: [ok, digest]}."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd import distributed as pd

    d = _dev(device)
    out = {}
    for wire in R.WIRES:
        for name in names:
            for dtn, dt in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
                per = [rank_inputs(n, size, 50 + i, dt) for i, n in enumerate(LISTS[name])]  # [tensor][rank]
                cats = [pad_cat([t[r] for t in per]) for r in range(size)]
                want = R.WIRES[wire].all_reduce(cats, "avg", dt)
                xs = [t[rank].clone().to(d) for t in per]
                flat = cats[rank].clone().to(d)
                for what in (xs, flat):
                    w = pd.all_reduce_compressed(what, dist.ReduceOp.AVG, wire=wire, async_op=async_op)
                    assert (type(w).__name__ == "CompressedWork") if async_op else w is None
                    if async_op:
                        w.wait()
                    _sync(d)
                got = pad_cat(xs)
                out[f"{wire}/{name}/{dtn}"] = [R.same(got, want) and torch.equal(got.cpu(), flat.cpu()), digest(got)]
    dist.barrier()
    return out


def bucketer(rank, size, device="cuda", wire="mxfp4_e2m1"):
    """GradBucketer(wire=, in_place=True, error_feedback=True) on the in-tree MLP, two steps: the gradients equal
    the list reference fed with the ranks' raw gradients, both residuals too, and no bucket owns a flat tensor."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd import ops
    from pytorch_distributed_collective_communication_amd.parallel import ddp

    d = _dev(device)
    model = _mlp(d)
    raw = {}
    params = [p for p in model.parameters() if p.requires_grad]
    hooks = [p.register_post_accumulate_grad_hook(lambda p: raw.__setitem__(id(p), p.grad.detach().clone()))
             for p in params]
    buck = ddp.GradBucketer(model, bucket_bytes=2048, wire=wire, in_place=True, error_feedback=True)
    out = {"buckets": len(buck.buckets), "flat": [b.flat is None for b in buck.buckets], "steps": []}
    sim_r = [[np.zeros(ops.mx_list_numel([p.numel() for p in b.params]), dtype=np.float32) for _ in range(size)]
             for b in buck.buckets]
    sim_o = [[np.zeros(ops.mx_owner_residual_numel(s[0].size, size, wire=wire), dtype=np.float32) for _ in range(size)]
             for s in sim_r]
    for step in range(2):
        model.zero_grad(set_to_none=True)
        xs, ys = _batch(rank, size, step, d)
        torch.nn.functional.mse_loss(model(xs), ys).backward()
        out["handles"] = sorted({type(b.work).__name__ for b in buck.buckets})
        buck.finish()
        _sync(d)
        oks = []
        for i, b in enumerate(buck.buckets):
            mine = pad_cat([raw[id(p)] for p in b.params])
            every = [torch.empty_like(mine) for _ in range(size)]
            dist.all_gather(every, mine)
            want, sim_r[i], sim_o[i] = EF.all_reduce([e.cpu() for e in every], sim_r[i], sim_o[i], "avg", wire, mine.dtype)
            oks.append(R.same(pad_cat([p.grad for p in b.params]), want) and bool(b.residual.any())
                       and R.same_residual(b.residual, sim_r[i][rank])  # (no rotation: the padding's is +0 in both)
                       and R.same_residual(b.owner_residual, sim_o[i][rank]))
        out["steps"].append(oks)
    for h in hooks:
        h.remove()
    buck.remove()
    dist.barrier()
    return out
