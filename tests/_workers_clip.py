"""Data, tolerances and rank workers of the gradient-clipping tests (docs/collectives.md "Gradient clipping")."""
import math

import torch

from tests._workers_mx import _dev, digest
from tests._workers_mx_ef import _batch, _mlp, _sync

DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
_MANT = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}  # stored mantissa bits, smallest normal exponent
U = 2.0 ** -24


def clip_data(n, seed, dtype):
    """Heavy-tailed values, randn * exp(randn), as a CPU tensor of `dtype`."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * torch.randn(n, generator=g).exp()).to(dtype)


def coef_ref(norm, max_norm):
    """The clip coefficient in f64 from the norm."""
    c = max_norm / (norm + 1e-6)
    return c if c < 1 or math.isnan(c) else 1.0


def scaled_ok(got, ref64):
    """`got` against the f64 product: f32 outputs within a relative 8 * 2^-24 (the f32 sqrt, add, divide and multiply
    round at most 8 ulp away), bf16 / f16 outputs within one ulp of that dtype at the reference."""
    got, ref64 = got.detach().cpu(), ref64.cpu()
    if got.dtype == torch.float32:
        tol = 8 * U * ref64.abs()
    else:
        mant, emin = _MANT[got.dtype]
        e = torch.frexp(ref64.abs())[1] - 1  # floor(log2 |ref|)
        tol = torch.ldexp(torch.ones_like(ref64), e.clamp(min=emin) - mant)
    return bool(((got.double() - ref64).abs() <= tol).all())


def _steps(model, opt, rank, size, d, dt, n=2):
    for step in range(n):
        opt.zero_grad()
        xs, ys = _batch(rank, size, step, d)
        torch.nn.functional.mse_loss(model(xs.to(dt)), ys.to(dt)).backward()
        opt.step()
        _sync(d)


def zero(rank, size, device="cuda", max_norm=0.05, bucket_bytes=2048):
    """ShardedOptimizer(max_grad_norm=...) on the in-tree MLP with SGD, for f32 and bf16 parameters, uncompressed and
    on the mxfp4_e2m1 gradient wire. The shards are copied as _clip() finds them and exchanged uncompressed after the
    step. Returns {case: {check: ok, "norm": the bits of grad_norm}}."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd import ops
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    d, out = _dev(device), {}
    bound = (ops.SUMSQ_CHAIN + 1) * U  # of the sum; the norm's error is half of it plus one f32 rounding
    for dtn, wire in [(a, w) for a in ("float32", "bfloat16") for w in (None, "mxfp4_e2m1")]:
        dt, kw = DTYPES[dtn], dict(lr=0.05, bucket_bytes=bucket_bytes, grad_wire=wire)
        model = _mlp(d).to(dt)
        opt = ShardedOptimizer(model.parameters(), torch.optim.SGD, max_grad_norm=max_norm, **kw)
        assert opt.grad_norm is None
        snap, clip = [], opt._clip
        opt._clip = lambda: (snap.__setitem__(slice(None), [s.grad_shard.clone() for s in opt.spaces]), clip())
        _steps(model, opt, rank, size, d, dt, 1)
        (s,), (mine,) = opt.spaces, snap
        every = [torch.empty_like(mine) for _ in range(size)]
        dist.all_gather(every, mine)
        norm = math.sqrt(sum(float(t.double().square().sum()) for t in every))
        got = opt.grad_norm
        after = s.master.grad.double().square().sum().reshape(1)
        dist.all_reduce(after)
        out[f"{dtn} {wire}"] = {
            "clips": max_norm < norm / 4, "norm": got.item().hex(),
            "norm_ok": got.dim() == 0 and got.dtype == torch.float32 and abs(got.item() - norm) <= bound * norm,
            # the coefficient from the f32 norm the kernel used: what is left is one add, one divide, one multiply
            "grad_ok": scaled_ok(s.master.grad, mine.double() * coef_ref(got.item(), max_norm)),
            "clipped": math.sqrt(after.item()) <= max_norm * (1 + 2.0 ** -20),
            "state": not any("norm" in k or "clip" in k for k in opt.state_dict()),
        }
        opt.remove_hooks()
        flats = []
        for extra in ({"max_grad_norm": 1e30}, {}):  # a coefficient of 1: bit for bit the optimizer without it
            model = _mlp(d).to(dt)
            opt = ShardedOptimizer(model.parameters(), torch.optim.SGD, **kw, **extra)
            _steps(model, opt, rank, size, d, dt)
            flats.append(digest(opt.spaces[0].flat))
            opt.remove_hooks()
        out[f"{dtn} {wire}"]["same"] = flats[0] == flats[1]
    dist.barrier()
    return out


def errors(rank, size, device="cpu"):
    """The constructor's ValueErrors; {case: raised}."""
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    d, out = _dev(device), {}
    cases = [(f"value {v!r}", torch.float32, dict(max_grad_norm=v))
             for v in (0, -1.0, float("inf"), float("nan"), True, "1")]
    cases += [("f64 parameters", torch.float64, dict(max_grad_norm=1.0)),
              ("bf16 master of f32", torch.float32, dict(max_grad_norm=1.0, master_dtype=torch.bfloat16)),
              ("f16 master of bf16", torch.bfloat16, dict(max_grad_norm=1.0, master_dtype=torch.float16))]
    for name, dt, kw in cases:
        try:
            ShardedOptimizer(_mlp(d).to(dt).parameters(), torch.optim.SGD, lr=0.05, **kw).remove_hooks()
            out[name] = False
        except ValueError:
            out[name] = True
    ShardedOptimizer(_mlp(d).parameters(), torch.optim.SGD, lr=0.05, max_grad_norm=2).remove_hooks()
    return out
