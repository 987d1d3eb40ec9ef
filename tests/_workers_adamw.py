"""The f64 reference, the derived bound and the rank worker of the fused AdamW tests (docs/collectives.md "Fused
AdamW step", "The bound": the K_* below are the rounding counts derived there, plus one for the second-order terms)."""
import math

import torch

from tests._workers_clip import DTYPES, U, clip_data  # noqa: F401 - the tests' data comes from here too
from tests._workers_mx import _dev, digest

K_M, K_V, K_P = 4 + 1, 6 + 1, 15 + 1
TINY = 16 * 2.0 ** -149  # an operation that underflows errs by at most 2^-150 instead of relatively
HP = dict(lr=0.01, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.1)


class Chain:
    """AdamW in f64 from f64 scalars, step by step, with the bound on what the f32 sequence may differ by:
    `bm`, `bv`, `bp` after one step from exact inputs, `em`, `ev`, `ep` accumulated over the steps taken."""

    def __init__(self, p, m=None, v=None):
        self.p = p.double().clone()
        self.m = torch.zeros_like(self.p) if m is None else m.double().clone()
        self.v = torch.zeros_like(self.p) if v is None else v.double().clone()
        self.em, self.ev, self.ep = (torch.zeros_like(self.p) for _ in range(3))

    def step(self, g, step, coef=1.0, lr=None, betas=None, eps=None, weight_decay=None):
        (b1, b2), g = betas, g.double() * coef
        t1, t2 = b1 * self.m, (1 - b1) * g
        m, mag = t1 + t2, t1.abs() + t2.abs()
        v = b2 * self.v + (1 - b2) * g * g
        c2, size = 1 / math.sqrt(1 - b2 ** step), lr / (1 - b1 ** step)
        den = v.sqrt() * c2 + eps
        pd = self.p * (1 - lr * weight_decay)
        self.bm, self.bv = K_M * U * mag + TINY, K_V * U * v + TINY
        self.bp = K_P * U * (pd.abs() + size * mag / den) + TINY
        # what the earlier steps' errors do to this one, to first order
        dden = torch.where(v > 0, c2 * b2 * self.ev / (2 * v.sqrt()), torch.zeros_like(v))
        self.ep = self.ep * abs(1 - lr * weight_decay) + size / den * (b1 * self.em + m.abs() / den * dden) + self.bp
        self.em, self.ev = b1 * self.em + self.bm, b2 * self.ev + self.bv
        self.m, self.v, self.p = m, v, pd - size * m / den
        return self


def within(got, ref, bound):
    got = got.detach().double().cpu().reshape(-1)
    return bool(((got - ref.reshape(-1)).abs() <= bound.reshape(-1)).all())


def coef32(norm32, max_norm):
    """The clip coefficient as the kernel and ops.clip_scale_reference compute it: f32 operations from the f32 norm."""
    c = torch.tensor(max_norm, dtype=torch.float32) / (norm32.detach().cpu().to(torch.float32) + 1e-6)
    return float(torch.clamp(c, max=1.0))


def hand_grad(shape, rank, step, i):
    """Small integers over 8, different on every rank: sums and averages over two ranks are exact in bf16."""
    n = math.prod(shape)
    k = (torch.arange(n) * (3 + 2 * rank + i) + 5 * step + rank) % 33 - 16
    return (k.double() / 8).reshape(shape)


def zero(rank, size, device="cuda", max_norm=1.0):
    """Two steps of ShardedOptimizer(params, "adamw", max_grad_norm=1.0, overlap=False) on a tiny f32 and a tiny bf16
    model with hand-made gradients against Chain on their exact averages. {dtype: {check: ok, "flat": digest}}."""
    from pytorch_distributed_collective_communication_amd import ops
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    d, out = _dev(device), {}
    for dtn in ("float32", "bfloat16"):
        torch.manual_seed(7)
        ps = list(torch.nn.Linear(6, 5).to(d).to(DTYPES[dtn]).parameters())
        chains = [Chain(p.detach().cpu()) for p in ps]
        opt = ShardedOptimizer(ps, "adamw", overlap=False, max_grad_norm=max_norm, **HP)
        norm_ok = True
        for step in (1, 2):
            per_rank = [[hand_grad(p.shape, r, step, i) for i, p in enumerate(ps)] for r in range(size)]
            for p, g in zip(ps, per_rank[rank]):
                p.grad.copy_(g)
            opt.step()
            avg = [sum(gs) / size for gs in zip(*per_rank)]
            norm = math.sqrt(sum(float(a.square().sum()) for a in avg))
            norm_ok = norm_ok and abs(opt.grad_norm.item() - norm) <= (ops.SUMSQ_CHAIN + 1) * U * norm
            for c, a in zip(chains, avg):
                c.step(a, step, coef32(opt.grad_norm, max_norm), **HP)
        # the gathered parameters are the masters rounded once: bf16 keeps 8 significant bits, unit roundoff 2^-8
        half_ulp = 0.0 if dtn == "float32" else 2.0 ** -8
        out[dtn] = {"norm": norm_ok, "clips": norm > max_norm, "flat": digest(opt.spaces[0].flat),
                    "params": all(within(p, c.p, c.ep + half_ulp * (c.p.abs() + c.ep)) for p, c in zip(ps, chains))}
        opt.remove_hooks()
    return out


def world1(rank, size):
    """CPU, one rank. {check: ok}: three steps against torch.optim.AdamW in f64 within Chain's accumulated bound, then
    checkpoints saved after two steps by one kind of optimizer and continued for one step by the other."""
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    def fresh(kind, dt=torch.float32):
        torch.manual_seed(7)
        ps = list(torch.nn.Linear(6, 5).to(dt).parameters())
        return ps, (torch.optim.AdamW(ps, **HP) if kind is None else ShardedOptimizer(ps, kind, **HP))

    def step(ps, opt, n):
        for i, p in enumerate(ps):
            g = hand_grad(p.shape, 0, n, i).to(p.dtype)
            if p.grad is None:
                p.grad = g
            else:
                p.grad.copy_(g)
        opt.step()

    (ps, opt), (ps64, opt64) = fresh("adamw"), fresh(None, torch.float64)
    chains = [Chain(p.detach()) for p in ps]
    for n in (1, 2, 3):
        step(ps, opt, n), step(ps64, opt64, n)
        for i, c in enumerate(chains):
            c.step(hand_grad(c.p.shape, 0, n, i), n, **HP)
    out = {"three steps": all(within(p, q.detach(), c.ep) for p, q, c in zip(ps, ps64, chains)),
           "state bytes": opt.sharded_state_bytes() == 3 * 4 * opt.spaces[0].shard_total}
    for a, b in (("adamw", torch.optim.AdamW), (torch.optim.AdamW, "adamw")):  # save with a, continue with b
        (pa, oa), (pb, ob) = fresh(a), fresh(b)
        for n in (1, 2):
            step(pa, oa, n)
        ob.load_state_dict(oa.state_dict())
        step(pb, ob, 3)
        out[f"{a} -> {b}"] = all(within(p, q.detach(), c.ep) for p, q, c in zip(pb, ps64, chains))
    return out


def errors(rank, size):
    """The constructor's ValueErrors; {case: raised}."""
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    lin, out = (lambda: torch.nn.Linear(3, 2)), {}
    for name, params, kind, kw in [("unknown string", lin().parameters(), "adam", {}),
                                   ("bf16 master", lin().parameters(), "adamw", dict(master_dtype=torch.bfloat16)),
                                   ("f64 parameters", lin().double().parameters(), "adamw", {}),
                                   ("integer parameters", [torch.zeros(4, dtype=torch.int32)], "adamw", {})]:
        try:
            ShardedOptimizer(params, kind, **kw)
            out[name] = False
        except ValueError as e:
            out[name] = name != "unknown string" or "'adamw'" in str(e)
    return out
