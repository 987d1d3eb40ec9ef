"""Data, checks and rank workers of the 8-bit AdamW state tests (docs/collectives.md "8-bit AdamW state").

The master is held to the f32 step's own bound (tests/_workers_adamw.py K_P) against Chain started from the unpacked
state: v0 = s0 * s0 is rounded before the chain starts, as in the kernel. A stored moment x is held to
2^-4 |x| + 2 * 2^(e - 10) plus its f32 bound: half an e4m3 ulp of a normal code, and twice half a subnormal step at
the block's scale exponent e (the documented rule on the reference's amax) for a scale one off at a binade boundary
and for the never-zero rule, whose error stays below 2^(e - 9)."""
import functools

import torch

from tests._workers_adamw import HP, U, Chain, clip_data, coef32, hand_grad, within
from tests._workers_clip import DTYPES
from tests._workers_mx import _dev, digest

FMT = "mxfp8_e4m3"
ZERO, TINY_AT = slice(64, 96), 40  # a block of g = m = v = 0; an element 2^-30 of its block's amax


def _ops():
    from pytorch_distributed_collective_communication_amd import ops

    return ops


@functools.lru_cache(maxsize=None)
def data(n, dtn):
    """CPU inputs of one step: heavy-tailed gradient and master, a plausible state, packed."""
    x = {"grad": DTYPES[dtn], "master": torch.float32, "exp_avg": torch.float32, "exp_avg_sq": torch.float32}
    x = {k: clip_data(n, 10 * n + i, dt) for i, (k, dt) in enumerate(x.items())}
    x["exp_avg"] *= 0.1
    x["exp_avg_sq"] = x["exp_avg_sq"].square() * 0.01
    for k in ("grad", "exp_avg", "exp_avg_sq"):
        x[k][ZERO] = 0
        if n > TINY_AT:
            x[k][TINY_AT] = x[k][32:64].abs().max() * 2.0 ** (-60 if k == "exp_avg_sq" else -30)
    x["exp_avg"], x["exp_avg_sq"] = _ops().adamw_state_pack(x["exp_avg"], x["exp_avg_sq"])
    return x


def stored_tol(ref):
    """2^-4 |x| + 2 * 2^(e - 10) per element of the f64 reference."""
    ops, n = _ops(), ref.numel()
    rb = torch.zeros(32 * ops.mx_chunk_blocks(n, 1))
    rb[:n] = ref.float()
    e = ops._mx_block_scale(rb.view(-1, 32), ops._MX_FORMATS[FMT])[0].double()
    return ref.abs() / 16 + 2 * torch.exp2(e - 10).repeat_interleave(32)[:n]


def check_step(got, x, hp, step, coef=1.0, keep=None):
    """`got` (master and the packed state after one step from `x`) against Chain; `keep`: the elements compared."""
    ops, n = _ops(), x["grad"].numel()
    c = Chain(x["master"], *ops.adamw_state_unpack(x["exp_avg"], x["exp_avg_sq"], n)).step(x["grad"], step, coef, **hp)
    s = c.v.sqrt()
    bs = torch.where(c.v > 0, c.bv / (2 * s).clamp(min=1e-300), c.bv.sqrt()) + U * s
    keep = torch.ones(n, dtype=torch.bool) if keep is None else keep
    for name, g, ref, bound in (("master", got["master"], c.p, c.bp),
                                ("exp_avg", ops.mx_dequantize_reference(got["exp_avg"], n), c.m, c.bm + stored_tol(c.m)),
                                ("exp_avg_sq", ops.mx_dequantize_reference(got["exp_avg_sq"], n), s, bs + stored_tol(s))):
        err = (g.double() - ref).abs()
        print(name, float((err / bound)[keep].max()))
        assert bool((err <= bound)[keep].all()), name
    return c


def check_exact(got, n):
    """The zero block and the tiny element of `data`."""
    cb = _ops().mx_chunk_blocks(n, 1)
    for k in ("exp_avg", "exp_avg_sq"):
        if n >= ZERO.stop:
            assert got[k][32 * cb + 2] == 127 and not got[k][ZERO].any(), k
    if n > TINY_AT:
        assert got["exp_avg_sq"][TINY_AT] == 1 and bool(got["master"][TINY_AT].isfinite())


def zero(rank, size, device="cuda"):
    """Two steps of ShardedOptimizer(ps, "adamw", state_format=FMT, max_grad_norm=1.0, overlap=False) on a tiny f32
    and a tiny bf16 model with hand-made gradients. Step 1 (from zeros: nothing quantized is read) against the
    accumulated bound of Chain on the exact averages, step 2 against one Chain step from this rank's own unpacked
    state after step 1. {dtype: {check: ok, "flat": digest}}."""
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    ops, d, out = _ops(), _dev(device), {}
    for dtn in ("float32", "bfloat16"):
        torch.manual_seed(7)
        ps = list(torch.nn.Linear(6, 5).to(d).to(DTYPES[dtn]).parameters())
        chains = [Chain(p.detach().cpu()) for p in ps]
        opt = ShardedOptimizer(ps, "adamw", state_format=FMT, max_grad_norm=1.0, overlap=False, **HP)
        (s,), half_ulp, res = opt.spaces, (0.0 if dtn == "float32" else 2.0 ** -8), {}
        for step in (1, 2):
            per_rank = [[hand_grad(p.shape, r, step, i) for i, p in enumerate(ps)] for r in range(size)]
            for p, g in zip(ps, per_rank[rank]):
                p.grad.copy_(g)
            before = (s.master.cpu().clone(), *(t.cpu() for t in ops.adamw_state_unpack(
                opt.inner.state[0]["exp_avg"], opt.inner.state[0]["exp_avg_sq"], s.shard_total)))
            opt.step()
            coef = coef32(opt.grad_norm, 1.0)
            if step == 1:
                for c, a in zip(chains, [sum(gs) / size for gs in zip(*per_rank)]):
                    c.step(a, 1, coef, **HP)
                res["step 1"] = all(within(p, c.p, c.ep + half_ulp * (c.p.abs() + c.ep)) for p, c in zip(ps, chains))
            else:
                c = Chain(*before).step(s.grad_shard.cpu(), 2, coef, **HP)
                res["step 2"] = within(s.master, c.p, c.bp) and \
                    within(s.param_shard, c.p, c.bp + half_ulp * (c.p.abs() + c.bp))
        res["bytes"] = opt.sharded_state_bytes() == 4 * s.shard_total + 2 * ops.mx_wire_bytes(s.shard_total, 1)
        out[dtn] = {**res, "flat": digest(s.flat)}
        opt.remove_hooks()
    return out


def world1(rank, size):
    """CPU, one rank: `zero`, checkpoints after two steps continued for one step by the other kind of optimizer
    (against one Chain step from the state the continuing optimizer holds after loading), and the ValueErrors."""
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    ops, out = _ops(), {f"{k} {dtn}": v for dtn, r in zero(rank, size, "cpu").items() for k, v in r.items() if k != "flat"}

    def fresh(packed):
        torch.manual_seed(7)
        ps = list(torch.nn.Linear(6, 5).parameters())
        return ps, (ShardedOptimizer(ps, "adamw", state_format=FMT, **HP) if packed else ShardedOptimizer(ps, torch.optim.AdamW, **HP))

    def step(ps, opt, n):
        for i, p in enumerate(ps):
            p.grad.copy_(hand_grad(p.shape, 0, n, i))
        opt.step()

    for a in (True, False):  # save with a, continue with the other
        (pa, oa), (pb, ob) = fresh(a), fresh(not a)
        step(pa, oa, 1), step(pa, oa, 2)
        ob.load_state_dict(oa.state_dict())
        (s,) = ob.spaces
        st = ob.inner.state[s.master if a else 0]
        m, v = (st["exp_avg"], st["exp_avg_sq"]) if a else ops.adamw_state_unpack(st["exp_avg"], st["exp_avg_sq"], s.shard_total)
        c = Chain(s.master, m, v)
        step(pb, ob, 3)
        c.step(s.grad_shard, 3, **HP)
        out["8-bit -> AdamW" if a else "AdamW -> 8-bit"] = within(s.master, c.p, c.bp)
    for name, kind, fmt in (("unknown format", "adamw", "mxfp4_e2m1"), ("inner class", torch.optim.AdamW, FMT)):
        try:
            ShardedOptimizer(torch.nn.Linear(3, 2).parameters(), kind, state_format=fmt)
            out[name] = False
        except ValueError:
            out[name] = True
    return out
