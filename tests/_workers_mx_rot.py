"""Rank functions of the Hadamard-rotation tests (tests/test_mx_rot_cpu.py, tests/test_mx_rot_gpu.py). The
reference is always tests/_mx_rot_ref.py, run as a single-process simulation of every rank inside each rank;
results (and residuals) must equal it as values (rtol = atol = 0, NaN where it has NaN) and be the same bytes on
every rank. Inputs are those of the other wires' tests (tests/_workers_mx.py, _workers_mx_shard.py)."""
import numpy as np
import torch

from tests import _mx_rot_ref as R
from tests._workers_mx import _dev, digest, rank_inputs
from tests._workers_mx6 import _batch, _call_seed, _mlp, _residual, _sync, rank_seeds
from tests._workers_mx_shard import shard_inputs

ROT = "hadamard"
RSEED = 0xFACE0FF1234567  # the rotation seed of every case: above 2^32
OPS3 = ("sum", "avg", "sum")
CASES_PER_SIZE = 7  # keys of collective_cases per (wire, dtype, n)


def _seed(n):
    return 7000 + n % 9973


def collective_cases(rank, size, device="cpu", numels=(1, 33), dtypes=("float32",), async_op=False,
                     wires=tuple(R.WIRES)):
    """For every (wire, dtype, n) with rotation="hadamard": the three collectives plain (sum and avg), with
    residuals carried over three calls and stochastic (one seed per rank), against the reference composition.
    Returns {case: [everything equals the simulation, digest of the last result]}."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd import distributed as pd
    from pytorch_distributed_collective_communication_amd import ops

    d = _dev(device)
    rops = {"sum": dist.ReduceOp.SUM, "avg": dist.ReduceOp.AVG}

    def done(w):
        if async_op:
            assert type(w).__name__ == "CompressedWork"
            w.wait()
        else:
            assert w is None
        _sync(d)

    out = {}
    for wire in wires:
        kw = dict(wire=wire, async_op=async_op, rotation=ROT, rotation_seed=RSEED)
        cb = R.WIRES[wire].chunk_blocks
        for dtn in dtypes:
            dt = R.DTYPES[dtn]
            for n in numels:
                tag = f"{wire}/{dtn}/{n}"
                xs = rank_inputs(n, size, _seed(n), dt)
                ss = shard_inputs(n, size, _seed(n) + 17, dt)
                shards = [v[:n] for v in ss]
                # ---- plain
                ok_ar = ok_rs = True
                for op in ("sum", "avg"):
                    t = xs[rank].clone().to(d)
                    done(pd.all_reduce_compressed(t, rops[op], **kw))
                    ok_ar = ok_ar and R.same(t, R.all_reduce(xs, op, wire, RSEED, dt))
                    x = ss[rank].clone().to(d)
                    o = torch.full((n,), -7.5, dtype=dt, device=d)
                    done(pd.reduce_scatter_compressed(o, x, rops[op], **kw))
                    ok_rs = ok_rs and R.same(o, R.reduce_scatter(ss, op, wire, RSEED, dt)[rank]) \
                        and torch.equal(x.cpu(), ss[rank])
                out[f"ar/{tag}"] = [ok_ar, digest(t)]
                out[f"rs/{tag}"] = [ok_rs, digest(o)]
                g = torch.full((n * size,), -7.5, dtype=dt, device=d)
                done(pd.all_gather_compressed(g, shards[rank].clone().to(d), **kw))
                out[f"ag/{tag}"] = [R.same(g, R.all_gather(shards, wire, RSEED, dt)), digest(g)]
                # ---- error feedback over three calls: local residuals start random, owner residuals at zero
                sim_r = [_residual(n, _seed(n) + 31 * k) for k in range(size)]
                sim_o = [np.zeros(R.BLOCK * cb(n, size), dtype=np.float32) for _ in range(size)]
                assert sim_o[0].size == ops.mx_owner_residual_numel(n, size, wire=wire)
                res = torch.from_numpy(sim_r[rank].copy()).to(d)
                own = torch.from_numpy(sim_o[rank].copy()).to(d)
                sim_s = [_residual(n * size, _seed(n) + 77 + k) for k in range(size)]
                res_s = torch.from_numpy(sim_s[rank].copy()).to(d)
                ok_ar = ok_rs = True
                for c, op in enumerate(OPS3):
                    ys = rank_inputs(n, size, _seed(n) + 100 + c, dt)
                    want, sim_r, sim_o = R.all_reduce(ys, op, wire, RSEED, dt, rs=sim_r, r2s=sim_o)
                    t = ys[rank].clone().to(d)
                    done(pd.all_reduce_compressed(t, rops[op], residual=res, owner_residual=own, **kw))
                    ok_ar = ok_ar and R.same(t, want) and R.same_residual(res, sim_r[rank]) \
                        and R.same_residual(own, sim_o[rank])
                    zs = shard_inputs(n, size, _seed(n) + 200 + c, dt)
                    wants, sim_s = R.reduce_scatter(zs, op, wire, RSEED, dt, rs=sim_s)
                    o = torch.full((n,), -7.5, dtype=dt, device=d)
                    done(pd.reduce_scatter_compressed(o, zs[rank].clone().to(d), rops[op], residual=res_s, **kw))
                    ok_rs = ok_rs and R.same(o, wants[rank]) and R.same_residual(res_s, sim_s[rank])
                out[f"ar_ef/{tag}"] = [ok_ar and bool(res.any()), digest(t)]
                out[f"rs_ef/{tag}"] = [ok_rs, digest(o)]
                # ---- stochastic rounding, one seed per rank
                seeds = rank_seeds(size, n, 1)
                t = xs[rank].clone().to(d)
                done(pd.all_reduce_compressed(t, rops["avg"], rounding="stochastic", seed=seeds[rank], **kw))
                ok_ar = R.same(t, R.all_reduce(xs, "avg", wire, RSEED, dt, sr_seeds=seeds))
                o = torch.full((n,), -7.5, dtype=dt, device=d)
                done(pd.reduce_scatter_compressed(o, ss[rank].clone().to(d), rops["sum"], rounding="stochastic",
                                                  seed=seeds[rank], **kw))
                ok_rs = R.same(o, R.reduce_scatter(ss, "sum", wire, RSEED, dt, sr_seeds=seeds)[rank])
                out[f"ar_sr/{tag}"] = [ok_ar, digest(t)]
                g = torch.full((n * size,), -7.5, dtype=dt, device=d)
                done(pd.all_gather_compressed(g, shards[rank].clone().to(d), rounding="stochastic", seed=seeds[rank], **kw))
                out[f"rs_ag_sr/{tag}"] = [ok_rs and R.same(g, R.all_gather(shards, wire, RSEED, dt, sr_seeds=seeds)),
                                          digest(o)]
    dist.barrier()
    return out


def world1_and_errors(rank, size, device="cpu"):
    """World 1 leaves the data bit for bit with a rotation too; the rotation errors are raised before any
    communication (a second rank would hang otherwise: only this rank would have entered a collective)."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd import distributed as pd

    d = _dev(device)
    out = {}
    kw = dict(wire="mxfp4_e2m1", rotation=ROT, rotation_seed=RSEED)
    if size == 1:
        src = torch.from_numpy(R.edge_tensor("mxfp4_e2m1"))[:777].clone().to(d)
        t = src.clone()
        pd.all_reduce_compressed(t, dist.ReduceOp.AVG, **kw)
        w = pd.all_reduce_compressed(t, async_op=True, rounding="stochastic", seed=7, **kw)
        out["unchanged"] = bool(torch.equal(t.view(torch.uint8), src.view(torch.uint8)) and w.is_completed() and w.wait())
        for name, fn in (("rs", lambda a, b: pd.reduce_scatter_compressed(a, b, dist.ReduceOp.AVG, **kw)),
                         ("ag", lambda a, b: pd.all_gather_compressed(a, b, **kw))):
            dst = torch.zeros_like(src)
            fn(dst, src)
            out[f"copied/{name}"] = bool(torch.equal(dst.view(torch.uint8), src.view(torch.uint8)))
    big, small = torch.ones(64 * size, device=d), torch.ones(64, device=d)

    def raises(kind, fn, *needles):
        try:
            fn()
            return False
        except kind as e:
            return all(n in str(e) for n in needles)

    calls = (("ar", lambda **k: pd.all_reduce_compressed(small, wire="mxfp4_e2m1", **k)),
             ("rs", lambda **k: pd.reduce_scatter_compressed(small, big, wire="mxfp4_e2m1", **k)),
             ("ag", lambda **k: pd.all_gather_compressed(big, small, wire="mxfp4_e2m1", **k)))
    for name, fn in calls:
        out[f"{name}_name"] = raises(ValueError, lambda: fn(rotation="haar"), "'haar'", "hadamard")
        out[f"{name}_seed_high"] = raises(ValueError, lambda: fn(rotation=ROT, rotation_seed=1 << 64), "2^64")
        out[f"{name}_seed_low"] = raises(ValueError, lambda: fn(rotation_seed=-1), "2^64")
        out[f"{name}_seed_type"] = raises(TypeError, lambda: fn(rotation=ROT, rotation_seed=1.5), "float")
    out["untouched"] = bool((big == 1).all() and (small == 1).all())
    dist.barrier()
    return out


N_ERRORS = 3 * 4 + 1


def bucketer(rank, size, device="cuda", wire="mxfp4_e2m1", mode="ef", bucket_bytes=2048):
    """GradBucketer(wire=..., rotation="hadamard") on the in-tree MLP, three steps; `mode`: "plain", "ef" or "sr".
    After every step each bucket (and in "ef" both of its residuals) must equal the simulation fed with the
    ranks' raw gradients. Returns {"buckets", "handles", "steps": [{bucket: [ok, digest]}]}."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd.parallel import ddp
    from tests._workers_mx6 import SEED

    d = _dev(device)
    model = _mlp(d)
    raw = {}
    params = [p for p in model.parameters() if p.requires_grad]
    hooks = [p.register_post_accumulate_grad_hook(lambda p: raw.__setitem__(id(p), p.grad.detach().clone()))
             for p in params]
    extra = {"ef": dict(error_feedback=True), "sr": dict(rounding="stochastic", seed=SEED), "plain": {}}[mode]
    buck = ddp.GradBucketer(model, bucket_bytes=bucket_bytes, wire=wire, rotation=ROT, rotation_seed=RSEED, **extra)
    nb = len(buck.buckets)
    cb = R.WIRES[wire].chunk_blocks
    sim_r = [[np.zeros(b.numel, dtype=np.float32) for _ in range(size)] for b in buck.buckets]
    sim_o = [[np.zeros(R.BLOCK * cb(b.numel, size), dtype=np.float32) for _ in range(size)] for b in buck.buckets]
    out = {"buckets": nb, "steps": []}
    for step in range(3):
        model.zero_grad(set_to_none=True)
        xs, ys = _batch(rank, size, step, d)
        torch.nn.functional.mse_loss(model(xs), ys).backward()
        out["handles"] = sorted({type(b.work).__name__ for b in buck.buckets})
        buck.finish()
        _sync(d)
        got_step = {}
        for i, b in enumerate(buck.buckets):
            mine = torch.cat([raw[id(p)].reshape(-1) for p in b.params])
            every = [torch.empty_like(mine) for _ in range(size)]
            dist.all_gather(every, mine)
            every = [e.cpu() for e in every]
            got = torch.cat([p.grad.reshape(-1) for p in b.params])
            ok = True
            if mode == "ef":
                want, sim_r[i], sim_o[i] = R.all_reduce(every, "avg", wire, RSEED, mine.dtype, rs=sim_r[i], r2s=sim_o[i])
                ok = R.same_residual(b.residual, sim_r[i][rank]) and R.same_residual(b.owner_residual, sim_o[i][rank]) \
                    and bool(b.residual.any())
            elif mode == "sr":
                want = R.all_reduce(every, "avg", wire, RSEED, mine.dtype, sr_seeds=[_call_seed(step, nb, i)] * size)
            else:
                want = R.all_reduce(every, "avg", wire, RSEED, mine.dtype)
            got_step[i] = [ok and R.same(got, want) and R.same(b.flat, want), digest(got)]
        out["steps"].append(got_step)
    for h in hooks:
        h.remove()
    buck.remove()
    dist.barrier()
    return out


def zero(rank, size, device="cuda", grad_wire="mxfp4_e2m1", param_wire="mxfp6_e2m3", mode="plain", bucket_bytes=2048):
    """ShardedOptimizer with both wires rotated on the in-tree MLP, three steps; `mode`: "plain" or "ef"
    (grad_error_feedback=True). Every bucket's grad_shard must equal the simulated rotated AVG reduce-scatter of the
    ranks' raw flat gradients (in "ef" the residual too), and `flat` after the step the rotated reference all-gather
    of the ranks' param_shards. Nothing of the rotation is in state_dict()."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    d = _dev(device)
    model = _mlp(d)
    raw = {}
    params = [p for p in model.parameters() if p.requires_grad]
    hooks = [p.register_post_accumulate_grad_hook(lambda p: raw.__setitem__(id(p), p.grad.detach().clone()))
             for p in params]
    opt = ShardedOptimizer(model.parameters(), torch.optim.SGD, lr=0.05, bucket_bytes=bucket_bytes, grad_wire=grad_wire,
                           param_wire=param_wire, grad_rotation=ROT, param_rotation=ROT, rotation_seed=RSEED,
                           grad_error_feedback=mode == "ef")
    (s,) = opt.spaces
    nb = len(s.buckets)
    sim = [[np.zeros(b.padded, dtype=np.float32) for _ in range(size)] for b in s.buckets]
    out = {"buckets": nb, "steps": []}
    for step in range(3):
        opt.zero_grad()
        xs, ys = _batch(rank, size, step, d)
        torch.nn.functional.mse_loss(model(xs), ys).backward()
        out["handles"] = sorted({type(b.work).__name__ for b in s.buckets})
        for b in s.buckets:  # (an exchange of the test's own must not overlap the side stream's reduce-scatters)
            if b.work is not None:
                b.work.wait()
        every = []
        for b in s.buckets:
            flat = torch.zeros(b.padded, dtype=s.dtype, device=d)
            for i in b.idx:
                p, o = s.params[i], s.offsets[i] - b.off
                flat[o:o + p.numel()] = raw[id(p)].reshape(-1)
            got = [torch.empty_like(flat) for _ in range(size)]
            dist.all_gather(got, flat)
            every.append([g.cpu() for g in got])
        opt.step()
        _sync(d)
        shards = [torch.empty_like(s.param_shard) for _ in range(size)]
        dist.all_gather(shards, s.param_shard)
        shards = [t.cpu() for t in shards]
        got_step = {}
        for i, b in enumerate(s.buckets):
            ok_r = True
            if mode == "ef":
                wants, sim[i] = R.reduce_scatter(every[i], "avg", grad_wire, RSEED, s.dtype, rs=sim[i])
                ok_r = R.same_residual(s.grad_residual[b.off:b.off + b.padded], sim[i][rank])
            else:
                wants = R.reduce_scatter(every[i], "avg", grad_wire, RSEED, s.dtype)
            want_p = R.all_gather([t[b.soff:b.soff + b.shard] for t in shards], param_wire, RSEED, s.dtype)
            got_step[i] = [R.same(s.grad_shard[b.soff:b.soff + b.shard], wants[rank]) and ok_r,
                           R.same(s.flat[b.off:b.off + b.padded], want_p)]
        got_step["digest"] = digest(s.flat)
        out["steps"].append(got_step)
    out["state_keys"] = sorted(k for k in opt.state_dict() if "rot" in k)
    for h in hooks:
        h.remove()
    opt.remove_hooks()
    dist.barrier()
    return out
