"""The fused AdamW step on the GPU (docs/collectives.md "Fused AdamW step"): ops.adamw_step against the f64 formula
evaluated from f64 scalars, and ShardedOptimizer(params, "adamw") with two ranks sharing GPU 0.

Tolerance: "The bound" of that section, k 2^-24 times the magnitudes of the terms with k = 4 (exp_avg), 6 (exp_avg_sq)
and 15 (master) f32 roundings, the eight scalars' own among them, plus one each for the second-order terms:
tests/_workers_adamw.py K_M, K_V, K_P. param_out must be the kernel's own master cast with .to(dtype), bit for bit."""
import functools

import pytest
import torch

from tests import _workers_adamw as W
from tests.test_backend_gpu import _gpu_launch
from tests.test_clip_gpu import DEV, _intact, _view

pytestmark = pytest.mark.gpu
SPAN = 4096  # elements a workgroup takes per trip
NUMELS = (1, 3, 4, 1023, 1024, 1025, SPAN - 1, SPAN, SPAN + 1)
SIDES = ("grad", "master", "exp_avg", "exp_avg_sq", "param_out")


def _ops():
    from pytorch_distributed_collective_communication_amd import ops

    return ops


@functools.lru_cache(maxsize=None)
def _data(n, dtn):
    """CPU inputs: heavy-tailed gradient and master, a plausible state, and where n allows a block of g = 0, v = 0."""
    x = {"grad": W.DTYPES[dtn], "master": torch.float32, "exp_avg": torch.float32, "exp_avg_sq": torch.float32}
    x = {k: W.clip_data(n, 10 * n + i, dt) for i, (k, dt) in enumerate(x.items())}
    x["exp_avg"] *= 0.1
    x["exp_avg_sq"] = x["exp_avg_sq"].square() * 0.01
    x["grad"][5:9], x["exp_avg_sq"][5:9] = 0, 0
    return x


def _run(n, dtn, pdn, step=1, wd=0.1, off_side=None, total=None, max_norm=None, max_blocks=0):
    """One call on guarded views (`off_side`: that view starts one element past a 16-byte boundary). Checks the guard
    bands, the untouched gradient and the round-once contract; returns the CPU results and the inputs."""
    ops, x = _ops(), _data(n, dtn)
    if pdn is not None:
        x = {**x, "param_out": torch.zeros(n, dtype=W.DTYPES[pdn])}
    off = {k: int(k == off_side) for k in x}
    views = {k: _view(t, off[k]) for k, t in x.items()}
    t = {k: v[1] for k, v in views.items()}
    hp = {**W.HP, "weight_decay": wd}
    ops.adamw_step(t["grad"], t["master"], t["exp_avg"], t["exp_avg_sq"], step=step, param_out=t.get("param_out"),
                   total=None if total is None else torch.tensor([total], dtype=torch.float64, device=DEV),
                   max_norm=max_norm, max_blocks=max_blocks, **hp)
    assert all(_intact(views[k][0], t[k], off[k]) for k in x), "guard bands"
    got = {k: v.cpu() for k, v in t.items()}
    assert torch.equal(got["grad"], x["grad"])
    if pdn is not None and not got["master"].isnan().any():
        assert torch.equal(got["param_out"], got["master"].to(W.DTYPES[pdn])), "param_out is the master rounded once"
    return got, x, hp


def _check(got, x, hp, step, coef=1.0):
    c = W.Chain(x["master"], x["exp_avg"], x["exp_avg_sq"]).step(x["grad"], step, coef, **hp)
    for k, ref, bound in (("exp_avg", c.m, c.bm), ("exp_avg_sq", c.v, c.bv), ("master", c.p, c.bp)):
        assert W.within(got[k], ref, bound), (k, float((got[k].double() - ref).abs().max()), float(bound.max()))
    return c


@pytest.mark.parametrize("n,max_blocks", [(n, 0) for n in NUMELS] + [(2 * SPAN + 5, 1)])
@pytest.mark.parametrize("dtn", list(W.DTYPES))
def test_sizes_against_f64_and_the_cpu_reference(dtn, n, max_blocks):
    got, x, hp = _run(n, dtn, dtn, max_blocks=max_blocks)
    c = _check(got, x, hp, 1)
    ref = {k: v.clone() for k, v in x.items()}
    _ops().adamw_step_reference(ref["grad"], ref["master"], ref["exp_avg"], ref["exp_avg_sq"], step=1, **hp)
    for k, bound in (("exp_avg", c.bm), ("exp_avg_sq", c.bv), ("master", c.bp)):
        assert W.within(got[k], ref[k].double(), bound), k


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("dtn,pdn", [(g, p) for g in W.DTYPES for p in dict.fromkeys((None, g, "float32"))])
def test_dtypes_steps_decay_and_misaligned_views(dtn, pdn, step, wd):
    base, x, hp = _run(1025, dtn, pdn, step, wd)
    _check(base, x, hp, step)
    for side in SIDES[:5 if pdn else 4]:  # the element path: the same bits
        got = _run(1025, dtn, pdn, step, wd, off_side=side)[0]
        assert all(torch.equal(got[k], base[k]) for k in base), side


@pytest.mark.parametrize("total,max_norm", [(0.25, 1.0), (4e4, 1.0), (float("inf"), 1.0), (float("nan"), 1.0)])
@pytest.mark.parametrize("dtn", ["float32", "bfloat16"])
def test_clipping_reads_the_total_on_the_device(dtn, total, max_norm):
    got, x, hp = _run(1025, dtn, dtn, total=total, max_norm=max_norm)
    coef = _ops().clip_scale_reference(torch.ones(1), torch.tensor([total], dtype=torch.float64), max_norm).item()
    if total != total:
        assert all(bool(got[k].isnan().all()) for k in (*SIDES[1:4], "param_out"))
        return
    assert coef == {0.25: 1.0, 4e4: W.coef32(torch.tensor(200.0), 1.0), float("inf"): 0.0}[total]
    _check(got, x, hp, 1, coef)


def test_sharded_optimizer_adamw_two_ranks():
    res = _gpu_launch(W.zero, 2, args=("cuda",), timeout_s=120)
    for got in res:
        for dtn, checks in got.items():
            assert checks["norm"] and checks["clips"] and checks["params"], (dtn, checks)
            assert checks["flat"] == res[0][dtn]["flat"]  # the same gathered parameters on every rank
