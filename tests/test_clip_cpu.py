"""Gradient clipping without a GPU (docs/collectives.md "Gradient clipping"): the plain-torch references and the CPU
paths of ops.sumsq / ops.clip_scale on the shapes of tests/test_clip_gpu.py, their argument checks, and
ShardedOptimizer(max_grad_norm=...) over two gloo ranks."""
import numpy as np
import pytest
import torch

from pytorch_distributed_collective_communication_amd import ops
from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _workers_clip as W

T = ops.SUMSQ_TILE
NUMELS = (1, 31, T - 1, T, T + 1, 3 * T + 5, 257 * T + 1)


@pytest.mark.parametrize("fn", [ops.sumsq, ops.sumsq_reference])
@pytest.mark.parametrize("dtn", list(W.DTYPES))
def test_sumsq(dtn, fn):
    xs = [W.clip_data(n, n, W.DTYPES[dtn]) for n in NUMELS] + [torch.empty(0, dtype=torch.float16)]
    refs = [float(np.square(x.double().numpy()).sum()) for x in xs]
    for x, ref in zip(xs, refs):
        got = fn([x])
        assert got.dtype == torch.float64 and got.shape == (1,)
        assert abs(got.item() - ref) <= 2.0 ** -40 * ref
    assert abs(fn(xs).item() - sum(refs)) <= 2.0 ** -40 * sum(refs)
    x = xs[4].clone()
    x[T] = float("inf")
    assert fn([x]).item() == float("inf")
    x[0] = float("nan")
    assert bool(fn([xs[0], x]).isnan())


@pytest.mark.parametrize("fn", [ops.clip_scale, ops.clip_scale_reference])
@pytest.mark.parametrize("sdn,odn,inplace", [("float32", "float32", False), ("float32", "float32", True)] + [
    (s, o, i) for s in ("bfloat16", "float16") for o, i in (("float32", False), (s, False), (s, True))])
def test_clip_scale(sdn, odn, inplace, fn):
    total = lambda v: torch.tensor([v], dtype=torch.float64)  # noqa: E731
    for n in (1, 31, 1025):
        x = W.clip_data(n, n, W.DTYPES[sdn])

        def run(tot, max_norm):
            src = x.clone()
            out = src if inplace else torch.zeros(n, dtype=W.DTYPES[odn])
            assert fn(src, tot, max_norm, out=out) is out and (inplace or torch.equal(src, x))
            return out

        assert torch.equal(run(total(1.0), 10.0), x.to(W.DTYPES[odn]))
        assert W.scaled_ok(run(total(4e4), 1.0), x.double() * W.coef_ref(200.0, 1.0))
        assert bool(run(total(float("nan")), 1.0).isnan().all())
        assert bool((run(total(float("inf")), 1.0) == 0).all())
    assert fn(x, total(1.0), 10.0).dtype == torch.float32


def test_argument_checks():
    x, tot = torch.ones(4), torch.ones(1, dtype=torch.float64)
    for fn in (ops.sumsq, ops.sumsq_reference):
        for bad in ([], [x.double()], [x.to(torch.int32)], [x, x.to("meta")]):
            with pytest.raises(ValueError):
                fn(bad)
    for fn in (ops.clip_scale, ops.clip_scale_reference):
        for args in ((x.double(), tot, 1.0), (x, tot.float(), 1.0), (x, torch.ones(2, dtype=torch.float64), 1.0),
                     (x, tot, 1.0, torch.ones(4, dtype=torch.bfloat16)), (x, tot, 1.0, torch.ones(5))):
            with pytest.raises(ValueError):
                fn(*args)


def test_sharded_optimizer_clips_by_global_norm():
    res = launch(W.zero, 2, args=("cpu",))
    for got in res:
        assert len(got) == 4
        for case, checks in got.items():
            bad = [k for k, v in checks.items() if k != "norm" and not v]
            assert not bad, (case, bad, checks)
            assert checks["norm"] == res[0][case]["norm"]


def test_constructor_errors():
    got = launch(W.errors, 1, args=("cpu",))[0]
    assert len(got) == 9 and all(got.values()), got
