"""Gradient clipping on the GPU (docs/collectives.md "Gradient clipping"): ops.sumsq and ops.clip_scale against f64
references, and ShardedOptimizer(max_grad_norm=...) with ranks sharing GPU 0.

sumsq bound: every term passes at most L = ops.SUMSQ_CHAIN f32 roundings and all terms are non-negative, the f64
stages add less than 2^-40, so |got - ref| <= (L + 1) 2^-24 ref. The sizes are a partial vector, the tile's edges,
several tiles per workgroup and more partials than stage-2 lanes."""
import functools

import pytest
import torch

from tests import _workers_clip as W
from tests.test_backend_gpu import _gpu_launch

pytestmark = pytest.mark.gpu


def _ops():
    from pytorch_distributed_collective_communication_amd import ops

    return ops


T, L = 8192, 38
NUMELS = (1, 31, T - 1, T, T + 1, 3 * T + 5, 257 * T + 1)
DEV = torch.device("cuda", 0)
GUARD = 64


@functools.lru_cache(maxsize=None)
def _data(n, dtn):
    x = W.clip_data(n, n, W.DTYPES[dtn])
    return x, float(x.double().square().sum())


def _bits(t):
    return int(t.view(torch.int64).item())


def _view(x, off):
    """A copy of `x` on the GPU, `off` elements past a 16-byte aligned address, between GUARD elements of -7.5."""
    arena = torch.full((x.numel() + 2 * GUARD + off,), -7.5, dtype=x.dtype, device=DEV)
    v = arena[GUARD + off:GUARD + off + x.numel()]
    v.copy_(x)
    assert (v.data_ptr() % 16 != 0) == bool(off)
    return arena, v


def _intact(arena, v, off):
    a = arena.cpu()
    return bool((a[:GUARD + off] == -7.5).all() and (a[GUARD + off + v.numel():] == -7.5).all())


def test_constants_of_the_extension():
    ops = _ops()
    assert (ops._C().SUMSQ_TILE, ops._C().SUMSQ_CHAIN) == (ops.SUMSQ_TILE, ops.SUMSQ_CHAIN) == (T, L)


@pytest.mark.parametrize("n", NUMELS)
@pytest.mark.parametrize("dtn", list(W.DTYPES))
def test_sumsq(dtn, n):
    ops = _ops()
    x, ref = _data(n, dtn)
    g = x.to(DEV)
    got = ops.sumsq([g])
    assert got.dtype == torch.float64 and got.shape == (1,) and got.device == g.device
    assert abs(got.item() - ref) <= (L + 1) * W.U * ref, (got.item(), ref)
    assert _bits(ops.sumsq([g], max_blocks=1)) == _bits(got)  # any grid
    assert _bits(ops.sumsq([_view(x, 1)[1]])) == _bits(got)   # the element path
    assert torch.equal(g.cpu(), x)


def test_sumsq_of_a_mixed_list_and_non_finite_values():
    ops = _ops()
    parts = [_data(3 * T + 5, "float32"), _data(T + 1, "bfloat16"), _data(31, "float16")]
    xs = [parts[0][0].to(DEV), torch.empty(0, dtype=torch.bfloat16, device=DEV), parts[1][0].to(DEV), parts[2][0].to(DEV)]
    ref = sum(r for _, r in parts)
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    assert ops.sumsq(xs, out) is out and abs(out.item() - ref) <= (L + 1) * W.U * ref
    assert _bits(ops.sumsq(xs, max_blocks=1)) == _bits(out)
    assert ops.sumsq([xs[1]]).item() == 0.0
    for bad, check in ((float("inf"), torch.isinf), (float("nan"), torch.isnan)):
        x = xs[0].clone()
        x[T] = bad
        assert bool(check(ops.sumsq([xs[2], x])).all())


CASES = [("float32", "float32", False), ("float32", "float32", True)] + \
    [(s, o, inplace) for s in ("bfloat16", "float16") for o, inplace in (("float32", False), (s, False), (s, True))]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("sdn,odn,inplace", CASES)
def test_clip_scale(sdn, odn, inplace, off):
    ops = _ops()
    total = lambda v: torch.tensor([v], dtype=torch.float64, device=DEV)  # noqa: E731
    for n in (1, 31, 1025):
        x = _data(n, sdn)[0]

        def run(tot, max_norm):
            sa, sv = _view(x, off)
            oa, ov = (sa, sv) if inplace else _view(torch.zeros(n, dtype=W.DTYPES[odn]), off)
            assert ops.clip_scale(sv, tot, max_norm, out=ov) is ov
            assert _intact(oa, ov, off) and _intact(sa, sv, off) and (inplace or torch.equal(sv.cpu(), x))
            return ov.cpu()

        assert torch.equal(run(total(1.0), 10.0), x.to(W.DTYPES[odn]))  # coef == 1: the plain cast
        got = run(total(4e4), 1.0)
        assert W.scaled_ok(got, x.double() * W.coef_ref(200.0, 1.0)), (sdn, odn, n)
        assert bool(run(total(float("nan")), 1.0).isnan().all())


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_optimizer_clips_by_global_norm(world):
    res = _gpu_launch(W.zero, world, args=("cuda",), timeout_s=120)
    for got in res:
        assert len(got) == 4
        for case, checks in got.items():
            bad = [k for k, v in checks.items() if k != "norm" and not v]
            assert not bad, (case, bad, checks)
            assert checks["norm"] == res[0][case]["norm"]  # the same bits on every rank
