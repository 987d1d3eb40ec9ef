"""The fused AdamW step on 8-bit state on the GPU (docs/collectives.md "8-bit AdamW state"): ops.adamw_step with
state_format="mxfp8_e4m3" against the f64 chain from the unpacked state (bounds: tests/_workers_adamw8.py), the
element path, clipping and non-finite values, and ShardedOptimizer with two ranks sharing GPU 0."""
import pytest
import torch

from tests import _workers_adamw8 as W8
from tests.test_backend_gpu import _gpu_launch
from tests.test_clip_gpu import DEV, _intact, _view

pytestmark = pytest.mark.gpu
SPAN = 4096
NUMELS = (1, 31, 32, 33, 511, 512, 513, SPAN - 1, SPAN, SPAN + 1)


def _run(x, hp, step=1, off_side=None, total=None, max_norm=None, max_blocks=0):
    """One call on guarded views of the CPU inputs `x` (`off_side`: that view starts one element past a 16-byte
    boundary), param_out of the gradient's dtype. Checks the guard bands, the untouched gradient and the round-once
    contract; returns the CPU results."""
    x = {**x, "param_out": torch.zeros_like(x["grad"])}
    off = {k: int(k == off_side) for k in x}
    views = {k: _view(t, off[k]) for k, t in x.items() if t.dtype != torch.uint8}
    state = {k: torch.full((t.numel() + 128,), 0xA5, dtype=torch.uint8, device=DEV) for k, t in x.items() if k not in views}
    t = {k: views[k][1] if k in views else state[k][64:-64].copy_(x[k]) for k in x}
    W8._ops().adamw_step(t["grad"], t["master"], t["exp_avg"], t["exp_avg_sq"], step=step, param_out=t["param_out"],
                         total=None if total is None else torch.tensor([total], dtype=torch.float64, device=DEV),
                         max_norm=max_norm, max_blocks=max_blocks, state_format=W8.FMT, **hp)
    assert all(_intact(views[k][0], t[k], off[k]) for k in views), "guard bands"
    assert all(bool((a[:64] == 0xA5).all() and (a[-64:] == 0xA5).all()) for a in state.values()), "guard bands of the state"
    got = {k: v.cpu() for k, v in t.items()}
    assert torch.equal(got["grad"].view(torch.uint8), x["grad"].view(torch.uint8))  # (the bytes: a NaN stays put)
    ok = ~got["master"].isnan()
    assert torch.equal(got["param_out"][ok], got["master"].to(x["grad"].dtype)[ok]), "param_out is the master rounded once"
    return got


@pytest.mark.parametrize("step,wd", [(1, 0.0), (1, 0.1), (1000, 0.0), (1000, 0.1)])
@pytest.mark.parametrize("dtn", list(W8.DTYPES))
@pytest.mark.parametrize("n,max_blocks", [(n, 0) for n in NUMELS] + [(2 * SPAN + 5, 1)])
def test_one_step_against_f64(n, max_blocks, dtn, step, wd):
    x, hp = W8.data(n, dtn), {**W8.HP, "weight_decay": wd}
    got = _run(x, hp, step, max_blocks=max_blocks)
    W8.check_step(got, x, hp, step)
    W8.check_exact(got, n)


@pytest.mark.parametrize("side", ["grad", "master", "param_out"])
@pytest.mark.parametrize("dtn", list(W8.DTYPES))
def test_element_path_gives_the_same_bytes(dtn, side):
    x = W8.data(1025, dtn)
    base, got = _run(x, W8.HP), _run(x, W8.HP, off_side=side)
    assert all(torch.equal(got[k], base[k]) for k in base)


@pytest.mark.parametrize("total", [0.25, 4e4, float("inf"), float("nan")])
@pytest.mark.parametrize("dtn", ["float32", "bfloat16"])
def test_clipping_reads_the_total_on_the_device(dtn, total):
    x = W8.data(1025, dtn)
    got = _run(x, W8.HP, total=total, max_norm=1.0)
    if total != total:
        assert bool(got["master"].isnan().all())
        return
    coef = {0.25: 1.0, 4e4: W8.coef32(torch.tensor(200.0), 1.0), float("inf"): 0.0}[total]
    W8.check_step(got, x, W8.HP, 1, coef)


def test_a_nan_gradient_takes_its_block_one_step_later():
    n, at = 1025, 100
    x = {k: v.clone() for k, v in W8.data(n, "float32").items()}
    x["grad"][at] = float("nan")
    cb, block = W8._ops().mx_chunk_blocks(n, 1), torch.arange(n) // 32 == at // 32
    one = _run(x, W8.HP)
    assert all(one[k][32 * cb + at // 32] == 255 for k in ("exp_avg", "exp_avg_sq"))
    assert torch.equal(one["master"].isnan(), torch.arange(n) == at)
    W8.check_step(one, x, W8.HP, 1, keep=~block)
    x2 = {**one, "grad": W8.data(n, "float32")["grad"]}
    del x2["param_out"]
    two = _run(x2, W8.HP, step=2)
    assert torch.equal(two["master"].isnan(), block)
    W8.check_step(two, x2, W8.HP, 2, keep=~block)


def test_sharded_optimizer_two_ranks():
    res = _gpu_launch(W8.zero, 2, args=("cuda",), timeout_s=120)
    for got in res:
        for dtn, checks in got.items():
            assert len(checks) == 4 and all(checks.values()), (dtn, checks)
            assert checks["flat"] == res[0][dtn]["flat"]  # the same gathered parameters on every rank
