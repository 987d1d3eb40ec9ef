"""The fused AdamW step without a GPU (docs/collectives.md "Fused AdamW step"): the plain-torch reference against the
f64 formula at the derived bound, and ShardedOptimizer(params, "adamw") on CPU tensors at world 1 against
torch.optim.AdamW in float64, checkpoints exchanged with optimizer_cls=torch.optim.AdamW in both directions."""
import pytest
import torch

from pytorch_distributed_collective_communication_amd import ops
from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _workers_adamw as W


@pytest.mark.parametrize("fn", [ops.adamw_step, ops.adamw_step_reference])
@pytest.mark.parametrize("dtn,pdn", [("float32", "float32"), ("bfloat16", "bfloat16"), ("float16", None)])
@pytest.mark.parametrize("step,wd,total", [(1, 0.1, None), (1000, 0.0, 4e4)])
def test_reference_against_f64(fn, dtn, pdn, step, wd, total):
    n, hp = 1025, {**W.HP, "weight_decay": wd}
    g = W.clip_data(n, 1, W.DTYPES[dtn])
    p, m, v = W.clip_data(n, 2, torch.float32), 0.1 * W.clip_data(n, 3, torch.float32), W.clip_data(n, 4, torch.float32).square()
    g[5:9], v[5:9] = 0, 0
    c = W.Chain(p, m, v).step(g, step, 1.0 if total is None else W.coef32(torch.tensor(200.0), 1.0), **hp)
    out = None if pdn is None else torch.zeros(n, dtype=W.DTYPES[pdn])
    fn(g, p, m, v, step=step, param_out=out, total=None if total is None else torch.tensor([total], dtype=torch.float64),
       max_norm=None if total is None else 1.0, **hp)
    assert W.within(m, c.m, c.bm) and W.within(v, c.v, c.bv) and W.within(p, c.p, c.bp)
    assert out is None or torch.equal(out, p.to(out.dtype))


def test_sharded_optimizer_adamw_and_checkpoint_interchange():
    got = launch(W.world1, 1)[0]
    assert len(got) == 4 and all(got.values()), got


def test_constructor_errors():
    got = launch(W.errors, 1)[0]
    assert len(got) == 4 and all(got.values()), got
