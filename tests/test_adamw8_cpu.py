"""The 8-bit AdamW state without a GPU (docs/collectives.md "8-bit AdamW state"): the plain-torch reference of
ops.adamw_step(state_format=...) against the f64 chain, pack / unpack, and ShardedOptimizer at world 1."""
import pytest
import torch

from pytorch_distributed_collective_communication_amd import ops
from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _workers_adamw8 as W8

NUMELS = (1, 31, 32, 33, 511, 512, 513, 4095, 4096, 4097, 2 * 4096 + 5)


@pytest.mark.parametrize("fn", [ops.adamw_step, ops.adamw_step_reference])
@pytest.mark.parametrize("step,wd", [(1, 0.0), (1000, 0.1)])
@pytest.mark.parametrize("dtn", list(W8.DTYPES))
@pytest.mark.parametrize("n", NUMELS)
def test_reference_step_against_f64(n, dtn, step, wd, fn):
    x, hp = W8.data(n, dtn), {**W8.HP, "weight_decay": wd}
    got = {k: v.clone() for k, v in x.items()}
    out = torch.zeros(n, dtype=W8.DTYPES[dtn])
    fn(got["grad"], got["master"], got["exp_avg"], got["exp_avg_sq"], step=step, param_out=out, state_format=W8.FMT, **hp)
    W8.check_step(got, x, hp, step)
    W8.check_exact(got, n)
    assert torch.equal(out, got["master"].to(out.dtype)) and torch.equal(got["grad"], x["grad"])


@pytest.mark.parametrize("n", [33, 1025])
def test_pack_and_unpack(n):
    m, v = 0.1 * W8.clip_data(n, 1, torch.float32), 0.01 * W8.clip_data(n, 2, torch.float32).square()
    b = ops.adamw_state_pack(m, v)
    assert torch.equal(b[0], ops.mx_quantize_reference(m, 1)) and b[1].numel() == ops.mx_wire_bytes(n, 1)
    m1, v1 = ops.adamw_state_unpack(*b, n)
    assert W8.within(m1, m.double(), W8.stored_tol(m.double()))
    assert W8.within(v1.sqrt(), v.double().sqrt(), W8.stored_tol(v.double().sqrt()) + 2 * W8.U * v.double().sqrt())
    m2, v2 = ops.adamw_state_unpack(*ops.adamw_state_pack(m1, v1), n)
    assert torch.equal(m2, m1) and torch.equal(v2, v1)
    z = ops.adamw_state_pack(torch.zeros(n), torch.zeros(n))
    cb = ops.mx_chunk_blocks(n, 1)
    assert all(not t[:32 * cb].any() and bool((t[32 * cb:] == 127).all()) for t in z)


def test_sharded_optimizer_world1_checkpoints_and_errors():
    got = launch(W8.world1, 1)[0]
    assert len(got) == 10 and all(got.values()), got


def test_unknown_state_format_and_misaligned_state():
    x = {k: v.clone() for k, v in W8.data(33, "float32").items()}
    off = torch.zeros(x["exp_avg"].numel() + 1, dtype=torch.uint8)[1:]
    for m, fmt in ((x["exp_avg"], "mxfp4_e2m1"), (off, W8.FMT)):
        with pytest.raises(ValueError):
            ops.adamw_step(x["grad"], x["master"], m, x["exp_avg_sq"], step=1, state_format=fmt, **W8.HP)
