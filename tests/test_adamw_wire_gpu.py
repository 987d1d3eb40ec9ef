"""The fused AdamW step that emits the parameter wire, on the GPU (docs/collectives.md "Parameter wire from the step"):
ops.adamw_step(wire_out=...) byte for byte against the plain-torch references, the dequantized wire against an f64
step, spans of a packed state, and ShardedOptimizer with two ranks sharing GPU 0."""
import pytest
import torch

from tests import _workers_adamw_wire as WW
from tests._workers_adamw import HP, Chain, coef32
from tests.test_backend_gpu import _gpu_launch

pytestmark = pytest.mark.gpu
WIRES = ("mxfp8_e4m3", "mxfp4_e2m1", "mxfp6_e2m3")


CASES = [pytest.mark.parametrize("n", WW.NUMELS), pytest.mark.parametrize("state", [None, WW.FMT]),
         pytest.mark.parametrize("dtn", ["float32", "bfloat16"]), pytest.mark.parametrize("wire", WIRES)]


def _cases(f):
    for mark in CASES:
        f = mark(f)
    return f


def _ran(wire, dtn, state, n):
    return WW.ran(n, dtn, state, wire, "cuda", 2 if n == WW.NUMELS[2] else 0)  # (max_blocks=2: the grid strides)


@_cases
def test_wire_is_the_quantized_param_out_byte_for_byte(wire, dtn, state, n):
    got = _ran(wire, dtn, state, n)
    WW.check_wire(got, n, wire)
    if n == WW.NUMELS[1]:  # without param_out: the same master, state and wire
        alone = WW.step(WW.data(n, dtn, state), wire, state, "cuda", param_out=False)
        assert alone["param_out"] is None and all(WW.same_bytes(alone[k], got[k]) for k in WW.KEYS if k != "param_out")


@_cases
def test_master_state_param_out_and_wire_equal_the_reference_bit_for_bit(wire, dtn, state, n):
    """adamw_step_reference runs on the same inputs where the kernel reads them, on the GPU: one plain torch operation
    per rounding. (Run on CPU copies of the inputs, the same reference differs from both by an ulp or two of the master
    in about 1 % of the elements, with identical moments; the kernel's division and square root are the correctly
    rounded expansions and nothing in it is contracted.)"""
    WW.check_reference(_ran(wire, dtn, state, n), WW.expected(n, dtn, state, wire, "cuda"))


@pytest.mark.parametrize("wire,div", [("mxfp8_e4m3", 16), ("mxfp4_e2m1", 3), ("mxfp6_e2m3", 16)])
def test_dequantized_wire_against_f64(wire, div):
    """Tolerance: the step's bound (docs "The bound") + half a bf16 ulp + the wire's amax_block / div, the block amax
    taken from the f64 step's values raised by the first two."""
    n, ops = 4096 + 36, WW._ops()
    x = {k: v.clone() for k, v in WW.data(n, "bfloat16", None).items()}
    x["master"][3] = 1.0  # (finite throughout: the bound speaks of numbers)
    got = WW.step(x, wire, None, "cuda")
    c = Chain(x["master"], x["exp_avg"], x["exp_avg_sq"]).step(x["grad"], 3, coef32(torch.tensor(200.0), WW.MAX_NORM), **HP)
    pre = c.bp + 2.0 ** -8 * (c.p.abs() + c.bp)
    amax = torch.nn.functional.pad(c.p.abs() + pre, (0, -n % 32)).view(-1, 32).amax(1).repeat_interleave(32)[:n]
    err = (ops.mx_dequantize_reference(got["wire"], n, wire=wire).double() - c.p).abs()
    print(wire, float((err / (pre + amax / div)).max()))
    assert bool((err <= pre + amax / div).all())


def test_spans_of_a_packed_state():
    WW.check_spans("cuda")


def test_misaligned_sides_raise():
    x = WW.data(40, "bfloat16", None)
    t = {k: torch.zeros(v.numel() + 1, dtype=v.dtype, device="cuda")[1:].copy_(v) for k, v in x.items()}
    w = torch.empty(WW._ops().mx_wire_bytes(40, 1), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        WW._ops().adamw_step(t["grad"], t["master"], t["exp_avg"], t["exp_avg_sq"], step=1, wire_out=w,
                             wire_dtype=torch.bfloat16, **HP)


def test_sharded_optimizer_two_ranks():
    res = _gpu_launch(WW.zero, 2, args=("cuda",), timeout_s=120)
    for got in res:
        assert len(got) == 9 and got.pop("rotation") == [False, True]
        assert all(v == [True, True] for v in got.values()), got
