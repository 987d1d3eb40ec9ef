"""The fused AdamW step that emits the parameter wire, without a GPU (docs/collectives.md "Parameter wire from the
step"): CPU tensors go through the plain-torch reference; the keyword validation; all_gather_compressed(input_wire=)
over the host transport."""
import pytest
import torch

from pytorch_distributed_collective_communication_amd import ops
from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _workers_adamw_wire as WW
from tests._workers_adamw import HP


@pytest.mark.parametrize("n", WW.NUMELS[:3])
@pytest.mark.parametrize("state", [None, WW.FMT])
@pytest.mark.parametrize("dtn", ["float32", "bfloat16"])
@pytest.mark.parametrize("wire", ops.MX_WIRES)
def test_cpu_tensors_take_the_reference(wire, dtn, state, n):
    got = WW.ran(n, dtn, state, wire, "cpu")
    WW.check_wire(got, n, wire)
    WW.check_reference(got, WW.expected(n, dtn, state, wire))
    alone = WW.step(WW.data(n, dtn, state), wire, state, "cpu", param_out=False, fn=ops.adamw_step_reference)
    assert WW.same_bytes(alone["wire"], got["wire"])


def test_spans_of_a_packed_state():
    WW.check_spans("cpu")


@pytest.mark.parametrize("fn", [ops.adamw_step, ops.adamw_step_reference])
def test_keyword_validation(fn):
    x = {k: v.clone() for k, v in WW.data(40, "bfloat16", None).items()}
    nb = ops.mx_wire_bytes(40, 1)
    call = lambda **kw: fn(x["grad"], x["master"], x["exp_avg"], x["exp_avg_sq"], step=1, **kw, **HP)  # noqa: E731
    w, bf = torch.zeros(nb, dtype=torch.uint8), torch.bfloat16
    for kw in (dict(wire_out=w),                                                # no param_out, no wire_dtype
               dict(wire_out=w, wire_dtype=torch.float16),                      # neither f32 nor the gradient's dtype
               dict(wire_out=w, wire_dtype=torch.float32, param_out=torch.zeros(40, dtype=bf)),  # they disagree
               dict(wire_out=w, wire_dtype=bf, wire="mxfp8"),                   # unknown wire
               dict(wire_out=w[:-1], wire_dtype=bf),                            # wrong size
               dict(wire_out=w, wire_dtype=bf, wire="mxfp4_e2m1"),              # ... for this wire
               dict(wire_out=torch.zeros(nb + 1, dtype=torch.uint8)[1:], wire_dtype=bf),  # misaligned
               dict(state_offset=0)):                                           # without state_format
        with pytest.raises(ValueError):
            call(**kw)
    call(wire="mxfp8", wire_dtype=torch.float16)  # without wire_out both are ignored
    call(wire_out=w, param_out=torch.zeros(40, dtype=bf))  # wire_dtype defaults to param_out's
    assert bool(w.any())


def test_all_gather_takes_a_ready_wire():
    for got in launch(WW.gather_input_wire, 2):
        assert len(got) == 5 and all(got.values()), got
