"""All-reduce over a block-scaled FP8 wire (``mxfp8_e4m3``).

The tensor stays f32 / bf16 / f16; what crosses the links is 32-element blocks of
``float8_e4m3fn`` with one power-of-two scale byte each, and every sum is taken in f32
(contract and error bound: docs/collectives.md "Compressed all-reduce"). For a 2-shot all-reduce
that is ``2 * 33/32 * (W-1)/W * n`` bytes per rank instead of ``8 * (W-1)/W * n`` for f32 -- 3.9x
fewer (1.94x for bf16).

No new cross-GPU protocol: three single-GPU kernels (``ops.mx_quantize`` / ``mx_reduce`` /
``mx_dequantize``) around two byte collectives the backend already has,

    quantize -> all_to_all_single -> dequantize, fold in rank order, requantize
             -> all_gather_into_tensor -> dequantize into the tensor

so the engine (IPC, copy engine, RCCL) is whatever the backend picks for a uint8 call of that
size. CPU tensors run the same sequence with the plain-PyTorch references of the three kernels.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from .. import ops

WIRES = ("mxfp8_e4m3",)
MAX_GPU_WORLD = 8  # ops.mx_reduce folds up to 8 sources (one xGMI node)

_side_streams = {}


class CompressedWork:
    """Handle of an ``async_op=True`` call: ``wait()`` orders the current stream after the result."""

    def __init__(self, event=None):
        self._event = event

    def wait(self, timeout=None) -> bool:
        if self._event is not None:
            torch.cuda.current_stream().wait_event(self._event)
        return True

    def is_completed(self) -> bool:
        return self._event is None or self._event.query()


def _op_name(op) -> str:
    """'sum' / 'avg' for the two supported ops, None otherwise."""
    for name, ref in (("sum", dist.ReduceOp.SUM), ("avg", dist.ReduceOp.AVG)):
        try:
            if op == ref:
                return name
        except Exception:  # an object ReduceOp cannot compare with
            pass
    return None


def _sequence(tensor, opn, group, world, quantize, reduce, dequantize):
    n = tensor.numel()
    wire = quantize(tensor, world)
    recv = torch.empty_like(wire)
    dist.all_to_all_single(recv, wire, group=group)  # chunk r of every rank -> rank r, in rank order
    mine = reduce(recv, world, opn)
    dist.all_gather_into_tensor(wire, mine, group=group)
    dequantize(wire, n, world)


def _run_gpu(tensor, opn, group, world):
    _sequence(tensor, opn, group, world, ops.mx_quantize, ops.mx_reduce,
              lambda w, n, W: ops.mx_dequantize(w, n, tensor.dtype, W, out=tensor))


def _run_cpu(tensor, opn, group, world):
    def store(w, n, W):
        tensor.copy_(ops.mx_dequantize_reference(w, n, tensor.dtype, W).view_as(tensor))

    _sequence(tensor, opn, group, world, ops.mx_quantize_reference, ops.mx_reduce_reference, store)


def all_reduce_compressed(tensor: torch.Tensor, op=dist.ReduceOp.SUM, group=None, wire: str = "mxfp8_e4m3",
                          async_op: bool = False):
    """In-place SUM / AVG all-reduce of ``tensor`` (float32, bfloat16 or float16) over the
    ``mxfp8_e4m3`` wire. Every rank ends with the same bits; at world 1 the tensor is left
    unchanged (not even quantized). GPU tensors run on the current stream; with ``async_op=True``
    on a side stream that first waits for the current one, and the returned handle's ``wait()``
    makes the current stream wait for it. CPU tensors run synchronously (the handle is complete)."""
    opn = _op_name(op)
    if opn is None:
        raise ValueError(f"all_reduce_compressed: only ReduceOp.SUM and ReduceOp.AVG are supported, got {op}")
    if wire not in WIRES:
        raise ValueError(f"all_reduce_compressed: unknown wire format {wire!r} (supported: {', '.join(WIRES)})")
    if tensor.dtype not in ops.MX_DTYPES:
        raise TypeError(f"all_reduce_compressed: float32, bfloat16 or float16 tensors only, got {tensor.dtype}")
    world = dist.get_world_size(group)
    if world == 1 or tensor.numel() == 0:
        return CompressedWork() if async_op else None
    if not tensor.is_cuda:
        with torch.no_grad():
            _run_cpu(tensor, opn, group, world)
        return CompressedWork() if async_op else None
    if world > MAX_GPU_WORLD:
        raise ValueError(f"all_reduce_compressed: GPU groups of up to {MAX_GPU_WORLD} ranks, got {world}")
    with torch.no_grad():
        if not async_op:
            _run_gpu(tensor, opn, group, world)
            return None
        dev = tensor.device
        side = _side_streams.get(dev)
        if side is None:
            side = _side_streams[dev] = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            _run_gpu(tensor, opn, group, world)
            event = side.record_event()
        tensor.record_stream(side)
        return CompressedWork(event)
