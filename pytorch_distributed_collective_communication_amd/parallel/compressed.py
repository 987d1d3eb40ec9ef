"""All-reduce, reduce-scatter and all-gather over a block-scaled wire: ``mxfp8_e4m3``, ``mxfp4_e2m1`` or ``mxfp6_e2m3``.

The tensor stays f32 / bf16 / f16; what crosses the links is 32-element blocks of
``float8_e4m3fn`` with one power-of-two scale byte each, and every sum is taken in f32
(contract and error bound: docs/collectives.md "Compressed all-reduce"). For a 2-shot all-reduce
that is ``2 * 33/32 * (W-1)/W * n`` bytes per rank instead of ``8 * (W-1)/W * n`` for f32 -- 3.9x
fewer (1.94x for bf16).

``wire="mxfp4_e2m1"`` (docs/collectives.md "The ``mxfp4_e2m1`` wire format") sends two e2m1 nibbles
per byte: a block is 17 bytes instead of 33, 7.5x fewer than f32, 3.76x fewer than bf16 and 1.94x
fewer than ``mxfp8_e4m3`` -- arithmetic on the layouts, not a measurement -- at an error bound five
times coarser (``amax / 3`` per quantization). The sequences, the fold order and every rule below are
the same for both formats; the single-quantization reduce-scatter is the intended use for gradients.

No new cross-GPU protocol: three single-GPU kernels (``ops.mx_quantize`` / ``mx_reduce`` /
``mx_dequantize``) around two byte collectives the backend already has,

    quantize -> all_to_all_single -> dequantize, fold in rank order, requantize
             -> all_gather_into_tensor -> dequantize into the tensor

so the engine (IPC, copy engine, RCCL) is whatever the backend picks for a uint8 call of that
size. CPU tensors run the same sequence with the plain-PyTorch references of the three kernels.

The two halves on their own (ZeRO's collectives; docs/collectives.md "Compressed reduce-scatter and
all-gather") use the shard layout -- one chunk per shard, blocks counted from the shard's start:

    reduce_scatter_compressed:  quantize_shards -> all_to_all_single -> fold into the output
    all_gather_compressed:      quantize -> all_gather_into_tensor -> dequantize_shards into the output

The fold's result stays on its owner, so it is not quantized again: one quantization per
contribution. A reduce-scatter moves ``33/32 * (W-1) * m`` bytes per rank instead of ``4 * (W-1) * m``
for f32 (3.9x fewer, 1.94x for bf16), a gather of bf16 shards 1.94x fewer.

Every quantizer rounds to nearest unless told otherwise, which biases an element that rounds the same
way at every step. The two remedies are alternatives (docs/collectives.md "Error feedback", "Stochastic
rounding"): ``residual=`` carries what was dropped to the next call, at 4 bytes of state per element;
``rounding="stochastic"`` with a ``seed=`` rounds up or down with the probability of the distance, so the
expected value of what is sent is the input, with no state and the bytes of the plain kernels, at
twice the worst-case error of one call. Rank ``r`` draws its words from stream ``2 r`` (its contribution)
and ``2 r + 1`` (the chunk it requantizes), so ranks are independent even with one seed; varying the seed
from call to call is the caller's job (``GradBucketer`` and ``ShardedOptimizer`` do it). Gradients are the
intended use. Both are properties of the local kernels: the wire and the protocol do not change.

``rotation="hadamard"`` with a ``rotation_seed=`` (docs/collectives.md "Hadamard rotation") composes with
either: every 32-element block is rotated by a randomized Hadamard matrix before it is quantized and back
after it is dequantized, inside the same kernels. A block's scale comes from its largest element, so one
outlier pushes the rest of its block below the grid of the narrow formats; the rotation spreads it over
the block. The fold is linear, so the owner's ``mx_reduce`` works on rotated chunks unchanged. Every rank
must pass the same rotation and seed, and a carried residual belongs to one seed.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from .. import ops

WIRES = ("mxfp8_e4m3", "mxfp4_e2m1", "mxfp6_e2m3")
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


def _run_gpu(tensor, opn, group, world, wire, residual=None, owner_residual=None, sr=({}, {}), rot={}):
    _sequence(tensor, opn, group, world,
              lambda x, W: ops.mx_quantize(x, W, wire=wire, residual=residual, **sr[0], **rot),
              lambda w, W, o: ops.mx_reduce(w, W, o, wire=wire, residual=owner_residual, **sr[1]),
              lambda w, n, W: ops.mx_dequantize(w, n, tensor.dtype, W, out=tensor, wire=wire, **rot))


def _run_cpu(tensor, opn, group, world, wire, residual=None, owner_residual=None, sr=({}, {}), rot={}):
    def store(w, n, W):
        tensor.copy_(ops.mx_dequantize_reference(w, n, tensor.dtype, W, wire=wire, **rot).view_as(tensor))

    _sequence(tensor, opn, group, world,
              lambda x, W: ops.mx_quantize_reference(x, W, wire=wire, residual=residual, **sr[0], **rot),
              lambda w, W, o: ops.mx_reduce_reference(w, W, o, wire=wire, residual=owner_residual, **sr[1]), store)


ROUNDINGS = ("nearest", "stochastic")


def _rounding_args(who, rounding, seed, group, residuals=()):
    """The rounding arguments of a collective, checked before any communication. Returns the keywords of this
    rank's quantization and of its requantization: none for ``"nearest"`` (the plain calls), else the seed
    with the streams ``2 rank`` and ``2 rank + 1``."""
    if not isinstance(rounding, str) or rounding not in ROUNDINGS:
        raise ValueError(f"{who}: unknown rounding {rounding!r} (supported: {', '.join(ROUNDINGS)})")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError(f"{who}: seed must be an int, got {type(seed).__name__}")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"{who}: seed must be in [0, 2^64), got {seed}")
    if rounding == "nearest":
        return {}, {}
    if any(r is not None for r in residuals):
        raise ValueError(f"{who}: rounding='stochastic' and a residual are alternatives, not both")
    rank = dist.get_rank(group)
    return (dict(rounding=rounding, seed=seed, stream=2 * rank),
            dict(rounding=rounding, seed=seed, stream=2 * rank + 1))


ROTATIONS = ("hadamard",)


def _rotation_args(who, rotation, rotation_seed):
    """The rotation arguments of a collective, checked before any communication. Returns the keywords of the
    kernels that touch the tensor: none for ``None`` (the plain calls)."""
    if rotation is not None and (not isinstance(rotation, str) or rotation not in ROTATIONS):
        raise ValueError(f"{who}: unknown rotation {rotation!r} (supported: None, {', '.join(ROTATIONS)})")
    if isinstance(rotation_seed, bool) or not isinstance(rotation_seed, int):
        raise TypeError(f"{who}: rotation_seed must be an int, got {type(rotation_seed).__name__}")
    if not 0 <= rotation_seed < 1 << 64:
        raise ValueError(f"{who}: rotation_seed must be in [0, 2^64), got {rotation_seed}")
    return {} if rotation is None else dict(rotation=rotation, rotation_seed=rotation_seed)


def _check_residual(who, name, res, numel, device):
    """An error-feedback residual, checked before any communication: float32, ``numel`` elements, on the
    tensor's device, contiguous and 16-byte aligned (it is updated in place, so it cannot be copied)."""
    if res is None:
        return
    if not isinstance(res, torch.Tensor) or res.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be a float32 tensor, got "
                        f"{res.dtype if isinstance(res, torch.Tensor) else type(res).__name__}")
    if res.numel() != numel:
        raise ValueError(f"{who}: {name} has {res.numel()} elements, {numel} expected")
    if res.device != device:
        raise ValueError(f"{who}: {name} is on {res.device}, the tensor on {device}")
    if not res.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")
    if res.data_ptr() % 16:
        raise ValueError(f"{who}: {name} must be 16-byte aligned")


def all_reduce_compressed(tensor: torch.Tensor, op=dist.ReduceOp.SUM, group=None, wire: str = "mxfp8_e4m3",
                          async_op: bool = False, *, residual: torch.Tensor | None = None,
                          owner_residual: torch.Tensor | None = None, rounding: str = "nearest", seed: int = 0,
                          rotation: str | None = None, rotation_seed: int = 0):
    """In-place SUM / AVG all-reduce of ``tensor`` (float32, bfloat16 or float16) over the wire
    format ``wire`` (``mxfp8_e4m3``, ``mxfp4_e2m1`` or ``mxfp6_e2m3``). Every rank ends with the same bits; at world 1 the tensor is left
    unchanged (not even quantized). GPU tensors run on the current stream; with ``async_op=True``
    on a side stream that first waits for the current one, and the returned handle's ``wait()``
    makes the current stream wait for it. CPU tensors run synchronously (the handle is complete).
    Until ``wait()``, issue no other collective of the group from another stream (two collectives
    of one group must not overlap on the device; :func:`order_after_compressed` is the fence).

    Error feedback (docs/collectives.md "Error feedback"): ``residual`` (float32, ``tensor.numel()``
    elements) is added to this rank's contribution before it is quantized and is left holding what the
    quantization dropped; ``owner_residual`` (float32, ``ops.mx_owner_residual_numel(numel, W, wire=wire)``
    elements) does the same for the requantization of the chunk this rank owns. Both are updated in place,
    by the kernel that quantizes; either may be given alone, and every rank must make the same choice. Carry
    them from call to call: the sum of what is sent then tracks the sum of the inputs to within one
    bounded residual. At world 1 they are left untouched, like the tensor.

    Stochastic rounding (docs/collectives.md "Stochastic rounding"): ``rounding="stochastic"`` rounds this
    rank's contribution by the words of ``(seed, 2 rank)`` and the chunk it owns by those of ``(seed,
    2 rank + 1)``; the expected value of either quantization is its input. Ranks may use any seeds (their
    errors are independent either way) and still end with the same bits; the same seeds give the same
    bits again, so pass a new seed with every call. Not together with a residual (``ValueError``).

    Hadamard rotation (docs/collectives.md "Hadamard rotation"): ``rotation="hadamard"`` rotates every block
    of this rank's contribution with the sign word of ``rotation_seed`` before it is quantized and rotates
    the gathered result back; the owner stage folds and requantizes rotated chunks as they are. Every rank
    must pass the same rotation and seed. Composes with the residuals (which then live in the rotated
    domain: keep the seed for as long as they are carried) and with stochastic rounding."""
    opn = _op_name(op)
    if opn is None:
        raise ValueError(f"all_reduce_compressed: only ReduceOp.SUM and ReduceOp.AVG are supported, got {op}")
    if wire not in WIRES:
        raise ValueError(f"all_reduce_compressed: unknown wire format {wire!r} (supported: {', '.join(WIRES)})")
    if tensor.dtype not in ops.MX_DTYPES:
        raise TypeError(f"all_reduce_compressed: float32, bfloat16 or float16 tensors only, got {tensor.dtype}")
    world = dist.get_world_size(group)
    _check_residual("all_reduce_compressed", "residual", residual, tensor.numel(), tensor.device)
    _check_residual("all_reduce_compressed", "owner_residual", owner_residual,
                    ops.mx_owner_residual_numel(tensor.numel(), world, wire=wire), tensor.device)
    sr = _rounding_args("all_reduce_compressed", rounding, seed, group, (residual, owner_residual))
    rot = _rotation_args("all_reduce_compressed", rotation, rotation_seed)
    if world == 1 or tensor.numel() == 0:
        return CompressedWork() if async_op else None
    if not tensor.is_cuda:
        with torch.no_grad():
            _run_cpu(tensor, opn, group, world, wire, residual, owner_residual, sr, rot)
        return CompressedWork() if async_op else None
    if world > MAX_GPU_WORLD:
        raise ValueError(f"all_reduce_compressed: GPU groups of up to {MAX_GPU_WORLD} ranks, got {world}")
    held = tuple(t for t in (tensor, residual, owner_residual) if t is not None)
    return _issue_gpu(lambda: _run_gpu(tensor, opn, group, world, wire, residual, owner_residual, sr, rot), held,
                      async_op)


def _issue_gpu(run, tensors, async_op):
    """``run()`` on the current stream, or (``async_op``) on the device's side stream after it."""
    with torch.no_grad():
        if not async_op:
            run()
            return None
        dev = tensors[0].device
        side = _side_streams.get(dev)
        if side is None:
            side = _side_streams[dev] = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            run()
            event = side.record_event()
        for t in tensors:
            t.record_stream(side)
        return CompressedWork(event)


def order_after_compressed(device=None) -> None:
    """Make the current stream wait for every ``async_op=True`` compressed call issued so far on
    ``device``. The backend keeps the collectives of one group from overlapping on its own streams,
    but the side stream of the compressed calls is not one of them: before ``wait()`` on their
    handles, another collective of the same group goes behind this fence (or behind the waits)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    side = _side_streams.get(dev)
    if side is not None:
        torch.cuda.current_stream(dev).wait_stream(side)


def _check_pair(who, output, input, wire, group, big, small):
    """The checks the two shard collectives share; returns the world size. ``big`` holds ``world`` times
    the elements of ``small``."""
    if wire not in WIRES:
        raise ValueError(f"{who}: unknown wire format {wire!r} (supported: {', '.join(WIRES)})")
    for t in (input, output):
        if t.dtype not in ops.MX_DTYPES:
            raise TypeError(f"{who}: float32, bfloat16 or float16 tensors only, got {t.dtype}")
    if input.dtype != output.dtype:
        raise TypeError(f"{who}: input is {input.dtype}, output is {output.dtype}")
    world = dist.get_world_size(group)
    if big.numel() != world * small.numel():
        raise ValueError(f"{who}: {'input' if big is input else 'output'} has {big.numel()} elements, "
                         f"{world} x {small.numel()} = {world * small.numel()} expected")
    if not output.is_contiguous():
        raise ValueError(f"{who}: output must be contiguous")
    if input.device != output.device:
        raise ValueError(f"{who}: input is on {input.device}, output on {output.device}")
    if input.is_cuda and world > MAX_GPU_WORLD:
        raise ValueError(f"{who}: GPU groups of up to {MAX_GPU_WORLD} ranks, got {world}")
    return world


def _done(async_op):
    return CompressedWork() if async_op else None


def reduce_scatter_compressed(output: torch.Tensor, input: torch.Tensor, op=dist.ReduceOp.SUM, group=None,
                              wire: str = "mxfp8_e4m3", async_op: bool = False, *,
                              residual: torch.Tensor | None = None, rounding: str = "nearest", seed: int = 0,
                              rotation: str | None = None, rotation_seed: int = 0):
    """SUM / AVG reduce-scatter of ``input`` (``W * m`` elements; f32, bf16 or f16) into ``output`` (``m``
    elements) over the wire format ``wire``: rank ``k`` ends with the f32 fold, in rank order, of every
    rank's quantized shard ``k`` (its own included), rounded once to the dtype. The fold is not
    quantized again. At world 1 ``input`` is copied bit for bit. Streams and ``async_op`` as in
    :func:`all_reduce_compressed`.

    ``residual`` (float32, ``input.numel()`` elements; error feedback as in :func:`all_reduce_compressed`) is
    added to ``input`` before it is quantized and left holding what the quantization dropped; ``input`` itself is
    not modified. The fold is not quantized, so there is no owner residual. Untouched at world 1.

    ``rounding="stochastic"`` with ``seed`` (as in :func:`all_reduce_compressed`): this rank's shards are
    rounded by the words of ``(seed, 2 rank)``, an element by its index in ``input``; the one quantization
    of each contribution is then unbiased and the W errors of a sum are independent. Not with ``residual``.

    ``rotation="hadamard"`` with ``rotation_seed`` (as in :func:`all_reduce_compressed`, the same on every
    rank): the blocks of every shard are rotated before they are quantized, and the fold is rotated back once
    before it is rounded."""
    who = "reduce_scatter_compressed"
    opn = _op_name(op)
    if opn is None:
        raise ValueError(f"{who}: only ReduceOp.SUM and ReduceOp.AVG are supported, got {op}")
    world = _check_pair(who, output, input, wire, group, input, output)
    _check_residual(who, "residual", residual, input.numel(), input.device)
    sr, _ = _rounding_args(who, rounding, seed, group, (residual,))
    rot = _rotation_args(who, rotation, rotation_seed)
    m = output.numel()
    if m == 0:
        return _done(async_op)
    if world == 1:
        with torch.no_grad():
            output.copy_(input.reshape(output.shape))
        return _done(async_op)
    if not input.is_cuda:
        with torch.no_grad():
            w = ops.mx_quantize_shards_reference(input, world, wire=wire, residual=residual, **sr, **rot)
            recv = torch.empty_like(w)
            dist.all_to_all_single(recv, w, group=group)
            output.copy_(ops.mx_fold_reference(recv, world, m, output.dtype, opn, wire=wire, **rot).view_as(output))
        return _done(async_op)

    def run():
        w = ops.mx_quantize_shards(input, world, wire=wire, residual=residual, **sr, **rot)
        recv = torch.empty_like(w)
        dist.all_to_all_single(recv, w, group=group)  # chunk r of every rank -> rank r, in rank order
        ops.mx_fold(recv, world, m, output.dtype, opn, out=output, wire=wire, **rot)

    return _issue_gpu(run, (output, input) if residual is None else (output, input, residual), async_op)


def all_gather_compressed(output: torch.Tensor, input: torch.Tensor, group=None, wire: str = "mxfp8_e4m3",
                          async_op: bool = False, *, rounding: str = "nearest", seed: int = 0,
                          rotation: str | None = None, rotation_seed: int = 0):
    """All-gather of ``input`` (``m`` elements; f32, bf16 or f16) into ``output`` (``W * m`` elements)
    over the wire format ``wire``: every rank ends with the same bits, the dequantized wire of every
    rank's shard -- its own slot included. At world 1 ``input`` is copied bit for bit. Streams and
    ``async_op`` as in :func:`all_reduce_compressed`.

    ``rounding="stochastic"`` with ``seed``: accepted because the gather shares the quantizer -- this rank's
    shard is rounded by the words of ``(seed, 2 rank)``, and every rank still ends with the same bits. It is
    meant for gradients; values that are not summed or averaged afterwards (parameters) gain nothing
    from it and pay twice the worst-case error.

    ``rotation="hadamard"`` with ``rotation_seed`` (the same on every rank): this rank's blocks are rotated
    before they are quantized and every gathered shard is rotated back."""
    who = "all_gather_compressed"
    world = _check_pair(who, output, input, wire, group, output, input)
    sr, _ = _rounding_args(who, rounding, seed, group)
    rot = _rotation_args(who, rotation, rotation_seed)
    m = input.numel()
    if m == 0:
        return _done(async_op)
    if world == 1:
        with torch.no_grad():
            output.copy_(input.reshape(output.shape))
        return _done(async_op)
    if not input.is_cuda:
        with torch.no_grad():
            mine = ops.mx_quantize_reference(input, 1, wire=wire, **sr, **rot)
            every = torch.empty(mine.numel() * world, dtype=torch.uint8)
            dist.all_gather_into_tensor(every, mine, group=group)
            output.copy_(ops.mx_dequantize_shards_reference(every, m, output.dtype, world, wire=wire, **rot).view_as(output))
        return _done(async_op)

    def run():
        mine = ops.mx_quantize(input, 1, wire=wire, **sr, **rot)
        every = torch.empty(mine.numel() * world, dtype=torch.uint8, device=mine.device)
        dist.all_gather_into_tensor(every, mine, group=group)
        ops.mx_dequantize_shards(every, m, output.dtype, world, out=output, wire=wire, **rot)

    return _issue_gpu(run, (output, input), async_op)
