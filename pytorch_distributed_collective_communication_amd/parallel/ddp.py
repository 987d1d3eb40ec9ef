"""Data-parallel gradient synchronisation on the mi355x backend.

The reference motivates collectives with data parallelism: every worker
computes gradients on its batch shard and they are all-reduced and averaged
before the optimizer step (README.md:5), parameters/optimizer state are
broadcast to keep replicas identical (README.md:286) and batches are split
with scatter (README.md:182). :class:`GradBucketer` implements exactly that
contract, MI355X-first:

* gradients are packed into a few large flat buckets (default 256 MiB: big
  messages keep RCCL/IPC on their bandwidth plateau and 288 GB of HBM makes the
  extra copy cheap), filled in reverse registration order = backward order;
* each bucket is all-reduced with ``async_op=True`` the moment its last
  gradient is produced (``register_post_accumulate_grad_hook``), so
  communication overlaps the rest of the backward pass on the backend's
  high-priority comm stream;
* the average is fused into the reduction itself (``ReduceOp.AVG``: the IPC
  kernels divide in registers, RCCL uses ``ncclAvg``) on the mi355x backend --
  no separate pass over the buckets; other backends get SUM plus one scale;
* :meth:`finish` waits and unpacks every GPU bucket with ONE K2 ``multi_copy``
  launch (per-parameter copies on CPU);
* gradient accumulation: backward passes inside ``with bucketer.no_sync():``
  only accumulate into ``.grad``; the first backward after it launches the
  reduction of the accumulated gradients. A second backward before
  :meth:`finish` (outside ``no_sync``) raises instead of silently dropping a
  micro-batch;
* ``wire="mxfp8_e4m3"``, ``wire="mxfp4_e2m1"`` or ``wire="mxfp6_e2m3"``: every bucket goes through
  ``all_reduce_compressed`` (block-scaled FP8, FP4 or FP6 on the links, f32 sums, AVG;
  parallel/compressed.py) instead of ``dist.all_reduce``. The default ``wire=None`` is the exact
  path above;
* ``error_feedback=True`` (with a wire): every bucket keeps what the quantizer dropped of its
  gradients -- a local residual for this rank's contribution and an owner residual for the chunk it
  requantizes -- and adds it to the next step's, so the quantization error cancels over steps instead
  of biasing every step the same way (docs/collectives.md "Error feedback"). The residuals are f32:
  4 bytes per gradient element, plus ``4 * 32 * cb`` bytes per bucket (``cb =
  ops.mx_chunk_blocks(bucket elements, world)``, about ``4 / world`` bytes per element more);
* ``rounding="stochastic"`` (with a wire, instead of error feedback): every quantization of a bucket
  rounds up or down with the probability of the distance, so what is sent is right on average and the
  error of a step is independent of the last one's, with no state at all (docs/collectives.md
  "Stochastic rounding"). Bucket ``b`` of synchronised step ``n`` uses the seed
  ``(seed + n * nbuckets + b) mod 2^64``.
* ``rotation="hadamard"`` (with a wire, together with either or neither of the two): every block of a
  bucket is rotated by a randomized Hadamard matrix before it is quantized and back afterwards, which
  keeps a block's small gradients on the grid next to an outlier (docs/collectives.md "Hadamard rotation").

``broadcast_parameters`` and ``scatter_batch`` cover the other two uses.
torch's own ``DistributedDataParallel`` also runs unchanged on this backend.
"""
from __future__ import annotations

import contextlib
from typing import Iterable, List

import torch
import torch.distributed as dist


def broadcast_parameters(module: torch.nn.Module, src: int = 0, group=None) -> None:
    """Make every replica identical to rank ``src`` (README.md:286)."""
    with torch.no_grad():
        for t in list(module.parameters()) + list(module.buffers()):
            dist.broadcast(t.data, src=src, group=group)


def scatter_batch(batch: torch.Tensor | None, shard_shape, dtype, device, src: int = 0, group=None) -> torch.Tensor:
    """Split ``batch`` (on ``src``) along dim 0 into equal shards, one per rank (README.md:182)."""
    world = dist.get_world_size(group)
    out = torch.empty(shard_shape, dtype=dtype, device=device)
    chunks = list(batch.chunk(world, 0)) if dist.get_rank(group) == src else None
    if chunks is not None:
        chunks = [c.contiguous() for c in chunks]
    dist.scatter(out, scatter_list=chunks, src=src, group=group)
    return out


class _Bucket:
    def __init__(self, params: List[torch.nn.Parameter], dtype, device):
        self.params = params
        self.numel = sum(p.numel() for p in params)
        self.flat = torch.empty(self.numel, dtype=dtype, device=device)
        self.offsets = []
        off = 0
        for p in params:
            self.offsets.append(off)
            off += p.numel()
        self.pending = 0
        self.work = None
        self.residual = self.owner_residual = None  # error feedback (GradBucketer(error_feedback=True))


class GradBucketer:
    """Overlapped, bucketed gradient all-reduce (average) for one module.

    ``error_feedback=True`` (needs ``wire``): each bucket owns a zero-initialised f32 local residual of
    ``flat.numel()`` elements and an owner residual of ``ops.mx_owner_residual_numel(flat.numel(), world)``
    and passes both to every ``all_reduce_compressed``. Memory: 4 bytes per gradient element plus
    ``4 * 32 * cb`` bytes per bucket. Backward passes inside ``no_sync()`` send nothing and leave the
    residuals alone. ``residuals`` lists them, ``reset_error_feedback()`` zeroes them.

    ``rounding="stochastic"`` (needs ``wire``, excludes ``error_feedback``): every ``all_reduce_compressed``
    rounds stochastically, bucket ``b`` of synchronised step ``n`` (``rounding_step``, counted by
    :meth:`finish`) with the seed ``(seed + n * len(buckets) + b) mod 2^64``. A backward inside
    ``no_sync()`` is no step.

    ``rotation="hadamard"`` with ``rotation_seed`` (needs ``wire``; composes with either of the above): every
    ``all_reduce_compressed`` rotates the blocks of the bucket before it quantizes them and back afterwards
    (docs/collectives.md "Hadamard rotation"). The seed is fixed for the object's life -- it does not step,
    the residuals live in the rotated domain of that one seed -- and must be the same on every rank."""

    def __init__(self, module: torch.nn.Module, group=None, bucket_bytes: int = 256 << 20,
                 average: bool = True, wire: str | None = None, error_feedback: bool = False,
                 rounding: str = "nearest", seed: int = 0, rotation: str | None = None, rotation_seed: int = 0):
        from .compressed import ROUNDINGS, _rotation_args

        self._rot = _rotation_args("GradBucketer", rotation, rotation_seed)
        if rotation is not None and wire is None:
            raise ValueError("GradBucketer: a rotation needs a compressed wire (wire=None sends exact gradients: "
                             "nothing is quantized)")
        self.rotation, self.rotation_seed = rotation, rotation_seed

        if rounding not in ROUNDINGS:
            raise ValueError(f"GradBucketer: unknown rounding {rounding!r} (supported: {', '.join(ROUNDINGS)})")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"GradBucketer: seed must be an int in [0, 2^64), got {seed!r}")
        if rounding == "stochastic" and wire is None:
            raise ValueError("GradBucketer: rounding='stochastic' needs a compressed wire (wire=None sends exact "
                             "gradients: nothing is rounded)")
        if rounding == "stochastic" and error_feedback:
            raise ValueError("GradBucketer: rounding='stochastic' and error_feedback=True are alternatives, not both")
        self.rounding, self.seed, self.rounding_step = rounding, seed, 0
        if error_feedback and wire is None:
            raise ValueError("GradBucketer: error_feedback=True needs a compressed wire (wire=None sends exact "
                             "gradients: there is no quantization error to feed back)")
        if wire is not None:
            from .compressed import WIRES

            if wire not in WIRES:
                raise ValueError(f"GradBucketer: unknown wire format {wire!r} (supported: {', '.join(WIRES)})")
            if not average:
                raise ValueError("GradBucketer: a compressed wire averages (average=True)")
        self.wire = wire
        self.error_feedback = bool(error_feedback)
        self.group = group
        self.average = average
        self.world = dist.get_world_size(group)
        params = [p for p in module.parameters() if p.requires_grad]
        self.buckets: List[_Bucket] = []
        self._where = {}
        cur, cur_bytes = [], 0
        # reverse order ~ the order backward produces gradients
        for p in reversed(params):
            nb = p.numel() * p.element_size()
            if cur and (cur_bytes + nb > bucket_bytes or p.dtype != cur[0].dtype or p.device != cur[0].device):
                self._add_bucket(cur)
                cur, cur_bytes = [], 0
            cur.append(p)
            cur_bytes += nb
        if cur:
            self._add_bucket(cur)
        if self.error_feedback:
            from ..ops import mx_owner_residual_numel

            for b in self.buckets:
                b.residual = torch.zeros(b.numel, dtype=torch.float32, device=b.flat.device)
                b.owner_residual = torch.zeros(mx_owner_residual_numel(b.numel, self.world, wire=wire),
                                               dtype=torch.float32, device=b.flat.device)
        self._hooks = [p.register_post_accumulate_grad_hook(self._on_grad) for p in params]
        self._sync = True
        # (a compressed wire divides before it requantizes: always fused)
        self._fused_avg = average and self.world > 1 and (wire is not None or _is_native(group, self.buckets))
        self._op = dist.ReduceOp.AVG if self._fused_avg else dist.ReduceOp.SUM
        self._reset()

    @contextlib.contextmanager
    def no_sync(self):
        """Backward passes in this context accumulate gradients locally (no communication)."""
        prev = self._sync
        self._sync = False
        try:
            yield
        finally:
            self._sync = prev

    def _add_bucket(self, ps):
        b = _Bucket(ps, ps[0].dtype, ps[0].device)
        idx = len(self.buckets)
        for i, p in enumerate(ps):
            self._where[id(p)] = (idx, i)
        self.buckets.append(b)

    def _reset(self):
        for b in self.buckets:
            b.pending = len(b.params)
            b.work = None

    def _on_grad(self, p: torch.nn.Parameter):
        if not self._sync:
            return
        bi, i = self._where[id(p)]
        b = self.buckets[bi]
        if b.pending <= 0:
            raise RuntimeError(
                "GradBucketer: a gradient arrived for a bucket that is already being reduced -- two backward "
                "passes without finish() in between; wrap the accumulation steps in `with bucketer.no_sync():`")
        off = b.offsets[i]
        b.flat[off:off + p.numel()].copy_(p.grad.reshape(-1))
        b.pending -= 1
        if b.pending == 0:
            b.work = self._reduce(b)

    def _reduce(self, b: _Bucket):
        if self.wire is not None:
            from .compressed import all_reduce_compressed

            if self.rounding == "stochastic":
                nb = len(self.buckets)
                seed = (self.seed + self.rounding_step * nb + self.buckets.index(b)) % (1 << 64)
                return all_reduce_compressed(b.flat, dist.ReduceOp.AVG, group=self.group, wire=self.wire,
                                             async_op=True, rounding="stochastic", seed=seed, **self._rot)
            return all_reduce_compressed(b.flat, dist.ReduceOp.AVG, group=self.group, wire=self.wire, async_op=True,
                                         residual=b.residual, owner_residual=b.owner_residual, **self._rot)
        return dist.all_reduce(b.flat, op=self._op, group=self.group, async_op=True)

    def finish(self) -> None:
        """Wait for every bucket, average, and write the result back into ``.grad``."""
        for b in self.buckets:
            if b.work is None:  # parameters without gradients this step: reduce what we have
                for p in b.params:
                    if p.grad is None:
                        p.grad = torch.zeros_like(p)
                for p, off in zip(b.params, b.offsets):
                    b.flat[off:off + p.numel()].copy_(p.grad.reshape(-1))
                b.work = self._reduce(b)
        for b in self.buckets:
            b.work.wait()
            if self.average and self.world > 1 and not self._fused_avg:
                b.flat.div_(self.world)
            _unpack(b)
        self.rounding_step += 1
        self._reset()

    @property
    def residuals(self):
        """[(local residual, owner residual)] per bucket, the live f32 tensors; empty without error feedback."""
        return [(b.residual, b.owner_residual) for b in self.buckets] if self.error_feedback else []

    def reset_error_feedback(self) -> None:
        """Zero every residual (after a change of learning-rate regime, a loss-scale change, a restart)."""
        for local, owner in self.residuals:
            local.zero_()
            owner.zero_()

    def remove(self) -> None:
        for h in self._hooks:
            h.remove()


def _is_native(group, buckets) -> bool:
    """Is ``group`` served by the mi355x backend for the buckets' device (fused AVG)?"""
    if not buckets:
        return False
    try:
        from .backend import native_backend

        native_backend(group, buckets[0].flat.device.type)
        return True
    except Exception:
        return False


def _unpack(b: _Bucket) -> None:
    views = [b.flat[off:off + p.numel()] for p, off in zip(b.params, b.offsets)]
    grads = [p.grad.reshape(-1) if p.grad.is_contiguous() else None for p in b.params]
    if b.flat.is_cuda and all(g is not None for g in grads):
        try:
            from ..ops import multi_copy

            multi_copy(views, grads)  # one launch for the whole bucket
            return
        except Exception:  # extension unavailable: plain copies below
            pass
    for p, v in zip(b.params, views):
        p.grad.copy_(v.view_as(p.grad))


def allreduce_gradients(params: Iterable[torch.nn.Parameter], group=None, average: bool = True) -> None:
    """Non-overlapped reference implementation: one coalesced all-reduce per call."""
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        return
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat, group=group)
    if average:
        flat.div_(dist.get_world_size(group))
    off = 0
    for g in grads:
        g.copy_(flat[off:off + g.numel()].view_as(g))
        off += g.numel()
