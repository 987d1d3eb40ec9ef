"""ZeRO-style sharded data parallelism on the mi355x backend.

The reference motivates ``all_gather`` with "have a copy of the information on
all the devices" (README.md:254) and data parallelism with gradient averaging
(README.md:5); BASELINE.json names the ZeRO-style parameter gather (bf16
``all_gather`` of 4 GiB per rank on 8 GPUs) as one of its configs. This module
is that workload: :class:`ShardedOptimizer` keeps ONE full copy of the
parameters for forward/backward but only 1/world of the optimizer state and
fp32 master weights per rank, and each step is

1. ``reduce_scatter_tensor`` (``ReduceOp.AVG``: divided inside the reduction on
   mi355x) of each gradient bucket -> this rank's shard of the bucket, launched
   with ``async_op=True`` the moment backward has produced the bucket's last
   gradient (``register_post_accumulate_grad_hook``), so the reduction overlaps
   the rest of the backward pass;
2. the inner optimizer's step on this rank's (fp32) master shard only;
3. ``all_gather_into_tensor`` of the updated shards (in the parameter dtype,
   e.g. bf16) straight back into the flat parameter buffer, one per bucket.

MI355X-first layout: every parameter of one (device, dtype) is a view into one
flat buffer (and its ``.grad`` a view into one flat gradient buffer, which
autograd accumulates into in place), laid out in backward order and cut into
buckets of ``bucket_bytes`` (default 256 MiB: large messages keep RCCL and the
IPC kernels over xGMI on their bandwidth plateau). No pack/unpack copies: the
collectives read and write the buffers the model uses. Buckets are padded to a
multiple of ``world x 64`` elements so every shard is 16-byte aligned (zero-copy
IPC). With 288 GB of HBM per GPU the full parameter copy is cheap; what sharding
saves is the optimizer state (2 fp32 words per parameter for Adam) and the
master weights.

Gradient accumulation: backward passes inside ``with opt.no_sync():`` only
accumulate; a second backward outside it before :meth:`step` raises instead of
double-reducing a bucket.

Compressed links: ``grad_wire="mxfp8_e4m3"`` sends every gradient bucket through
``reduce_scatter_compressed`` (AVG, divided inside the fold) and
``param_wire="mxfp8_e4m3"`` every parameter bucket through
``all_gather_compressed`` (parallel/compressed.py; 3.9x / 1.94x fewer bytes on
the links for f32 / bf16). Either may be ``"mxfp4_e2m1"`` instead (7.5x / 3.76x
fewer bytes, an error bound five times coarser), independently of the other:
FP4 gradients with FP8 parameters is the ZeRO++ setting. Master weights and optimizer state stay exact f32:
only the replicated copy used for forward and backward is the dequantized
wire, the same bits on every rank. Spaces of other dtypes keep the uncompressed
calls; the defaults (``None``) are the uncompressed path, call for call.

``grad_error_feedback=True`` (with a ``grad_wire``): every space on the gradient wire keeps an f32
residual of its flat gradient's size -- 4 bytes per gradient element -- that
``reduce_scatter_compressed`` adds to this rank's gradients before it quantizes them and leaves
holding what the quantizer dropped (docs/collectives.md "Error feedback"), so the error cancels over
steps. The fold is not quantized again, so there is no owner residual; ``param_wire`` is untouched
(parameters are not accumulated). ``state_dict()`` saves the residuals, ``load_state_dict()`` restores
them (a checkpoint without them loads as zeros).

``grad_rounding="stochastic"`` (with a ``grad_wire``, instead of ``grad_error_feedback``): the
reduce-scatters round this rank's gradients stochastically (docs/collectives.md "Stochastic rounding"):
unbiased, no state but a step counter. Gradient bucket ``b`` (counted over all spaces) of synchronised
step ``n`` uses the seed ``(grad_seed + n * nbuckets + b) mod 2^64``; ``state_dict()`` saves ``n`` as
``grad_rounding_step`` (a checkpoint without it loads as 0). ``param_wire`` stays nearest.

``grad_rotation="hadamard"`` / ``param_rotation="hadamard"`` (each with its wire) with one ``rotation_seed``:
the reduce-scatters / the all-gathers rotate every 32-element block by a randomized Hadamard matrix before
they quantize it and back afterwards (docs/collectives.md "Hadamard rotation"), which is what makes the
narrow wires usable for heavy-tailed gradients. The seed never steps and is not saved: the gradient
residuals live in the rotated domain of that seed.

``state_dict()`` / ``load_state_dict()`` save and restore this rank's shard
(sharded checkpoint: every rank writes its own file) and re-gather the
parameters on load.
"""
from __future__ import annotations

import contextlib
import copy
from typing import Dict, Iterable, List

import torch
import torch.distributed as dist

_ALIGN = 64  # elements; x world = padding unit of every bucket


class _Bucket:
    """A contiguous range [off, off + padded) of one flat space; this rank owns
    [off + rank * shard, off + (rank + 1) * shard) of it, stored at
    [soff, soff + shard) of the space's shard buffers."""

    def __init__(self, idx: List[int], off: int, padded: int, world: int, soff: int):
        self.idx, self.off, self.padded = idx, off, padded
        self.shard = padded // world
        self.soff = soff
        self.pending = len(idx)
        self.work = None


class _FlatSpace:
    """All parameters of one (device, dtype): flat params, flat grads, buckets, this rank's shards."""

    def __init__(self, params: List[torch.nn.Parameter], world: int, rank: int, master_dtype, bucket_bytes: int):
        p0 = params[0]
        self.params = params  # backward order
        self.dtype, self.device = p0.dtype, p0.device
        unit = world * _ALIGN
        esize = p0.element_size()
        self.offsets = []
        self.buckets: List[_Bucket] = []
        off = soff = 0
        cur, cur_n = [], 0

        def close():
            nonlocal off, soff, cur, cur_n
            padded = (cur_n + unit - 1) // unit * unit
            b = _Bucket(cur, off, padded, world, soff)
            self.buckets.append(b)
            off += padded
            soff += b.shard
            cur, cur_n = [], 0

        for i, p in enumerate(params):
            if cur and (cur_n + p.numel()) * esize > bucket_bytes:
                close()
            self.offsets.append(off + cur_n)
            cur.append(i)
            cur_n += p.numel()
        close()
        self.where = {}
        for bi, b in enumerate(self.buckets):
            for i in b.idx:
                self.where[id(params[i])] = bi
        self.padded, self.shard_total = off, soff
        self.rank = rank
        with torch.no_grad():
            self.flat = torch.zeros(off, dtype=self.dtype, device=self.device)
            self.grad = torch.zeros(off, dtype=self.dtype, device=self.device)
            for p, o in zip(params, self.offsets):
                self.flat[o:o + p.numel()].copy_(p.detach().reshape(-1))
            self.attach()
            self.grad_shard = torch.empty(soff, dtype=self.dtype, device=self.device)
            self.param_shard = torch.empty(soff, dtype=self.dtype, device=self.device)
            for b in self.buckets:
                self.param_shard[b.soff:b.soff + b.shard].copy_(self.own(self.flat, b))
            md = master_dtype if self.dtype.is_floating_point else self.dtype
            self.master = self.param_shard.to(md).clone()

    def own(self, buf: torch.Tensor, b: _Bucket) -> torch.Tensor:
        lo = b.off + self.rank * b.shard
        return buf[lo:lo + b.shard]

    def attach(self) -> None:
        """(Re)point every parameter and its ``.grad`` at the flat buffers."""
        for p, o in zip(self.params, self.offsets):
            n = p.numel()
            p.data = self.flat[o:o + n].view_as(p)
            p.grad = self.grad[o:o + n].view_as(p)

    def sync_grads_in(self, b: _Bucket) -> None:
        """Gradients replaced behind our back (``set_to_none``, manual assignment) are
        copied into the flat buffer and re-attached."""
        for i in b.idx:
            p, o = self.params[i], self.offsets[i]
            view = self.grad[o:o + p.numel()]
            if p.grad is None:
                view.zero_()
            elif p.grad.data_ptr() != view.data_ptr():
                view.copy_(p.grad.reshape(-1))
            p.grad = view.view_as(p)


class ShardedOptimizer:
    """ZeRO-style (optimizer state + master weights sharded) data-parallel optimizer.

    Usage::

        opt = ShardedOptimizer(model.parameters(), torch.optim.AdamW, lr=1e-3)
        for x, y in batches:             # this rank's batch shard
            loss_fn(model(x), y).backward()   # bucket reduce-scatters start here
            opt.step()                    # wait, sharded step, all-gather
            opt.zero_grad()

    ``broadcast_from`` (default 0) makes every replica start from that rank's
    parameters; ``master_dtype`` (default fp32) is the dtype of the sharded
    master weights and optimizer state for floating-point parameters -- with
    bf16 parameters the optimizer math runs in fp32 and only the gathered
    parameters are bf16. ``overlap=False`` defers every reduce-scatter to
    :meth:`step`. ``grad_wire`` / ``param_wire`` (default ``None``: uncompressed;
    ``"mxfp8_e4m3"``, ``"mxfp4_e2m1"`` or ``"mxfp6_e2m3"``, each on its own) pick the wire of the reduce-scatters / the all-gathers of
    float32, bfloat16 and float16 parameters. ``grad_error_feedback=True`` (needs ``grad_wire``) carries the
    quantization error of this rank's gradients from step to step in an f32 residual, 4 bytes per gradient
    element, saved by :meth:`state_dict`. ``grad_rounding="stochastic"`` with ``grad_seed`` (needs ``grad_wire``,
    excludes ``grad_error_feedback``) rounds the gradients on the wire stochastically, a fresh seed per bucket
    and step; :meth:`state_dict` saves the step counter. ``grad_rotation="hadamard"`` / ``param_rotation="hadamard"``
    (each needs its wire; ``rotation_seed`` serves both) rotate every block by a randomized Hadamard matrix before it
    is quantized and back afterwards (docs/collectives.md "Hadamard rotation"); the seed is fixed for the object's
    life, must be the same on every rank and is a constructor argument, not part of :meth:`state_dict` -- a
    checkpoint with gradient residuals is loaded into an optimizer built with the seed that wrote it. One parameter group: the inner optimizer's hyper-parameters
    come from ``**opt_kwargs``.
    """

    def __init__(self, params: Iterable[torch.nn.Parameter], optimizer_cls=torch.optim.SGD, group=None,
                 master_dtype: torch.dtype = torch.float32, broadcast_from: int | None = 0,
                 bucket_bytes: int = 256 << 20, overlap: bool = True, grad_wire: str | None = None,
                 param_wire: str | None = None, grad_error_feedback: bool = False, grad_rounding: str = "nearest",
                 grad_seed: int = 0, grad_rotation: str | None = None, param_rotation: str | None = None,
                 rotation_seed: int = 0, **opt_kwargs):
        from .compressed import ROUNDINGS, WIRES, _rotation_args

        self._grad_rot = _rotation_args("ShardedOptimizer", grad_rotation, rotation_seed)
        self._param_rot = _rotation_args("ShardedOptimizer", param_rotation, rotation_seed)
        for name, rot, w in (("grad", grad_rotation, grad_wire), ("param", param_rotation, param_wire)):
            if rot is not None and w is None:
                raise ValueError(f"ShardedOptimizer: {name}_rotation needs a {name}_wire ({name}_wire=None sends exact "
                                 "values: nothing is quantized)")
        self.grad_rotation, self.param_rotation, self.rotation_seed = grad_rotation, param_rotation, rotation_seed

        if grad_rounding not in ROUNDINGS:
            raise ValueError(f"ShardedOptimizer: unknown grad_rounding {grad_rounding!r} "
                             f"(supported: {', '.join(ROUNDINGS)})")
        if isinstance(grad_seed, bool) or not isinstance(grad_seed, int) or not 0 <= grad_seed < 1 << 64:
            raise ValueError(f"ShardedOptimizer: grad_seed must be an int in [0, 2^64), got {grad_seed!r}")
        if grad_rounding == "stochastic" and grad_wire is None:
            raise ValueError("ShardedOptimizer: grad_rounding='stochastic' needs a grad_wire (grad_wire=None sends "
                             "exact gradients: nothing is rounded)")
        if grad_rounding == "stochastic" and grad_error_feedback:
            raise ValueError("ShardedOptimizer: grad_rounding='stochastic' and grad_error_feedback=True are "
                             "alternatives, not both")
        self.grad_rounding, self.grad_seed, self.grad_rounding_step = grad_rounding, grad_seed, 0

        if grad_error_feedback and grad_wire is None:
            raise ValueError("ShardedOptimizer: grad_error_feedback=True needs a grad_wire (grad_wire=None sends "
                             "exact gradients: there is no quantization error to feed back)")
        self.grad_error_feedback = bool(grad_error_feedback)

        for name, w in (("grad_wire", grad_wire), ("param_wire", param_wire)):
            if w is not None and w not in WIRES:
                raise ValueError(f"ShardedOptimizer: unknown {name} {w!r} (supported: {', '.join(WIRES)})")
        self.grad_wire, self.param_wire = grad_wire, param_wire
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("ShardedOptimizer: no parameters that require grad")
        if broadcast_from is not None:
            src = dist.get_global_rank(group, broadcast_from) if group is not None else broadcast_from
            with torch.no_grad():
                for p in params:
                    dist.broadcast(p.data, src=src, group=group)
        by_key: Dict[tuple, List[torch.nn.Parameter]] = {}
        for p in reversed(params):  # ~ the order backward produces gradients
            by_key.setdefault((str(p.device), p.dtype), []).append(p)
        self.spaces = [_FlatSpace(ps, self.world, self.rank, master_dtype, bucket_bytes) for ps in by_key.values()]
        self._space_of = {id(p): s for s in self.spaces for p in s.params}
        self._bucket_no = {id(b): i for i, b in enumerate(b for s in self.spaces for b in s.buckets)}
        for s in self.spaces:  # the error-feedback residual of the space's flat gradient, or None
            s.grad_residual = (torch.zeros(s.padded, dtype=torch.float32, device=s.device)
                               if self.grad_error_feedback and self._on_wire(s, grad_wire) else None)
        self.inner = optimizer_cls([s.master for s in self.spaces], **opt_kwargs)
        self._avg = self._fused_avg()
        self._op = dist.ReduceOp.AVG if self._avg else dist.ReduceOp.SUM
        self._sync = True
        self.overlapped = 0  # buckets whose reduce-scatter started during backward (last step())
        self._hooks = [p.register_post_accumulate_grad_hook(self._on_grad) for p in params] if overlap else []

    def _fused_avg(self) -> bool:
        """mi355x divides inside the reduction (ReduceOp.AVG); others get SUM + one scale."""
        try:
            from .backend import native_backend

            native_backend(self.group, self.spaces[0].device.type)
            return True
        except Exception:
            return False

    @property
    def param_groups(self):
        return self.inner.param_groups

    @contextlib.contextmanager
    def no_sync(self):
        """Backward passes in this context accumulate gradients locally (no communication)."""
        prev = self._sync
        self._sync = False
        try:
            yield
        finally:
            self._sync = prev

    @staticmethod
    def _on_wire(s: _FlatSpace, wire) -> bool:
        from .. import ops

        return wire is not None and s.dtype in ops.MX_DTYPES

    def _fence(self, s: _FlatSpace) -> None:
        """An uncompressed call next to compressed ones (a space of another dtype): the compressed calls
        run on a side stream the backend does not order its own streams against, and two collectives of
        one group must not overlap -- the current stream, which the backend does wait for, waits for it."""
        if s.device.type == "cuda" and (self.grad_wire is not None or self.param_wire is not None):
            from .compressed import order_after_compressed

            order_after_compressed(s.device)

    def _launch(self, s: _FlatSpace, b: _Bucket) -> None:
        s.sync_grads_in(b)
        if self._on_wire(s, self.grad_wire):
            from .compressed import reduce_scatter_compressed

            if self.grad_rounding == "stochastic":
                seed = (self.grad_seed + self.grad_rounding_step * len(self._bucket_no)
                        + self._bucket_no[id(b)]) % (1 << 64)
                b.work = reduce_scatter_compressed(s.grad_shard[b.soff:b.soff + b.shard],
                                                   s.grad[b.off:b.off + b.padded], op=dist.ReduceOp.AVG,
                                                   group=self.group, wire=self.grad_wire, async_op=True,
                                                   rounding="stochastic", seed=seed, **self._grad_rot)
                return
            b.work = reduce_scatter_compressed(s.grad_shard[b.soff:b.soff + b.shard], s.grad[b.off:b.off + b.padded],
                                               op=dist.ReduceOp.AVG, group=self.group, wire=self.grad_wire,
                                               async_op=True,
                                               residual=None if s.grad_residual is None
                                               else s.grad_residual[b.off:b.off + b.padded], **self._grad_rot)
            return
        self._fence(s)
        b.work = dist.reduce_scatter_tensor(s.grad_shard[b.soff:b.soff + b.shard], s.grad[b.off:b.off + b.padded],
                                            op=self._op, group=self.group, async_op=True)

    def _on_grad(self, p: torch.nn.Parameter) -> None:
        if not self._sync:
            return
        s = self._space_of[id(p)]
        b = s.buckets[s.where[id(p)]]
        if b.pending <= 0:
            raise RuntimeError(
                "ShardedOptimizer: a gradient arrived for a bucket that is already being reduced -- two backward "
                "passes without step() in between; wrap the accumulation steps in `with opt.no_sync():`")
        b.pending -= 1
        if b.pending == 0:
            with torch.no_grad():
                self._launch(s, b)

    def zero_grad(self, set_to_none: bool = False) -> None:  # noqa: ARG002 - the flat buffer stays attached
        for s in self.spaces:
            s.grad.zero_()
            s.attach()

    @torch.no_grad()
    def step(self) -> None:
        self.overlapped = sum(b.work is not None for s in self.spaces for b in s.buckets)
        for s in self.spaces:
            for b in s.buckets:
                if b.work is None:  # not launched during backward (overlap off, unused params)
                    self._launch(s, b)
        for s in self.spaces:
            for b in s.buckets:
                b.work.wait()
                b.work = None
                b.pending = len(b.idx)
            g = s.grad_shard if s.master.dtype == s.dtype else s.grad_shard.to(s.master.dtype)
            if not self._avg and self.world > 1 and not self._on_wire(s, self.grad_wire):  # (a wire divides inside)
                g = g / self.world
            s.master.grad = g
        self.grad_rounding_step += 1
        self.inner.step()
        self._gather()

    @torch.no_grad()
    def _gather(self) -> None:
        works = []
        for s in self.spaces:
            s.param_shard.copy_(s.master)
            for b in s.buckets:
                if self._on_wire(s, self.param_wire):
                    from .compressed import all_gather_compressed

                    works.append(all_gather_compressed(s.flat[b.off:b.off + b.padded],
                                                       s.param_shard[b.soff:b.soff + b.shard], group=self.group,
                                                       wire=self.param_wire, async_op=True, **self._param_rot))
                    continue
                self._fence(s)
                works.append(dist.all_gather_into_tensor(s.flat[b.off:b.off + b.padded],
                                                         s.param_shard[b.soff:b.soff + b.shard],
                                                         group=self.group, async_op=True))
        for w in works:
            w.wait()

    def remove_hooks(self) -> None:
        for h in self._hooks:
            h.remove()
        self._hooks = []

    # ---- sharded checkpoint / resume
    def _layout(self):
        return [(str(s.dtype), [(b.off, b.padded) for b in s.buckets]) for s in self.spaces]

    def state_dict(self) -> dict:
        """This rank's shard: master weights + inner optimizer state (+ layout check), and with
        ``grad_error_feedback`` this rank's gradient residuals (``grad_residual``: per space a CPU clone, or None)."""
        for s in self.spaces:  # (a reduce-scatter still in flight on the side stream is updating its residual)
            if s.grad_residual is not None:
                self._fence(s)
        extra = {"grad_residual": [None if s.grad_residual is None else s.grad_residual.detach().cpu().clone()
                                   for s in self.spaces]} if self.grad_error_feedback else {}
        if self.grad_rounding == "stochastic":
            extra["grad_rounding_step"] = self.grad_rounding_step
        return {
            **extra,
            "world": self.world,
            "rank": self.rank,
            "layout": self._layout(),
            "master": [s.master.detach().clone() for s in self.spaces],
            "inner": copy.deepcopy(self.inner.state_dict()),  # a snapshot, not live state
        }

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        if sd["world"] != self.world or sd["rank"] != self.rank:
            raise ValueError(f"ShardedOptimizer: checkpoint is rank {sd['rank']}/{sd['world']}, "
                             f"this is rank {self.rank}/{self.world}")
        if sd["layout"] != self._layout():
            raise ValueError("ShardedOptimizer: checkpoint parameter layout differs from this model's")
        for s, m in zip(self.spaces, sd["master"]):
            s.master.copy_(m)
        self.inner.load_state_dict(sd["inner"])
        self.grad_rounding_step = int(sd.get("grad_rounding_step", 0))  # (a checkpoint without it: 0)
        saved = sd.get("grad_residual") or [None] * len(self.spaces)  # (an older checkpoint: zeros)
        for s, r in zip(self.spaces, saved):
            if s.grad_residual is None:
                continue
            self._fence(s)
            if r is None:
                s.grad_residual.zero_()
            else:
                s.grad_residual.copy_(r)
        self._gather()

    def sharded_state_bytes(self) -> int:
        """Bytes of master weights + optimizer state held by this rank."""
        n = sum(s.master.numel() * s.master.element_size() for s in self.spaces)
        for st in self.inner.state.values():
            for v in st.values():
                if torch.is_tensor(v):
                    n += v.numel() * v.element_size()
        return n


__all__ = ["ShardedOptimizer"]
