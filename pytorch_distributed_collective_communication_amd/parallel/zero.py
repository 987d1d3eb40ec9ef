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

``max_grad_norm=c`` clips the reduced gradients by their global 2-norm (docs/collectives.md "Gradient
clipping"), between the last bucket's wait and the inner optimizer's step -- the one place where it can be
done: after the reduce-scatter a rank holds only its shard, so ``torch.nn.utils.clip_grad_norm_`` on the model
would see the local, unreduced gradients. ``ops.sumsq`` of the shards (one read, deterministic), an
``all_reduce`` of the f64 scalar (every rank folds in rank order: the same bits, so the same coefficient,
everywhere), and ``ops.clip_scale`` in place of the cast to the master dtype: the coefficient rides on the
cast bf16 / f16 parameters need anyway, and f32 parameters are scaled in place. The norm never reaches the host;
``opt.grad_norm`` holds it (before clipping) as a 0-d device tensor.

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


class _FusedAdamW:
    """The built-in step of ``ShardedOptimizer(params, "adamw")``: per space ``exp_avg`` / ``exp_avg_sq`` f32 shards,
    one step counter, one parameter group read at every step, and ``ops.adamw_step`` -- one pass over the gradient
    shard, the state and the master that also writes ``param_shard`` (docs/collectives.md "Fused AdamW step").
    ``state`` / ``param_groups`` / ``state_dict()`` / ``load_state_dict()`` are those of ``torch.optim.AdamW`` over
    the masters, one parameter per space, so checkpoints go either way. ``state_format="mxfp8_e4m3"`` keeps the two
    moments as the uint8 buffers of ``ops.adamw_state_pack`` (docs/collectives.md "8-bit AdamW state"); ``state_dict()``
    unpacks them to f32 and ``load_state_dict()`` packs, so the checkpoint format stays torch's."""

    DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    # what torch.optim.AdamW writes next to them, and the only values this step implements
    TORCH_FLAGS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                       decoupled_weight_decay=True)

    def __init__(self, spaces, state_format=None, **kw):
        from .. import ops

        self.packed = ops._adamw_state_format(state_format, "ShardedOptimizer")
        self.state_format = state_format
        unknown = sorted(set(kw) - set(self.DEFAULTS))
        if unknown:
            raise ValueError(f"ShardedOptimizer: 'adamw' takes {', '.join(self.DEFAULTS)}, got {', '.join(unknown)}")
        for s in spaces:
            if s.dtype not in (torch.float32, torch.bfloat16, torch.float16) or s.master.dtype != torch.float32:
                raise ValueError(f"ShardedOptimizer: 'adamw' steps float32, bfloat16 and float16 parameters on a float32 "
                                 f"master, got {s.dtype} parameters with a {s.master.dtype} master")
        self.param_groups = [{**self.DEFAULTS, **kw}]
        self.masters = [s.master for s in spaces]
        self.state = {i: dict(zip(("exp_avg", "exp_avg_sq"), self._fresh(s.master))) for i, s in enumerate(spaces)}
        self.steps = 0

    def _fresh(self, master, exp_avg=None, exp_avg_sq=None):
        """The two moments of a space as this optimizer holds them, zeros unless given (f32, any device). The packed
        state of zeros is not zero bytes: an all-zero block carries scale byte 127."""
        from .. import ops

        m, v = (torch.zeros_like(master) if t is None else t.to(device=master.device, dtype=torch.float32).reshape(-1)
                for t in (exp_avg, exp_avg_sq))
        return ops.adamw_state_pack(m, v) if self.packed else (m, v)

    def step(self, spaces, total, max_norm, param_wire=None) -> None:
        """One step of every space. A space with ``param_wires`` (one buffer per bucket; ShardedOptimizer's
        ``fused_param_wire``) is stepped bucket by bucket, each launch writing the bucket's ``param_wire`` wire instead
        of ``param_shard`` (docs/collectives.md "Parameter wire from the step")."""
        from .. import ops

        g = self.param_groups[0]
        self.steps += 1
        kw = dict(lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"], step=self.steps,
                  total=total, max_norm=None if total is None else max_norm)
        for i, s in enumerate(spaces):
            m, v = self.state[i]["exp_avg"], self.state[i]["exp_avg_sq"]
            if s.param_wires is None:
                ops.adamw_step(s.grad_shard, s.master, m, v, param_out=s.param_shard, **kw,
                               **({"state_format": self.state_format} if self.packed else {}))
                continue
            for b, w in zip(s.buckets, s.param_wires):
                sl = slice(b.soff, b.soff + b.shard)
                state = (dict(state_format=self.state_format, state_offset=b.soff) if self.packed else {})
                ops.adamw_step(s.grad_shard[sl], s.master[sl], *((m, v) if self.packed else (m[sl], v[sl])), wire_out=w,
                               wire=param_wire, wire_dtype=s.dtype, **kw, **state)

    def _f32_state(self, i) -> dict:
        from .. import ops

        st = self.state[i]
        if not self.packed:
            return st
        return dict(zip(("exp_avg", "exp_avg_sq"),
                        ops.adamw_state_unpack(st["exp_avg"], st["exp_avg_sq"], self.masters[i].numel())))

    def state_dict(self) -> dict:
        state = {i: {"step": torch.tensor(float(self.steps)), **self._f32_state(i)} for i in self.state} if self.steps else {}
        return {"state": state,
                "param_groups": [{**self.param_groups[0], **self.TORCH_FLAGS, "params": list(range(len(self.state)))}]}

    def load_state_dict(self, sd: dict) -> None:
        (group,) = sd["param_groups"]
        if len(group["params"]) != len(self.state):
            raise ValueError(f"ShardedOptimizer: the checkpoint has {len(group['params'])} parameters, "
                             f"'adamw' has {len(self.state)} spaces")
        for k, v in self.TORCH_FLAGS.items():
            if k in ("amsgrad", "maximize", "decoupled_weight_decay") and group.get(k, v) != v:
                raise ValueError(f"ShardedOptimizer: 'adamw' cannot continue a checkpoint written with {k}={group[k]!r}")
        self.param_groups[0].update({k: group[k] for k in self.DEFAULTS})
        steps = {int(st["step"]) for st in sd["state"].values()}
        if len(steps) > 1 or (steps and len(sd["state"]) != len(self.state)):
            raise ValueError(f"ShardedOptimizer: 'adamw' keeps one step counter, the checkpoint has {sorted(steps)}")
        self.steps = steps.pop() if steps else 0
        for i, st in self.state.items():
            saved = sd["state"].get(i, {})
            fresh = self._fresh(self.masters[i], saved.get("exp_avg"), saved.get("exp_avg_sq"))
            for t, new in zip((st["exp_avg"], st["exp_avg_sq"]), fresh):
                t.copy_(new.view_as(t))


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
    checkpoint with gradient residuals is loaded into an optimizer built with the seed that wrote it.
    ``max_grad_norm`` (default ``None``: :meth:`step` is what it is without the argument, call for call; else a
    positive finite float; f32 / bf16 / f16 parameters, ``master_dtype`` float32 or the parameters' own) clips the
    reduced gradients to that global 2-norm before the inner optimizer sees them, with the coefficient of
    ``torch.nn.utils.clip_grad_norm_``, ``min(1, max_grad_norm / (norm + 1e-6))`` in f32; ``grad_norm`` is then the
    norm before clipping, a 0-d float32 tensor on the device (``None`` before the first step), the same bits on every
    rank. Non-finite norms behave as ``clip_grad_norm_(error_if_nonfinite=False)``: an infinite norm gives
    coefficient 0 (finite elements become 0, infinite ones NaN), a NaN norm makes every element NaN. On a backend that
    cannot divide inside the reduction the shard is divided by the world size first, in its own dtype. Nothing of
    it is part of :meth:`state_dict`. One parameter group: the inner optimizer's hyper-parameters
    come from ``**opt_kwargs``.

    ``optimizer_cls="adamw"`` (with ``lr``, ``betas``, ``eps``, ``weight_decay``; torch's defaults) selects the
    built-in step instead of an inner torch optimizer: per space one ``ops.adamw_step`` reads the gradient shard, the
    clip coefficient (with ``max_grad_norm``), ``exp_avg`` / ``exp_avg_sq`` and the master and writes the state, the
    master and ``param_shard`` in one pass (docs/collectives.md "Fused AdamW step"). f32 / bf16 / f16 parameters and a
    float32 master, else ``ValueError``. ``param_groups[0]`` is read at every step; ``state_dict()["inner"]`` has
    ``torch.optim.AdamW.state_dict()``'s format, so a checkpoint of ``optimizer_cls=torch.optim.AdamW`` loads into
    ``"adamw"`` and the reverse. Any other string raises ``ValueError``; a class behaves as it always did.

    With ``"adamw"`` and a ``param_wire``, on the GPU at world > 1 and without ``param_rotation``, the step emits the
    parameter wire itself (read-only ``fused_param_wire``; docs/collectives.md "Parameter wire from the step"): one
    ``ops.adamw_step(wire_out=...)`` per bucket writes the bucket's wire, which the all-gather sends as it is, instead
    of ``param_shard`` and a quantizer that reads it back. ``param_shard`` is not maintained in this mode (it holds
    what the last checkpoint load left there); ``flat`` and the masters are exactly what the unfused sequence gives.

    ``state_format="mxfp8_e4m3"`` (with ``"adamw"`` only; default ``None``: f32 state) holds ``exp_avg`` and the square
    root of ``exp_avg_sq`` as block-scaled 8-bit buffers, 2 x 33/32 bytes per element instead of 8, read and
    requantized by the same one pass (docs/collectives.md "8-bit AdamW state"). ``state_dict()["inner"]`` still has
    torch's f32 format; :meth:`sharded_state_bytes` counts the packed buffers. Any other string, or a
    ``state_format`` next to an inner optimizer class, raises ``ValueError``.
    """

    def __init__(self, params: Iterable[torch.nn.Parameter], optimizer_cls=torch.optim.SGD, group=None,
                 master_dtype: torch.dtype = torch.float32, broadcast_from: int | None = 0,
                 bucket_bytes: int = 256 << 20, overlap: bool = True, grad_wire: str | None = None,
                 param_wire: str | None = None, grad_error_feedback: bool = False, grad_rounding: str = "nearest",
                 grad_seed: int = 0, grad_rotation: str | None = None, param_rotation: str | None = None,
                 rotation_seed: int = 0, max_grad_norm: float | None = None, state_format: str | None = None,
                 **opt_kwargs):
        from .compressed import ROUNDINGS, WIRES, _rotation_args

        self._fused = isinstance(optimizer_cls, str)  # the built-in step, not an inner torch optimizer
        if self._fused and optimizer_cls != "adamw":
            raise ValueError(f"ShardedOptimizer: unknown built-in optimizer {optimizer_cls!r} (supported: 'adamw'; "
                             "anything else is passed as a class)")
        if state_format is not None:
            from .. import ops

            ops._adamw_state_format(state_format, "ShardedOptimizer")
            if not self._fused:
                raise ValueError("ShardedOptimizer: state_format is the built-in 'adamw' step's; an inner optimizer "
                                 "class keeps its own state")
            opt_kwargs["state_format"] = state_format
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) \
                    or not 0 < max_grad_norm < float("inf"):
                raise ValueError(f"ShardedOptimizer: max_grad_norm must be a positive finite number or None, "
                                 f"got {max_grad_norm!r}")
            max_grad_norm = float(max_grad_norm)
        self.max_grad_norm, self.grad_norm = max_grad_norm, None

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
        if max_grad_norm is not None:
            from .. import ops

            for s in self.spaces:
                if s.dtype not in ops.CLIP_DTYPES:
                    raise ValueError(f"ShardedOptimizer: max_grad_norm clips float32, bfloat16 and float16 parameters, "
                                     f"got {s.dtype}")
                if s.master.dtype not in (torch.float32, s.dtype):
                    raise ValueError(f"ShardedOptimizer: with max_grad_norm the master_dtype is float32 or the "
                                     f"parameters' own ({s.dtype}), got {s.master.dtype}")
                # the master gradient: the shard itself, scaled in place, or an f32 buffer the scaled cast fills
                # (the built-in step needs neither: its kernel takes the coefficient)
                if not self._fused:
                    s.master_grad = s.grad_shard if s.master.dtype == s.dtype else torch.empty_like(s.master)
        # the built-in step writes the parameter wire itself where the gather would only quantize param_shard again:
        # per bucket one wire buffer, allocated once (None: the space keeps param_shard and today's path)
        for s in self.spaces:
            s.param_wires = None
            if self._fused and self.world > 1 and param_rotation is None and self._on_wire(s, param_wire) \
                    and s.device.type == "cuda":
                from .. import ops

                s.param_wires = [torch.empty(ops.mx_wire_bytes(b.shard, 1, wire=param_wire), dtype=torch.uint8,
                                             device=s.device) for b in s.buckets]
        self.inner = (_FusedAdamW(self.spaces, **opt_kwargs) if self._fused
                      else optimizer_cls([s.master for s in self.spaces], **opt_kwargs))
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

    @property
    def fused_param_wire(self) -> bool:
        """Whether the built-in step emits the parameter wire itself (class docstring, ``param_wire``)."""
        return any(s.param_wires is not None for s in self.spaces)

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
            if self.max_grad_norm is not None or self._fused:  # (_clip below sets every master gradient; the
                if not self._avg and self.world > 1 and not self._on_wire(s, self.grad_wire):  # built-in step needs none)
                    s.grad_shard.div_(self.world)
                continue
            g = s.grad_shard if s.master.dtype == s.dtype else s.grad_shard.to(s.master.dtype)
            if not self._avg and self.world > 1 and not self._on_wire(s, self.grad_wire):  # (a wire divides inside)
                g = g / self.world
            s.master.grad = g
        if self._fused:  # one kernel per space: coefficient, update and the cast into param_shard
            total = self._sumsq_total() if self.max_grad_norm is not None else None
            self.grad_rounding_step += 1
            self.inner.step(self.spaces, total, self.max_grad_norm, self.param_wire)
            self._gather(cast=False)
            return
        if self.max_grad_norm is not None:
            self._clip()
        self.grad_rounding_step += 1
        self.inner.step()
        self._gather()

    def _sumsq_total(self) -> torch.Tensor:
        """The f64 sum of squares of this rank's gradient shards (their padding is zeros), summed over the ranks: one
        element on the device, the same bits on every rank. Sets ``grad_norm``."""
        from .. import ops

        total = ops.sumsq([s.grad_shard for s in self.spaces])
        self._fence(self.spaces[0])
        dist.all_reduce(total, op=dist.ReduceOp.SUM, group=self.group)
        self.grad_norm = total[0].sqrt().to(torch.float32)
        return total

    def _clip(self) -> None:
        """Clip by global norm (docs/collectives.md "Gradient clipping"): the total of :meth:`_sumsq_total`, then
        per space the cast to the master dtype with the coefficient on it. Everything stays on the device."""
        from .. import ops

        total = self._sumsq_total()
        for s in self.spaces:
            ops.clip_scale(s.grad_shard, total, self.max_grad_norm, out=s.master_grad)
            s.master.grad = s.master_grad

    @torch.no_grad()
    def _gather(self, cast: bool = True) -> None:
        """All-gather the parameter shards; ``cast``: fill them from the masters first (the built-in step's kernel
        has written them already, or with ``fused_param_wire`` the buckets' wires, which are gathered as they are)."""
        works = []
        for s in self.spaces:
            if cast:
                s.param_shard.copy_(s.master)
            for bi, b in enumerate(s.buckets):
                if self._on_wire(s, self.param_wire):
                    from .compressed import all_gather_compressed

                    ready = {} if cast or s.param_wires is None else {"input_wire": s.param_wires[bi]}
                    works.append(all_gather_compressed(s.flat[b.off:b.off + b.padded],
                                                       s.param_shard[b.soff:b.soff + b.shard], group=self.group,
                                                       wire=self.param_wire, async_op=True, **self._param_rot, **ready))
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
