"""Tensor-level access to the gfx950 kernels.

* :func:`reduce_nway` -- K1: ``out = op(srcs[0], ..., srcs[k-1])`` for 1..8
  same-shaped GPU tensors; ``op`` in sum/avg/prod/min/max (+ band/bor/bxor for
  integers). Floats include the OCP FP8 dtypes ``float8_e4m3fn`` / ``float8_e5m2``:
  like bf16 / f16 they are widened to fp32, folded in source order and rounded
  once (torch's CPU cast: nearest even, no saturation), with the gfx950 packed
  converts. Default implementation stages tiles through LDS with
  ``global_load_lds_dwordx4`` (LDS-DMA ring); ``impl="regs"`` is the
  register-staged variant kept for A/B measurement; a ``_nt`` suffix
  (``"lds_nt"``, ``"regs_nt"``) makes the destination stores non-temporal.
* :func:`multi_copy`, :func:`pack`, :func:`unpack` -- K2: one launch copies a
  whole list of tensors (the staging used by gather/scatter/all_gather with
  tensor lists, reference main.py:35-37,51-52,66-68).

* :func:`mx_quantize`, :func:`mx_reduce`, :func:`mx_dequantize` -- the block-scaled wire formats
  ``mxfp8_e4m3`` (docs/collectives.md "Compressed all-reduce": 32-element blocks, one E8M0 scale
  byte and 32 ``float8_e4m3fn`` bytes each), ``mxfp4_e2m1`` ("The ``mxfp4_e2m1`` wire format":
  16 bytes of two e2m1 nibbles instead) and ``mxfp6_e2m3`` ("The ``mxfp6_e2m3`` wire format": 24 bytes,
  a bit stream of 32 six-bit e2m3 codes), picked by the trailing keyword ``wire``.
  ``parallel/compressed.py`` builds ``all_reduce_compressed`` from them.
  :func:`mx_quantize`, :func:`mx_quantize_shards` and :func:`mx_reduce` take ``rounding="stochastic"`` with
  ``seed=`` and ``stream=``: unbiased, stateless rounding of the payload (docs/collectives.md "Stochastic
  rounding"), and ``residual=``: error feedback
  (docs/collectives.md "Error feedback"), an f32 tensor added before the quantization and left holding
  what it dropped, fused into the same kernel.
  :func:`mx_quantize`, :func:`mx_quantize_shards`, :func:`mx_dequantize`, :func:`mx_dequantize_shards` and
  :func:`mx_fold` take ``rotation="hadamard"`` with ``rotation_seed=``: a randomized Hadamard rotation of
  every 32-element block before the quantization and back after the dequantization (docs/collectives.md
  "Hadamard rotation"), inside the same kernels; :func:`mx_reduce` folds rotated wires as they are.
* :func:`mx_quantize_shards`, :func:`mx_dequantize_shards`, :func:`mx_fold` -- the same wire with one
  chunk per shard (docs/collectives.md "Compressed reduce-scatter and all-gather") and the fold of
  chunk wires straight into a tensor; ``reduce_scatter_compressed`` / ``all_gather_compressed``.
* :func:`mx_quantize_list`, :func:`mx_dequantize_list`, :func:`mx_list_numel` -- the same wire for a list of
  tensors, read and written where they are, every tensor starting a fresh block (docs/collectives.md
  "Tensor-list layout"); ``all_reduce_compressed`` of a list and ``GradBucketer(in_place=True)``.
* :func:`sumsq`, :func:`clip_scale` -- gradient clipping by global norm (docs/collectives.md "Gradient
  clipping"): a deterministic f64 sum of squares of a tensor list, and the cast that multiplies by the clip
  coefficient it computes on the device from that sum; ``ShardedOptimizer(max_grad_norm=...)``.
* :func:`adamw_step` -- one AdamW step on a shard in one pass: gradient, clip coefficient, f32 state and the
  parameter cast (docs/collectives.md "Fused AdamW step"); ``ShardedOptimizer(params, "adamw")``. With
  ``state_format="mxfp8_e4m3"`` the two moments are block-scaled 8-bit buffers (:func:`adamw_state_pack`,
  :func:`adamw_state_unpack`; docs/collectives.md "8-bit AdamW state").

Every function runs on the current HIP stream and raises if the native
extension is missing (no silent eager fallback). ``*_reference`` functions are
the plain-PyTorch fp32 references the tests compare against.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Sequence

import torch

_OPS = ("sum", "avg", "prod", "min", "max", "band", "bor", "bxor")


def _C():
    from .. import _load_native

    return _load_native()


# K1 variants (csrc/kernels/kernel_api.h K1Mode): the LDS-DMA pipeline, the register pipeline,
# the streaming kernel (one slab per workgroup, grid over the whole buffer); `_nt` =
# non-temporal stores, `_ntl` = non-temporal loads and stores
K1_IMPLS = {"lds": 1, "regs": 0, "lds_nt": 3, "regs_nt": 2, "lds_ntl": 11, "regs_ntl": 10, "stream": 4,
            "stream_nt": 6, "stream_ntl": 14}


def reduce_nway(srcs: Sequence[torch.Tensor], out: torch.Tensor | None = None, op: str = "sum",
                impl: str = "lds_ntl", max_blocks: int = 0) -> torch.Tensor:
    """K1 N-way element-wise reduction on the GPU (1 <= len(srcs) <= 8).

    Default: the LDS-DMA pipeline with non-temporal loads and stores (6.27 TB/s for 2 fp32
    sources of 256 MiB on MI355X vs 6.06 for ``torch.add``, profiles/r3/k1_sweep_ntl_r3.json);
    ``stream_ntl`` is the fastest variant there (6.48 TB/s)."""
    if op not in _OPS:
        raise ValueError(f"op must be one of {_OPS}, got {op!r}")
    if impl not in K1_IMPLS:
        raise ValueError(f"impl must be one of {sorted(K1_IMPLS)}, got {impl!r}")
    srcs = list(srcs)
    if not srcs:
        raise ValueError("reduce_nway needs at least one source")
    if out is None:
        out = torch.empty_like(srcs[0], memory_format=torch.contiguous_format)
    _C().reduce_nway(srcs, out, op, K1_IMPLS[impl], int(max_blocks))
    return out


def reduce_nway_reference(srcs: Sequence[torch.Tensor], op: str = "sum") -> torch.Tensor:
    """Plain-PyTorch reference of :func:`reduce_nway` (f32 accumulation for floats, FP8 included:
    one cast back at the end)."""
    srcs = list(srcs)
    dt = srcs[0].dtype
    fl = dt.is_floating_point
    acc = srcs[0].to(torch.float64 if dt == torch.float64 else torch.float32) if fl else srcs[0].clone()
    for s in srcs[1:]:
        s2 = s.to(acc.dtype)
        if op in ("sum", "avg"):
            acc = acc + s2 if dt != torch.bool else (acc | s2)
        elif op == "prod":
            acc = acc * s2 if dt != torch.bool else (acc & s2)
        elif op == "max":
            acc = torch.maximum(acc, s2)
        elif op == "min":
            acc = torch.minimum(acc, s2)
        elif op == "band":
            acc = acc & s2
        elif op == "bor":
            acc = acc | s2
        elif op == "bxor":
            acc = acc ^ s2
    if op == "avg":
        acc = acc / len(srcs) if fl else torch.div(acc, len(srcs), rounding_mode="trunc")
    return acc.to(dt)


def multi_copy(srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor], max_blocks: int = 0,
               depth: int = 0, ntl: bool | None = None) -> None:
    """K2: copy srcs[i] -> dsts[i] for every i in ONE kernel launch.

    ``max_blocks`` caps the grid and ``depth`` (4 or 8) sets the LDS-DMA ring
    depth; 0 keeps the tuned defaults (csrc/kernels/kernel_api.h kK2Grid/kK2Depth); ``ntl``
    forces non-temporal source loads on / off (None: by the list's shape, see k2_ntl in copy.hip)."""
    _C().multi_copy(list(srcs), list(dsts), max_blocks, depth, -1 if ntl is None else int(bool(ntl)))


def _byte_view(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(-1).view(torch.uint8)


def pack(tensors: Sequence[torch.Tensor], out: torch.Tensor | None = None) -> torch.Tensor:
    """Concatenate ``tensors`` (any dtypes) into one flat uint8 buffer with K2."""
    tensors = list(tensors)
    total = sum(t.numel() * t.element_size() for t in tensors)
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=tensors[0].device)
    dsts, off = [], 0
    for t in tensors:
        n = t.numel() * t.element_size()
        dsts.append(out[off:off + n])
        off += n
    multi_copy([_byte_view(t) for t in tensors], dsts)
    return out


def unpack(flat: torch.Tensor, tensors: Sequence[torch.Tensor]) -> None:
    """Inverse of :func:`pack`: scatter a flat uint8 buffer back into ``tensors``."""
    tensors = list(tensors)
    srcs, off = [], 0
    for t in tensors:
        n = t.numel() * t.element_size()
        srcs.append(flat[off:off + n])
        off += n
    multi_copy(srcs, [_byte_view(t) for t in tensors])


# ------------------------------------------ block-scaled wires (mxfp8_e4m3, mxfp4_e2m1, mxfp6_e2m3)
# Every function below takes the format as the trailing keyword ``wire``. Where the first argument is the
# wire tensor itself it is positional-only (``w``), so the keyword is free for the format's name.
MX_BLOCK = 32
MX_DTYPES = (torch.float32, torch.bfloat16, torch.float16)

class _MxFormat(NamedTuple):
    """What the Python side knows of a wire format (the kernels' table: MxFmt in csrc/kernels/mx_wire.hip)."""
    payload: int    # payload bytes per block; one scale byte follows
    mant: int       # mantissa bits of a code
    fmin: int       # f32 exponent field of the smallest normal magnitude
    bias: int       # the scale rule: e = k - bias for amax = m 2^k, 1 <= m < 2 ...
    switch: float   # ... and one more where frexp's mantissa m / 2 is above this
    emin: int       # lower and upper clamp of e
    emax: int
    sign: int       # the sign's bit in a code


_MX_FORMATS = {"mxfp8_e4m3": _MxFormat(32, 3, 121, 8, 0.875, -117, 120, 7),
               "mxfp4_e2m1": _MxFormat(16, 1, 127, 2, 0.75, -125, 126, 3),
               "mxfp6_e2m3": _MxFormat(24, 3, 127, 2, 0.9375, -123, 126, 5)}
MX_WIRES = tuple(_MX_FORMATS)


def _mx_format(wire, who: str) -> _MxFormat:
    """The table row of a wire format; ValueError for a name that is not one."""
    if not isinstance(wire, str) or wire not in _MX_FORMATS:
        raise ValueError(f"{who}: unknown wire format {wire!r} (supported: {', '.join(MX_WIRES)})")
    return _MX_FORMATS[wire]


def mx_chunk_blocks(numel: int, world: int = 1, *, wire: str = "mxfp8_e4m3") -> int:
    """Blocks per chunk when ``numel`` elements are dealt to ``world`` chunks (csrc/kernels/mx_layout.h):
    a multiple of 16, and of 4096 once a chunk's wire (33, 17 or 25 bytes per block) reaches 1 MiB."""
    bw = _mx_format(wire, "mx_chunk_blocks").payload + 1
    world = max(1, int(world))
    blocks = (int(numel) + MX_BLOCK - 1) // MX_BLOCK
    cb = max(16, ((blocks + world - 1) // world + 15) // 16 * 16)
    if bw * cb >= 1 << 20:
        cb = (cb + 4095) // 4096 * 4096
    return cb


def mx_wire_bytes(numel: int, world: int = 1, *, wire: str = "mxfp8_e4m3") -> int:
    """Bytes of the wire of ``numel`` elements in ``world`` chunks: ``world`` x (32 cb payload + cb scales);
    16 cb payload bytes for ``mxfp4_e2m1``, 24 cb for ``mxfp6_e2m3``."""
    return (_mx_format(wire, "mx_wire_bytes").payload + 1) * mx_chunk_blocks(numel, world, wire=wire) * max(1, int(world))


def mx_shard_blocks(m: int, *, wire: str = "mxfp8_e4m3") -> int:
    """Blocks per chunk of a shard wire of ``m``-element shards: ``mx_chunk_blocks(m, 1)``. Chunk ``r`` of
    such a wire holds shard ``r`` alone, its blocks counted from the shard's first element."""
    return mx_chunk_blocks(m, 1, wire=wire)


def mx_shard_wire_bytes(m: int, world: int = 1, *, wire: str = "mxfp8_e4m3") -> int:
    """Bytes of the shard wire of ``world`` shards of ``m`` elements."""
    return (_mx_format(wire, "mx_shard_wire_bytes").payload + 1) * mx_shard_blocks(m, wire=wire) * max(1, int(world))


def _mx_check_dtype(dt, who):
    if dt not in MX_DTYPES:
        raise TypeError(f"{who}: float32, bfloat16 or float16 tensors only, got {dt}")


def mx_owner_residual_numel(numel: int, world: int = 1, *, wire: str = "mxfp8_e4m3") -> int:
    """Elements of the owner residual of an all-reduce of ``numel`` elements over ``world`` ranks: one float
    per element of a rank's chunk, padding blocks included -- ``32 * mx_chunk_blocks(numel, world)``."""
    return MX_BLOCK * mx_chunk_blocks(numel, world, wire=wire)


def _mx_check_residual(residual, numel: int, device, who: str, name: str = "the residual", data: str = "data") -> None:
    """An error-feedback residual (docs/collectives.md "Error feedback") is updated in place, which rules
    out the copy the other arguments may go through: float32, ``numel`` elements, on ``device``,
    contiguous and 16-byte aligned. ``name``, ``data``: what the messages call it and what it belongs to."""
    if residual is None:
        return
    if not isinstance(residual, torch.Tensor) or residual.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be a float32 tensor, got "
                        f"{residual.dtype if isinstance(residual, torch.Tensor) else type(residual).__name__}")
    if residual.numel() != int(numel):
        raise ValueError(f"{who}: {name} has {residual.numel()} elements, {int(numel)} expected")
    if residual.device != device:
        raise ValueError(f"{who}: {name} is on {residual.device}, the {data} on {device}")
    if not residual.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")
    if residual.data_ptr() % 16:
        raise ValueError(f"{who}: {name} must be 16-byte aligned")


MX_ROUNDINGS = ("nearest", "stochastic")


def _mx_check_rounding(rounding, seed, stream, index_offset, numel, residual, who: str) -> bool:
    """The rounding arguments (docs/collectives.md "Stochastic rounding"); True for ``"stochastic"``. The seed,
    the stream and the offset are checked whatever the rounding is, so a wrong call fails the same way with both."""
    if not isinstance(rounding, str) or rounding not in MX_ROUNDINGS:
        raise ValueError(f"{who}: unknown rounding {rounding!r} (supported: {', '.join(MX_ROUNDINGS)})")
    for name, v, top in (("seed", seed, 1 << 64), ("stream", stream, 1 << 32), ("index_offset", index_offset, 1 << 64)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{who}: {name} must be an int, got {type(v).__name__}")
        if not 0 <= v < top:
            raise ValueError(f"{who}: {name} must be in [0, 2^{top.bit_length() - 1}), got {v}")
    if index_offset + int(numel) > 1 << 64:
        raise ValueError(f"{who}: index_offset + numel must not exceed 2^64")
    sr = rounding == "stochastic"
    if sr and residual is not None:
        raise ValueError(f"{who}: rounding='stochastic' and a residual are alternatives, not both")
    return sr


MX_ROTATIONS = ("hadamard",)
_MX_ROT_STREAM = 0x52484431  # the stream of the sign word ("RHD1"), no rank's stream


def _mx_check_rotation(rotation, rotation_seed, who: str) -> bool:
    """The rotation arguments (docs/collectives.md "Hadamard rotation"); True for a rotation. The seed is checked
    whatever the rotation is."""
    if rotation is not None and (not isinstance(rotation, str) or rotation not in MX_ROTATIONS):
        raise ValueError(f"{who}: unknown rotation {rotation!r} (supported: None, {', '.join(MX_ROTATIONS)})")
    if isinstance(rotation_seed, bool) or not isinstance(rotation_seed, int):
        raise TypeError(f"{who}: rotation_seed must be an int, got {type(rotation_seed).__name__}")
    if not 0 <= rotation_seed < 1 << 64:
        raise ValueError(f"{who}: rotation_seed must be in [0, 2^64), got {rotation_seed}")
    return rotation is not None


def _mx_quantizer_args(who: str, wire, residual, numel: int, device, rounding, seed, stream, index_offset=0,
                       rot=False, rotation_seed=0) -> tuple:
    """The options of a quantizer after the caller's look at the format and (``rot``: what ``_mx_check_rotation``
    returned) the rotation: the rounding, then the residual (of ``numel`` elements on ``device``). Returns the
    trailing arguments of the native call: ``(wire, residual, sr, seed, stream, index_offset, rot, rot_seed)``."""
    sr = _mx_check_rounding(rounding, seed, stream, index_offset, numel, residual, who)
    _mx_check_residual(residual, numel, device, who)
    return wire, None if residual is None else residual.detach(), sr, seed, stream, index_offset, rot, rotation_seed


def mx_rotation_signs(seed: int) -> int:
    """The 32-bit sign word of a rotation seed: bit ``j`` set flips the sign of position ``j`` of every
    32-element block (csrc/kernels/mx_rot.h): the word of index 0 under the key of ``(seed, 0x52484431)``."""
    _mx_check_rotation(None, seed, "mx_rotation_signs")
    return int(_mx_sr_mix(torch.tensor(mx_sr_key(seed, _MX_ROT_STREAM), dtype=torch.int64)))


def mx_quantize(x: torch.Tensor, world: int = 1, out: torch.Tensor | None = None, *,
                wire: str = "mxfp8_e4m3", residual: torch.Tensor | None = None, rounding: str = "nearest",
                seed: int = 0, stream: int = 0, index_offset: int = 0, rotation: str | None = None,
                rotation_seed: int = 0) -> torch.Tensor:
    """``x`` (GPU; f32 / bf16 / f16) -> its wire in the format ``wire``: a uint8 tensor of ``world`` chunks
    of ``[32 cb payload bytes][cb scale bytes]`` (``mxfp4_e2m1``: 16 cb payload bytes, two elements to a
    byte; ``mxfp6_e2m3``: 24 cb payload bytes, six bits to an element), padding blocks included (scale 127, payload 0).

    ``residual`` (float32, one element per element of ``x``; error feedback): what is quantized is
    ``x.float() + residual``, and the residual becomes what the quantization dropped of that sum (+0
    where that is not finite), in place and in the same launch. ``x`` is not modified.

    ``rounding="stochastic"`` (docs/collectives.md "Stochastic rounding"): every payload element is rounded up
    or down with the probability of its distance, by the counter-based word of ``(seed, stream,
    index_offset + its index in x)`` -- no state, the same arguments give the same bytes. Scale bytes and
    layout are unchanged. Not together with ``residual``.

    ``rotation="hadamard"`` (docs/collectives.md "Hadamard rotation"): every 32-element block, padding zeros
    included, is rotated with the sign word of ``rotation_seed`` before anything else happens to it, so the
    scale, the rounding and the residual all belong to the rotated block; :func:`mx_dequantize` and
    :func:`mx_fold` with the same two arguments rotate back. Wire layout and size are unchanged."""
    _mx_check_dtype(x.dtype, "mx_quantize")
    _mx_format(wire, "mx_quantize")
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_quantize")
    args = _mx_quantizer_args("mx_quantize", wire, residual, x.numel(), x.device, rounding, seed, stream, index_offset,
                              rot, rotation_seed)
    return _C().mx_quantize(x.detach().reshape(-1), int(world), out, *args)


def mx_reduce(w: torch.Tensor, /, nsrc: int, op: str = "sum", out: torch.Tensor | None = None, *,
              wire: str = "mxfp8_e4m3", residual: torch.Tensor | None = None, rounding: str = "nearest",
              seed: int = 0, stream: int = 0) -> torch.Tensor:
    """``nsrc`` (1..8) chunk wires ``w`` back to back -> one chunk wire: every source dequantized, folded
    in f32 in source order (``avg``: then divided by ``nsrc``), and quantized again.

    ``residual`` (float32, 32 elements per block of a chunk: the owner residual) is added to the fold
    before it is quantized again and becomes what that quantization dropped, in place.

    ``rounding="stochastic"``: the fold is quantized again by the words of ``(seed, stream, index in the
    chunk)``; a single finite source comes back as its own bytes. Not together with ``residual``."""
    if op not in ("sum", "avg"):
        raise ValueError(f"mx_reduce: op must be 'sum' or 'avg', got {op!r}")
    bw = _mx_format(wire, "mx_reduce").payload + 1
    n = 0 if residual is None else w.numel() // (bw * max(1, int(nsrc))) * MX_BLOCK  # the elements of a chunk
    args = _mx_quantizer_args("mx_reduce", wire, residual, n, w.device, rounding, seed, stream)
    return _C().mx_reduce(w, int(nsrc), op, out, *args[:5])  # (no index offset, no rotation: rotated wires fold as they are)


def mx_dequantize(w: torch.Tensor, /, numel: int, dtype: torch.dtype = torch.float32, world: int = 1,
                  out: torch.Tensor | None = None, *, wire: str = "mxfp8_e4m3", rotation: str | None = None,
                  rotation_seed: int = 0) -> torch.Tensor:
    """The first ``numel`` elements of a wire ``w`` of ``world`` chunks, rounded once to ``dtype``; written
    into ``out`` (``numel`` elements, any shape) when given -- exactly those elements and nothing else.
    ``rotation``, ``rotation_seed``: those of the :func:`mx_quantize` that made the wire; every dequantized
    block is rotated back before it is rounded."""
    _mx_format(wire, "mx_dequantize")
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_dequantize")
    if out is None:
        _mx_check_dtype(dtype, "mx_dequantize")
        out = torch.empty(int(numel), dtype=dtype, device=w.device)
    else:
        _mx_check_dtype(out.dtype, "mx_dequantize")
        if out.numel() != int(numel):
            raise ValueError(f"mx_dequantize: out has {out.numel()} elements, numel is {numel}")
    _C().mx_dequantize(w, int(world), out, wire, rot, rotation_seed)
    return out


def mx_list_numel(numels: Sequence[int]) -> int:
    """Elements of the virtual tensor of a tensor list (docs/collectives.md "Tensor-list layout"): every tensor
    starts a fresh block, so ``32 * sum(ceil(n_i / 32))``. The size of a list's residual."""
    return MX_BLOCK * sum((int(n) + MX_BLOCK - 1) // MX_BLOCK for n in numels)


def _mx_check_list(xs, who: str) -> list:
    """The tensors of a list call: a list or tuple of tensors of one MX dtype on one device, contiguous (they are
    read and written where they are, so none can go through a copy)."""
    if not isinstance(xs, (list, tuple)) or not all(isinstance(x, torch.Tensor) for x in xs):
        raise TypeError(f"{who}: a list or tuple of tensors expected")
    if not xs:
        raise ValueError(f"{who}: an empty list has no device and no dtype")
    if len(xs) > 65535:
        raise ValueError(f"{who}: at most 65535 tensors in a list, got {len(xs)}")
    _mx_check_dtype(xs[0].dtype, who)
    for x in xs:
        if x.dtype != xs[0].dtype:
            raise TypeError(f"{who}: the tensors of a list share one dtype, got {xs[0].dtype} and {x.dtype}")
        if x.device != xs[0].device:
            raise ValueError(f"{who}: the tensors of a list share one device, got {xs[0].device} and {x.device}")
        if not x.is_contiguous():
            raise ValueError(f"{who}: the tensors of a list must be contiguous")
    return [x.detach() for x in xs]


def mx_quantize_list(xs: Sequence[torch.Tensor], world: int = 1, out: torch.Tensor | None = None, *,
                     wire: str = "mxfp8_e4m3", residual: torch.Tensor | None = None, rounding: str = "nearest",
                     seed: int = 0, stream: int = 0, rotation: str | None = None,
                     rotation_seed: int = 0) -> torch.Tensor:
    """The tensors ``xs`` (GPU, one dtype, contiguous) -> the wire of their tensor-list layout (docs/collectives.md
    "Tensor-list layout"), read where they are: byte for byte ``mx_quantize`` of their concatenation with every
    tensor zero-padded to a multiple of 32 elements, so no block holds elements of two tensors. A tensor that is
    not 16-byte aligned is read element by element; the others move as vectors.

    ``residual``: float32, ``mx_list_numel`` elements, indexed by the position in that padded concatenation; the
    positions past a tensor's end are left as +0. ``rounding``, ``seed``, ``stream``: as in :func:`mx_quantize`,
    the word index of an element being its position in the padded concatenation. ``rotation``: as there."""
    xs = _mx_check_list(xs, "mx_quantize_list")
    _mx_format(wire, "mx_quantize_list")
    n = mx_list_numel([x.numel() for x in xs])
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_quantize_list")
    args = _mx_quantizer_args("mx_quantize_list", wire, residual, n, xs[0].device, rounding, seed, stream, 0, rot,
                              rotation_seed)
    return _C().mx_quantize_list(xs, int(world), out, *args[:5], *args[6:])  # (no index offset)


def mx_dequantize_list(w: torch.Tensor, /, outs: Sequence[torch.Tensor], world: int = 1, *,
                       wire: str = "mxfp8_e4m3", rotation: str | None = None, rotation_seed: int = 0) -> None:
    """The wire ``w`` of a tensor list in ``world`` chunks -> the tensors ``outs`` (GPU, one dtype, contiguous),
    written where they are: exactly their elements and nothing else. ``rotation``, ``rotation_seed``: those of
    the :func:`mx_quantize_list` that made the wire."""
    outs = _mx_check_list(outs, "mx_dequantize_list")
    _mx_format(wire, "mx_dequantize_list")
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_dequantize_list")
    _C().mx_dequantize_list(w, outs, int(world), wire, rot, rotation_seed)


def _mx_check_shards(numel: int, world: int, who: str) -> int:
    world = int(world)
    if world < 1 or numel < 1 or numel % world:
        raise ValueError(f"{who}: {numel} elements are not {world} shards of one or more elements")
    return numel // world


def mx_quantize_shards(x: torch.Tensor, world: int, out: torch.Tensor | None = None, *,
                       wire: str = "mxfp8_e4m3", residual: torch.Tensor | None = None, rounding: str = "nearest",
                       seed: int = 0, stream: int = 0, index_offset: int = 0, rotation: str | None = None,
                       rotation_seed: int = 0) -> torch.Tensor:
    """``x`` (GPU; ``world`` shards of ``m`` elements) -> its shard wire: chunk ``r`` is the wire of shard
    ``r`` alone (``mx_shard_blocks(m)`` blocks; what lies past the shard's end counts as +0).
    ``residual``: as in :func:`mx_quantize`, one float per element of ``x``. ``rounding``, ``seed``,
    ``stream``, ``index_offset``: as in :func:`mx_quantize` -- an element draws the word of its index in
    ``x``, so it is rounded the same way in both layouts. ``rotation``, ``rotation_seed``: as in
    :func:`mx_quantize`, on the blocks counted from each shard's first element."""
    _mx_check_dtype(x.dtype, "mx_quantize_shards")
    _mx_format(wire, "mx_quantize_shards")
    _mx_check_shards(x.numel(), world, "mx_quantize_shards")
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_quantize_shards")
    args = _mx_quantizer_args("mx_quantize_shards", wire, residual, x.numel(), x.device, rounding, seed, stream,
                              index_offset, rot, rotation_seed)
    return _C().mx_quantize_shards(x.detach().reshape(-1), int(world), out, *args)


def mx_dequantize_shards(w: torch.Tensor, /, shard_numel: int, dtype: torch.dtype = torch.float32, world: int = 1,
                         out: torch.Tensor | None = None, *, wire: str = "mxfp8_e4m3", rotation: str | None = None,
                         rotation_seed: int = 0) -> torch.Tensor:
    """A shard wire ``w`` of ``world`` chunks -> ``world * shard_numel`` elements: chunk ``r`` fills
    ``out[r * m:(r + 1) * m]``, rounded once to the dtype; nothing outside ``out`` is written.
    ``rotation``, ``rotation_seed``: as in :func:`mx_dequantize`."""
    _mx_format(wire, "mx_dequantize_shards")
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_dequantize_shards")
    n = int(shard_numel) * int(world)
    if out is None:
        _mx_check_dtype(dtype, "mx_dequantize_shards")
        out = torch.empty(n, dtype=dtype, device=w.device)
    else:
        _mx_check_dtype(out.dtype, "mx_dequantize_shards")
        if out.numel() != n:
            raise ValueError(f"mx_dequantize_shards: out has {out.numel()} elements, {world} shards of "
                             f"{shard_numel} are {n}")
    _mx_check_shards(n, world, "mx_dequantize_shards")
    _C().mx_dequantize_shards(w, int(world), out, wire, rot, rotation_seed)
    return out


def mx_fold(w: torch.Tensor, /, nsrc: int, numel: int, dtype: torch.dtype = torch.float32, op: str = "sum",
            out: torch.Tensor | None = None, *, wire: str = "mxfp8_e4m3", rotation: str | None = None,
            rotation_seed: int = 0) -> torch.Tensor:
    """``nsrc`` (1..8) chunk wires ``w`` of ``mx_shard_blocks(numel)`` blocks back to back -> ``numel``
    elements: every source dequantized, folded in f32 in source order (``avg``: then divided by ``nsrc``)
    and rounded once to the dtype -- :func:`mx_reduce` then :func:`mx_dequantize` without the
    requantization between. ``rotation``, ``rotation_seed``: those of the sources' quantization; the fold
    runs on the rotated values (the rotation is linear) and is rotated back once, after the ``avg`` division
    and before the rounding."""
    if op not in ("sum", "avg"):
        raise ValueError(f"mx_fold: op must be 'sum' or 'avg', got {op!r}")
    _mx_format(wire, "mx_fold")
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_fold")
    if out is None:
        _mx_check_dtype(dtype, "mx_fold")
        out = torch.empty(int(numel), dtype=dtype, device=w.device)
    else:
        _mx_check_dtype(out.dtype, "mx_fold")
        if out.numel() != int(numel):
            raise ValueError(f"mx_fold: out has {out.numel()} elements, numel is {numel}")
    _C().mx_fold(w, int(nsrc), op, out, wire, rot, rotation_seed)
    return out


def _mx_exp2(e: torch.Tensor) -> torch.Tensor:
    """2^e as f32 for integer -126 <= e <= 127, built from the exponent field (exact)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def _mx_block_scale(xb: torch.Tensor, fmt: _MxFormat):
    """The scale rule of every format's Q on (blocks, 32) f32: ``(e, special, zero)`` -- the exponent of a
    block's scale, and which blocks hold an inf or a NaN or are all zero (their payload is written as zeros)."""
    amax = xb.abs().amax(dim=1)
    special = ~torch.isfinite(xb).all(dim=1)
    zero = (amax == 0) & ~special
    # amax = m 2^k with 1 <= m < 2: frexp returns m / 2 and k + 1 (for a subnormal amax the true
    # exponent, below -126 either way: the clamp decides)
    m, ex = torch.frexp(torch.where(special | zero, torch.ones_like(amax), amax))
    e = ((ex.to(torch.int64) - 1) - fmt.bias + (m > fmt.switch).to(torch.int64)).clamp(fmt.emin, fmt.emax)
    e[zero] = 0
    return e, special, zero


def _mx_scale_bytes(e: torch.Tensor, special: torch.Tensor) -> torch.Tensor:
    s = (e + 127).to(torch.uint8)
    s[special] = 255
    return s


def _mx_quantize_blocks(xb: torch.Tensor):
    """(blocks, 32) f32 -> ((blocks, 32) uint8 payload, (blocks,) uint8 scales), the FP8 contract's Q."""
    e, special, zero = _mx_block_scale(xb, _MX_FORMATS["mxfp8_e4m3"])
    q = (xb * _mx_exp2(-e)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).clone()
    q[special | zero] = 0
    return q, _mx_scale_bytes(e, special)


def _mx_scale_values(s: torch.Tensor) -> torch.Tensor:
    """(blocks,) scale bytes -> f32 2^(s - 127), NaN for 255."""
    si = s.to(torch.int32)
    scale = torch.where(si == 0, torch.full_like(si, 0x00400000), si << 23).view(torch.float32).clone()
    scale[si == 255] = float("nan")
    return scale


def _mx_dequantize_blocks(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """The FP8 contract's D: (blocks, 32) payload bytes and (blocks,) scale bytes -> (blocks, 32) f32."""
    return q.view(torch.float8_e4m3fn).to(torch.float32) * _mx_scale_values(s)[:, None]


_MX4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # magnitudes of the e2m1 codes 0..7


def _mx4_quantize_blocks(xb: torch.Tensor):
    """(blocks, 32) f32 -> ((blocks, 16) uint8 payload, (blocks,) uint8 scales), the FP4 contract's Q."""
    e, special, zero = _mx_block_scale(xb, _MX_FORMATS["mxfp4_e2m1"])
    a = (xb * _mx_exp2(-e)[:, None]).abs()  # exact, or far below 0.25 where the product is subnormal
    # nearest code, ties to the even one: a midpoint belongs to the even neighbour
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8)
            + (a >= 1.75).to(torch.uint8) + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8)
            + (a > 5.0).to(torch.uint8))
    code = code | (torch.signbit(xb).to(torch.uint8) << 3)
    code[special | zero] = 0
    return (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous(), _mx_scale_bytes(e, special)


def _mx4_dequantize_blocks(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """The FP4 contract's D: (blocks, 16) payload bytes and (blocks,) scale bytes -> (blocks, 32) f32."""
    code = torch.stack([q & 15, q >> 4], dim=2).reshape(q.shape[0], 32).to(torch.int64)
    v = torch.tensor(_MX4_VALUES, dtype=torch.float32)[code & 7]
    v = torch.where((code & 8) != 0, -v, v)
    return v * _mx_scale_values(s)[:, None]  # 6 2^126 -> inf: one f32 product


def _mx6_pack(code: torch.Tensor) -> torch.Tensor:
    """(blocks, 32) six-bit codes -> (blocks, 24) payload bytes: the code of element j in bits 6j .. 6j + 5 of
    the block's little-endian bit stream, so four codes fill three bytes."""
    c = code.to(torch.int32).view(code.shape[0], 8, 4)
    k = c[:, :, 0] | (c[:, :, 1] << 6) | (c[:, :, 2] << 12) | (c[:, :, 3] << 18)
    return torch.stack([k & 255, (k >> 8) & 255, k >> 16], dim=2).reshape(code.shape[0], 24).to(torch.uint8)


def _mx6_unpack(q: torch.Tensor) -> torch.Tensor:
    """(blocks, 24) payload bytes -> (blocks, 32) six-bit codes (int32)."""
    b = q.to(torch.int32).view(q.shape[0], 8, 3)
    k = b[:, :, 0] | (b[:, :, 1] << 8) | (b[:, :, 2] << 16)
    return torch.stack([k & 63, (k >> 6) & 63, (k >> 12) & 63, (k >> 18) & 63], dim=2).reshape(q.shape[0], 32)


def _mx6_quantize_blocks(xb: torch.Tensor):
    """(blocks, 32) f32 -> ((blocks, 24) uint8 payload, (blocks,) uint8 scales), the FP6 contract's Q."""
    e, special, zero = _mx_block_scale(xb, _MX_FORMATS["mxfp6_e2m3"])
    # e2m3 is e4m3 with the exponent field cut to two bits: for |s| <= 7.5 the float8_e4m3fn byte of s / 64
    # (nearest even; both products exact, or far below half a grid step where they are subnormal) has bits 5
    # and 6 clear, and the code is its low five bits with its sign in bit 5
    b = ((xb * _mx_exp2(-e)[:, None]) * 0.015625).to(torch.float8_e4m3fn).view(torch.uint8).to(torch.int32)
    code = (b & 31) | ((b >> 7) << 5)
    code[special | zero] = 0
    return _mx6_pack(code), _mx_scale_bytes(e, special)


def _mx6_dequantize_blocks(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """The FP6 contract's D: (blocks, 24) payload bytes and (blocks,) scale bytes -> (blocks, 32) f32."""
    code = _mx6_unpack(q)
    mant, ex = (code & 7).to(torch.float32), (code >> 3) & 3
    v = torch.where(ex == 0, mant / 8, (1 + mant / 8) * _mx_exp2(torch.clamp(ex - 1, min=0)))
    v = torch.where((code & 32) != 0, -v, v)
    return v * _mx_scale_values(s)[:, None]  # 4 2^126 and above -> inf: one f32 product


# ---- stochastic rounding (docs/collectives.md "Stochastic rounding"), integer arithmetic on int64 tensors
_M32 = 0xFFFFFFFF


def _mx_sr_mul(x: torch.Tensor, c: int) -> torch.Tensor:
    """x * c mod 2^32 for 0 <= x < 2^32, without leaving int64."""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & _M32


def _mx_sr_mix(x: torch.Tensor) -> torch.Tensor:
    x = x ^ (x >> 16)
    x = _mx_sr_mul(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mx_sr_mul(x, 0x846CA68B)
    return x ^ (x >> 16)


def mx_sr_key(seed: int, stream: int = 0) -> int:
    """The 32-bit key of a stochastic call from its 64-bit seed and its 32-bit stream."""
    def mix(v):
        return int(_mx_sr_mix(torch.tensor(v & _M32, dtype=torch.int64)))
    return mix(mix(mix((seed & _M32) ^ 0x9E3779B9) + (seed >> 32)) + stream)


def _mx_sr_words(key: int, first: int, count: int) -> torch.Tensor:
    """The words of the element indices first .. first + count - 1 (below 2^64), as int64 in [0, 2^32)."""
    l = (first & _M32) + torch.arange(count, dtype=torch.int64)
    h = (first >> 32) + (l >> 32)
    kh = torch.where(h == 0, torch.full_like(h, key), _mx_sr_mix((key + h) & _M32))
    return _mx_sr_mix((l & _M32) ^ kh)


def _mx_sr_quantize_blocks(xb: torch.Tensor, u: torch.Tensor, fmt: _MxFormat):
    """(blocks, 32) f32 and (blocks, 32) words -> (payload, scale bytes): the contract's Q with the payload
    rounded stochastically. The scale is the nearest path's; the code of |s| is that of the grid point below
    it plus one where u < T, T = floor(t 2^32), read off the f32 bits of s."""
    mb, fmin, pb = fmt.mant, fmt.fmin, fmt.payload
    e, special, zero = _mx_block_scale(xb, fmt)
    bits = (xb * _mx_exp2(-e)[:, None]).view(torch.int32).to(torch.int64) & _M32  # one f32 product
    a = bits & 0x7FFFFFFF
    field, mant = a >> 23, (a & 0x7FFFFF) | 0x800000
    normal = field >= fmin
    sh = 23 - mb + (fmin - field).clamp(0, 40)
    lo = torch.where(normal, (field - fmin) << mb, torch.zeros_like(a)) + (mant >> sh)
    thr = ((mant & ((torch.ones_like(sh) << sh) - 1)) << 32) >> sh
    code = (lo + (u < thr).to(torch.int64)) | ((bits >> 31) << fmt.sign)
    code[special | zero] = 0
    code = code.to(torch.uint8)
    q = code if pb == 32 else (_mx6_pack(code) if pb == 24 else (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous())
    return q, _mx_scale_bytes(e, special)


# ---- Hadamard rotation (docs/collectives.md "Hadamard rotation"): f32 tensor operations in the defined order
def _mx_rot_flip(b: torch.Tensor, signs: int) -> torch.Tensor:
    """(blocks, 32) f32 with the sign of position j flipped where bit j of ``signs`` is set."""
    bits = (signs >> torch.arange(MX_BLOCK, dtype=torch.int64)) & 1
    mask = (bits * -0x80000000).to(torch.int32)  # 0x80000000 as an int32
    return (b.contiguous().view(torch.int32) ^ mask).view(torch.float32)


def _mx_rot_butterfly(b: torch.Tensor) -> torch.Tensor:
    """The product with the unnormalized Sylvester-Hadamard matrix, stage by stage: h = 1, 2, 4, 8, 16, and
    (y_j, y_{j+h}) <- (y_j + y_{j+h}, y_j - y_{j+h}) for every j with (j & h) == 0; one f32 operation each."""
    for h in (1, 2, 4, 8, 16):
        y = b.reshape(-1, MX_BLOCK // (2 * h), 2, h)
        lo, hi = y[:, :, 0, :], y[:, :, 1, :]
        b = torch.stack([lo + hi, lo - hi], dim=2).reshape(-1, MX_BLOCK)
    return b


def _mx_rot_forward(xb: torch.Tensor, signs: int) -> torch.Tensor:
    """R x of (blocks, 32) f32: the signs, then the butterfly."""
    return _mx_rot_butterfly(_mx_rot_flip(xb, signs))


def _mx_rot_inverse(db: torch.Tensor, signs: int) -> torch.Tensor:
    """R^-1 d of (blocks, 32) f32: the butterfly, one multiply by 2^-5, then the signs."""
    return _mx_rot_flip(_mx_rot_butterfly(db) * torch.tensor(0.03125, dtype=torch.float32), signs)


def _mx_blocks_fns(wire: str, who: str):
    """(table row, Q, D) of a format."""
    fmt = _mx_format(wire, who)
    return {32: (fmt, _mx_quantize_blocks, _mx_dequantize_blocks), 16: (fmt, _mx4_quantize_blocks, _mx4_dequantize_blocks),
            24: (fmt, _mx6_quantize_blocks, _mx6_dequantize_blocks)}[fmt.payload]


def _mx_split(w: torch.Tensor, nchunks: int, pb: int = 32):
    """Wire of ``nchunks`` chunks -> ((nchunks * cb, pb) payload, (nchunks * cb,) scales)."""
    if w.dtype != torch.uint8 or w.dim() != 1 or w.numel() % ((pb + 1) * 16 * nchunks):
        raise ValueError(f"not a wire of {nchunks} chunks: {w.dtype}, {tuple(w.shape)}")
    cb = w.numel() // ((pb + 1) * nchunks)
    w = w.view(nchunks, (pb + 1) * cb)
    return w[:, :pb * cb].reshape(nchunks * cb, pb), w[:, pb * cb:].reshape(nchunks * cb)


def _mx_join(q: torch.Tensor, s: torch.Tensor, nchunks: int) -> torch.Tensor:
    cb = s.numel() // nchunks
    return torch.cat([q.reshape(nchunks, q.shape[1] * cb), s.reshape(nchunks, cb)], dim=1).reshape(-1).contiguous()


def _mx_feed_back(v: torch.Tensor, d: torch.Tensor, residual: torch.Tensor) -> None:
    """The contract's residual update: ``residual <- v - d`` where that is finite, +0 elsewhere."""
    r = v - d
    residual.detach().view(-1).copy_(torch.where(torch.isfinite(r), r, torch.zeros_like(r)))


def mx_quantize_reference(x: torch.Tensor, world: int = 1, *, wire: str = "mxfp8_e4m3",
                          residual: torch.Tensor | None = None, rounding: str = "nearest", seed: int = 0,
                          stream: int = 0, index_offset: int = 0, rotation: str | None = None,
                          rotation_seed: int = 0) -> torch.Tensor:
    """Plain-PyTorch :func:`mx_quantize` on a CPU tensor, bit for bit the documented contract (with
    ``residual``: the contract of "Error feedback", the residual updated in place; with
    ``rounding="stochastic"``: the contract of "Stochastic rounding"; with ``rotation``: the contract of
    "Hadamard rotation", every block rotated before any of that)."""
    _mx_check_dtype(x.dtype, "mx_quantize_reference")
    fmt, Q, D = _mx_blocks_fns(wire, "mx_quantize_reference")
    world = max(1, int(world))
    flat = x.detach().reshape(-1).to(torch.float32)
    n = flat.numel()
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_quantize_reference")
    sr = _mx_check_rounding(rounding, seed, stream, index_offset, n, residual, "mx_quantize_reference")
    total = mx_chunk_blocks(n, world, wire=wire) * world
    xb = torch.zeros(total * MX_BLOCK, dtype=torch.float32)
    xb[:n] = flat
    if rot:  # the padding zeros of a partial block take part
        xb = _mx_rot_forward(xb.view(total, MX_BLOCK), mx_rotation_signs(rotation_seed)).reshape(-1)
    if sr:
        u = _mx_sr_words(mx_sr_key(seed, stream), index_offset, total * MX_BLOCK)
        return _mx_join(*_mx_sr_quantize_blocks(xb.view(total, MX_BLOCK), u.view(total, MX_BLOCK), fmt), world)
    if residual is not None:  # (one float per element of x: what lies past the end counts as +0 and is dropped)
        _mx_check_residual(residual, n, x.device, "mx_quantize_reference")
        rb = torch.zeros_like(xb)
        rb[:n] = residual.detach().view(-1)
        xb = xb + rb
    q, s = Q(xb.view(total, MX_BLOCK))
    if residual is not None:
        _mx_feed_back(xb[:n], D(q, s).reshape(-1)[:n], residual)
    return _mx_join(q, s, world)


def mx_reduce_reference(w: torch.Tensor, /, nsrc: int, op: str = "sum", *, wire: str = "mxfp8_e4m3",
                        residual: torch.Tensor | None = None, rounding: str = "nearest", seed: int = 0,
                        stream: int = 0) -> torch.Tensor:
    """Plain-PyTorch :func:`mx_reduce` on a CPU wire (``residual``: updated in place; ``rounding``, ``seed``,
    ``stream``: as in :func:`mx_reduce`)."""
    if op not in ("sum", "avg"):
        raise ValueError(f"mx_reduce_reference: op must be 'sum' or 'avg', got {op!r}")
    fmt, Q, D = _mx_blocks_fns(wire, "mx_reduce_reference")
    q, s = _mx_split(w, nsrc, fmt.payload)
    cb = s.numel() // nsrc
    d = D(q, s).view(nsrc, cb, MX_BLOCK)
    acc = d[0].clone()
    for r in range(1, nsrc):
        acc = acc + d[r]
    if op == "avg":
        acc = acc / torch.tensor(float(nsrc), dtype=torch.float32)
    if _mx_check_rounding(rounding, seed, stream, 0, 0, residual, "mx_reduce_reference"):
        u = _mx_sr_words(mx_sr_key(seed, stream), 0, cb * MX_BLOCK).view(cb, MX_BLOCK)
        return _mx_join(*_mx_sr_quantize_blocks(acc, u, fmt), 1)
    if residual is None:
        return _mx_join(*Q(acc), 1)
    _mx_check_residual(residual, cb * MX_BLOCK, w.device, "mx_reduce_reference")
    acc = acc + residual.detach().view(cb, MX_BLOCK)
    q, s = Q(acc)
    _mx_feed_back(acc.reshape(-1), D(q, s).reshape(-1), residual)
    return _mx_join(q, s, 1)


def mx_dequantize_reference(w: torch.Tensor, /, numel: int, dtype: torch.dtype = torch.float32,
                            world: int = 1, *, wire: str = "mxfp8_e4m3", rotation: str | None = None,
                            rotation_seed: int = 0) -> torch.Tensor:
    """Plain-PyTorch :func:`mx_dequantize` on a CPU wire."""
    _mx_check_dtype(dtype, "mx_dequantize_reference")
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_dequantize_reference")
    fmt, _, D = _mx_blocks_fns(wire, "mx_dequantize_reference")
    world = max(1, int(world))
    if w.numel() != mx_wire_bytes(numel, world, wire=wire):
        raise ValueError(f"the wire of {numel} elements in {world} chunks has "
                         f"{mx_wire_bytes(numel, world, wire=wire)} bytes, got {w.numel()}")
    q, s = _mx_split(w, world, fmt.payload)
    d = D(q, s)
    if rot:
        d = _mx_rot_inverse(d, mx_rotation_signs(rotation_seed))
    return d.reshape(-1)[:int(numel)].to(dtype)


def _mx_list_pad(n: int) -> int:
    return -int(n) % MX_BLOCK


def mx_quantize_list_reference(xs: Sequence[torch.Tensor], world: int = 1, *, wire: str = "mxfp8_e4m3",
                               residual: torch.Tensor | None = None, rounding: str = "nearest", seed: int = 0,
                               stream: int = 0, rotation: str | None = None, rotation_seed: int = 0) -> torch.Tensor:
    """Plain-PyTorch :func:`mx_quantize_list` on CPU tensors: :func:`mx_quantize_reference` of the concatenation
    of the tensors, each zero-padded to a multiple of 32 elements. ``residual`` is updated in place; its
    positions past a tensor's end are left as +0."""
    xs = _mx_check_list(xs, "mx_quantize_list_reference")
    flat = torch.cat([torch.nn.functional.pad(x.reshape(-1), (0, _mx_list_pad(x.numel()))) for x in xs])
    w = mx_quantize_reference(flat, world, wire=wire, residual=residual, rounding=rounding, seed=seed, stream=stream,
                              rotation=rotation, rotation_seed=rotation_seed)
    if residual is not None:
        at, r = 0, residual.detach().view(-1)
        for x in xs:
            at += x.numel() + _mx_list_pad(x.numel())
            r[at - _mx_list_pad(x.numel()):at] = 0.0
    return w


def mx_dequantize_list_reference(w: torch.Tensor, /, outs: Sequence[torch.Tensor], world: int = 1, *,
                                 wire: str = "mxfp8_e4m3", rotation: str | None = None, rotation_seed: int = 0) -> None:
    """Plain-PyTorch :func:`mx_dequantize_list` on a CPU wire: :func:`mx_dequantize_reference` of the padded
    concatenation, split into ``outs``."""
    outs = _mx_check_list(outs, "mx_dequantize_list_reference")
    d = mx_dequantize_reference(w, mx_list_numel([o.numel() for o in outs]), outs[0].dtype, world, wire=wire,
                                rotation=rotation, rotation_seed=rotation_seed)
    at = 0
    for o in outs:
        o.copy_(d[at:at + o.numel()].view_as(o))
        at += o.numel() + _mx_list_pad(o.numel())


def mx_quantize_shards_reference(x: torch.Tensor, world: int, *, wire: str = "mxfp8_e4m3",
                                 residual: torch.Tensor | None = None, rounding: str = "nearest", seed: int = 0,
                                 stream: int = 0, index_offset: int = 0, rotation: str | None = None,
                                 rotation_seed: int = 0) -> torch.Tensor:
    """Plain-PyTorch :func:`mx_quantize_shards` on a CPU tensor (``residual``: updated in place; ``rounding``,
    ``seed``, ``stream``, ``index_offset``, ``rotation``, ``rotation_seed``: as in :func:`mx_quantize_shards`)."""
    _mx_check_dtype(x.dtype, "mx_quantize_shards_reference")
    _mx_format(wire, "mx_quantize_shards_reference")
    m = _mx_check_shards(x.numel(), world, "mx_quantize_shards_reference")
    flat = x.detach().reshape(-1)
    _mx_check_rotation(rotation, rotation_seed, "mx_quantize_shards_reference")
    rot = {"rotation": rotation, "rotation_seed": rotation_seed}
    if _mx_check_rounding(rounding, seed, stream, index_offset, flat.numel(), residual,
                          "mx_quantize_shards_reference"):
        return torch.cat([mx_quantize_reference(flat[r * m:(r + 1) * m], 1, wire=wire, rounding=rounding, seed=seed,
                                                stream=stream, index_offset=index_offset + r * m, **rot)
                          for r in range(int(world))])
    if residual is None:
        return torch.cat([mx_quantize_reference(flat[r * m:(r + 1) * m], 1, wire=wire, **rot)
                          for r in range(int(world))])
    _mx_check_residual(residual, flat.numel(), x.device, "mx_quantize_shards_reference")
    out = []
    for r in range(int(world)):  # (a shard's slice of the residual need not be aligned: it goes through a copy)
        part = residual.detach().view(-1)[r * m:(r + 1) * m].clone()
        out.append(mx_quantize_reference(flat[r * m:(r + 1) * m], 1, wire=wire, residual=part, **rot))
        residual.detach().view(-1)[r * m:(r + 1) * m] = part
    return torch.cat(out)


def mx_dequantize_shards_reference(w: torch.Tensor, /, shard_numel: int, dtype: torch.dtype = torch.float32,
                                   world: int = 1, *, wire: str = "mxfp8_e4m3", rotation: str | None = None,
                                   rotation_seed: int = 0) -> torch.Tensor:
    """Plain-PyTorch :func:`mx_dequantize_shards` on a CPU wire."""
    _mx_check_dtype(dtype, "mx_dequantize_shards_reference")
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_dequantize_shards_reference")
    fmt, _, D = _mx_blocks_fns(wire, "mx_dequantize_shards_reference")
    m, world = int(shard_numel), int(world)
    _mx_check_shards(m * world, world, "mx_dequantize_shards_reference")
    if w.numel() != mx_shard_wire_bytes(m, world, wire=wire):
        raise ValueError(f"the wire of {world} shards of {m} elements has "
                         f"{mx_shard_wire_bytes(m, world, wire=wire)} bytes, got {w.numel()}")
    q, s = _mx_split(w, world, fmt.payload)
    d = D(q, s)
    if rot:
        d = _mx_rot_inverse(d, mx_rotation_signs(rotation_seed))
    return d.reshape(world, -1)[:, :m].reshape(-1).to(dtype)


def mx_fold_reference(w: torch.Tensor, /, nsrc: int, numel: int, dtype: torch.dtype = torch.float32,
                      op: str = "sum", *, wire: str = "mxfp8_e4m3", rotation: str | None = None,
                      rotation_seed: int = 0) -> torch.Tensor:
    """Plain-PyTorch :func:`mx_fold` on a CPU wire."""
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_fold_reference")
    if op not in ("sum", "avg"):
        raise ValueError(f"mx_fold_reference: op must be 'sum' or 'avg', got {op!r}")
    _mx_check_dtype(dtype, "mx_fold_reference")
    fmt, _, D = _mx_blocks_fns(wire, "mx_fold_reference")
    nsrc, numel = int(nsrc), int(numel)
    if numel < 1 or w.numel() != mx_shard_wire_bytes(numel, nsrc, wire=wire):
        raise ValueError(f"{nsrc} chunk wires of {numel} elements have "
                         f"{mx_shard_wire_bytes(numel, nsrc, wire=wire)} bytes, got {w.numel()}")
    q, s = _mx_split(w, nsrc, fmt.payload)
    d = D(q, s).view(nsrc, -1)
    acc = d[0].clone()
    for r in range(1, nsrc):
        acc = acc + d[r]
    if op == "avg":
        acc = acc / torch.tensor(float(nsrc), dtype=torch.float32)
    if rot:
        acc = _mx_rot_inverse(acc.view(-1, MX_BLOCK), mx_rotation_signs(rotation_seed)).reshape(-1)
    return acc[:numel].to(dtype)


# ------------------------------------------ gradient clipping (docs/collectives.md "Gradient clipping")
CLIP_DTYPES = MX_DTYPES
SUMSQ_TILE = 8192  # elements of a stage-1 tile (csrc/kernels/kernel_api.h kSumsqTile)
SUMSQ_CHAIN = 38   # L: f32 roundings between an element and its tile's f64 partial, at most (kSumsqChain)


def _clip_check_list(tensors, who: str) -> list:
    if not isinstance(tensors, (list, tuple)) or not all(isinstance(t, torch.Tensor) for t in tensors):
        raise TypeError(f"{who}: a list or tuple of tensors expected")
    if not tensors:
        raise ValueError(f"{who}: an empty list has no device")
    for t in tensors:
        if t.dtype not in CLIP_DTYPES:
            raise ValueError(f"{who}: float32, bfloat16 or float16 tensors only, got {t.dtype}")
        if t.device != tensors[0].device:
            raise ValueError(f"{who}: the tensors share one device, got {tensors[0].device} and {t.device}")
    return [t.detach() for t in tensors]


def _clip_check_total(t, device, who: str, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.numel() != 1 or t.device != device:
        raise ValueError(f"{who}: {what} must be one float64 element on {device}")


def sumsq_reference(tensors: Sequence[torch.Tensor]) -> torch.Tensor:
    """Plain-PyTorch :func:`sumsq`: the f64 sum of the squares of the values as stored, shape ``[1]``."""
    xs = _clip_check_list(tensors, "sumsq_reference")
    total = torch.zeros(1, dtype=torch.float64, device=xs[0].device)
    for x in xs:
        total += x.double().square().sum()
    return total


def sumsq(tensors: Sequence[torch.Tensor], out: torch.Tensor | None = None, *, max_blocks: int = 0) -> torch.Tensor:
    """The sum of the squares of every element of ``tensors`` (f32 / bf16 / f16, mixed freely, empty ones allowed)
    as one float64 element of shape ``[1]`` on their device, left there: nothing synchronises with the host.

    On the GPU (contiguous tensors, any alignment) two plain launches per call and one more per further tensor:
    fixed 8192-element tiles counted from each tensor's element 0, a fixed tree inside a tile, one f64 partial per
    tile, and one workgroup that folds the partials in a fixed order -- so the result is the same bits for any grid
    (``max_blocks`` caps the tile kernel's) and any base alignment, and within ``(SUMSQ_CHAIN + 1) 2^-24`` of the
    exact sum, relatively (docs/collectives.md "Gradient clipping"). inf and NaN propagate. CPU tensors:
    :func:`sumsq_reference`."""
    xs = _clip_check_list(tensors, "sumsq")
    if out is not None:
        _clip_check_total(out, xs[0].device, "sumsq", "out")
    if xs[0].device.type == "cpu":
        total = sumsq_reference(xs)
        return total if out is None else out.copy_(total.view_as(out))
    if not all(x.is_contiguous() for x in xs):
        raise ValueError("sumsq: the tensors must be contiguous")
    return _C().sumsq(xs, out, int(max_blocks))


def _clip_check_scale(src, total, max_norm, out, who: str) -> torch.Tensor:
    if not isinstance(src, torch.Tensor) or src.dtype not in CLIP_DTYPES:
        raise ValueError(f"{who}: src must be a float32, bfloat16 or float16 tensor")
    _clip_check_total(total, src.device, who, "total")
    float(max_norm)
    if out is None:
        return torch.empty(src.shape, dtype=torch.float32, device=src.device)
    if out.dtype not in (torch.float32, src.dtype) or out.numel() != src.numel() or out.device != src.device:
        raise ValueError(f"{who}: out must hold {src.numel()} float32 or {src.dtype} elements on {src.device}")
    return out


def _clip_coef(total: torch.Tensor, max_norm: float) -> torch.Tensor:
    """The coefficient as a 0-d f32 tensor on ``total``'s device: f32 operations from the f64 total on."""
    norm = total.detach().reshape(()).sqrt().to(torch.float32)
    c = torch.tensor(float(max_norm), dtype=torch.float32, device=total.device) / (norm + 1e-6)
    return torch.clamp(c, max=1.0)  # (a NaN stays a NaN)


def clip_scale_reference(src: torch.Tensor, total: torch.Tensor, max_norm: float,
                         out: torch.Tensor | None = None) -> torch.Tensor:
    """Plain-PyTorch :func:`clip_scale`: the coefficient of ``torch.nn.utils.clip_grad_norm_`` in f32 from the f64
    ``total``, one f32 product per element, one rounding to ``out``'s dtype."""
    out = _clip_check_scale(src, total, max_norm, out, "clip_scale_reference")
    return out.copy_((src.detach().to(torch.float32) * _clip_coef(total, max_norm)).view_as(out))


def clip_scale(src: torch.Tensor, total: torch.Tensor, max_norm: float, out: torch.Tensor | None = None) -> torch.Tensor:
    """``out[i] = round_once(float(src[i]) * coef)`` with ``coef = min(1, max_norm / (float(sqrt(total)) + 1e-6))``
    evaluated in f32 from the float64 one-element tensor ``total`` (:func:`sumsq`) where it lives: on the GPU the
    kernel reads it, the host never does. ``out`` is float32 (the default: a new tensor) or of ``src``'s dtype, and
    may then be ``src`` itself. With ``coef == 1`` the result is bit for bit the plain cast. A NaN total gives NaN
    everywhere, an infinite one coefficient 0 (finite elements 0, infinite ones NaN) --
    ``clip_grad_norm_(error_if_nonfinite=False)``. CPU tensors: :func:`clip_scale_reference`."""
    out = _clip_check_scale(src, total, max_norm, out, "clip_scale")
    if src.device.type == "cpu":
        return clip_scale_reference(src, total, max_norm, out)
    if not (src.is_contiguous() and out.is_contiguous()):
        raise ValueError("clip_scale: src and out must be contiguous")
    _C().clip_scale(src.detach(), total.detach(), float(max_norm), out)
    return out


# ------------------------------------------ fused AdamW step (docs/collectives.md "Fused AdamW step")
ADAMW_SPAN = 4096  # elements a workgroup takes per trip of its grid-stride loop (kernel_api.h kAdamWSpan)
ADAMW_STATE_FORMATS = ("mxfp8_e4m3",)  # state_format= of adamw_step (docs/collectives.md "8-bit AdamW state")


def _adamw_scalars(lr, betas, eps, weight_decay, step) -> tuple:
    """The eight scalars of one step as Python floats (f64), in kern::AdamWArgs' order: b1, 1 - b1, b2, 1 - b2,
    1 - lr wd, lr / (1 - b1^step), 1 / sqrt(1 - b2^step), eps. The kernel's binding and the reference round each
    to f32 once."""
    lr, (b1, b2), eps, wd, step = float(lr), (float(b) for b in betas), float(eps), float(weight_decay), int(step)
    if step < 1 or not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"adamw_step: step >= 1 and betas in [0, 1) expected, got step {step}, betas ({b1}, {b2})")
    return (b1, 1.0 - b1, b2, 1.0 - b2, 1.0 - lr * wd, lr / (1.0 - b1 ** step), 1.0 / math.sqrt(1.0 - b2 ** step), eps)


def _adamw_state_format(state_format, who: str) -> bool:
    """Whether the state is packed; ``None``: the f32 state."""
    if state_format is not None and state_format not in ADAMW_STATE_FORMATS:
        raise ValueError(f"{who}: unknown state_format {state_format!r} (supported: None, "
                         f"{', '.join(map(repr, ADAMW_STATE_FORMATS))})")
    return state_format is not None


def _adamw_check_wire(grad, param_out, wire_out, wire, wire_dtype, who: str):
    """The parameter-wire keywords of :func:`adamw_step`; returns the dtype the master is rounded to, ``None`` without
    ``wire_out`` (``wire`` is then ignored)."""
    if wire_out is None:
        return None
    _mx_format(wire, who)
    nb = mx_wire_bytes(grad.numel(), 1, wire=wire)
    if not isinstance(wire_out, torch.Tensor) or wire_out.dtype != torch.uint8 or wire_out.numel() != nb \
            or wire_out.device != grad.device or not wire_out.is_contiguous() or wire_out.data_ptr() % 16:
        raise ValueError(f"{who}: wire_out must be a contiguous, 16-byte aligned uint8 tensor of {nb} bytes on {grad.device}")
    if wire_dtype is None and param_out is None:
        raise ValueError(f"{who}: wire_out without param_out needs wire_dtype")
    dt = param_out.dtype if wire_dtype is None else wire_dtype
    if dt not in (torch.float32, grad.dtype) or (param_out is not None and param_out.dtype != dt):
        raise ValueError(f"{who}: wire_dtype must be float32 or {grad.dtype}, and param_out's dtype when both are given, "
                         f"got {wire_dtype}")
    return dt


def _adamw_check(grad, master, exp_avg, exp_avg_sq, param_out, total, max_norm, who: str, packed: bool = False,
                 state_offset=None) -> None:
    if not isinstance(grad, torch.Tensor) or grad.dtype not in CLIP_DTYPES:
        raise ValueError(f"{who}: grad must be a float32, bfloat16 or float16 tensor")
    if state_offset is not None:
        if not packed:
            raise ValueError(f"{who}: state_offset comes with state_format only")
        nb = exp_avg.numel() if isinstance(exp_avg, torch.Tensor) else 0
        if isinstance(state_offset, bool) or not isinstance(state_offset, int) or state_offset < 0 or state_offset % MX_BLOCK \
                or grad.numel() % MX_BLOCK or nb % (MX_BLOCK + 1) or state_offset + grad.numel() > nb // (MX_BLOCK + 1) * MX_BLOCK:
            raise ValueError(f"{who}: state_offset ({state_offset!r}) and numel ({grad.numel()}) must be multiples of "
                             f"{MX_BLOCK} inside the state's {nb // (MX_BLOCK + 1) * MX_BLOCK} elements")
    for name, t in (("master", master), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if packed and name != "master":
            nb = mx_wire_bytes(grad.numel(), 1) if state_offset is None else exp_avg.numel()
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.numel() != nb or t.device != grad.device \
                    or not t.is_contiguous() or t.data_ptr() % 16:
                raise ValueError(f"{who}: with state_format {name} must be a contiguous, 16-byte aligned uint8 wire of "
                                 f"{nb} bytes on {grad.device}")
        elif not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != grad.numel() \
                or t.device != grad.device:
            raise ValueError(f"{who}: {name} must hold {grad.numel()} float32 elements on {grad.device}")
    if param_out is not None and (param_out.dtype not in (torch.float32, grad.dtype)
                                  or param_out.numel() != grad.numel() or param_out.device != grad.device):
        raise ValueError(f"{who}: param_out must hold {grad.numel()} float32 or {grad.dtype} elements on {grad.device}")
    if (total is None) != (max_norm is None):
        raise ValueError(f"{who}: total and max_norm come together or not at all")
    if total is not None:
        _clip_check_total(total, grad.device, who, "total")
        float(max_norm)


def _adamw_pack_one(x: torch.Tensor, never_zero: bool) -> torch.Tensor:
    """n f32 elements -> their dealt ``mxfp8_e4m3`` wire of one chunk, on ``x``'s device. ``never_zero``: the rule
    of the stored square root, a positive value's scaled product is raised to 2^-9 (the smallest e4m3 subnormal)."""
    cb = mx_chunk_blocks(x.numel(), 1)
    xb = torch.zeros(cb * MX_BLOCK, dtype=torch.float32, device=x.device)
    xb[:x.numel()] = x.detach().reshape(-1)
    xb = xb.view(cb, MX_BLOCK)
    if not never_zero:
        return _mx_join(*_mx_quantize_blocks(xb), 1)
    e, special, zero = _mx_block_scale(xb, _MX_FORMATS["mxfp8_e4m3"])
    t = xb * _mx_exp2(-e)[:, None]
    t = torch.where((xb > 0) & (t < 2.0 ** -9), torch.full_like(t, 2.0 ** -9), t)
    q = t.to(torch.float8_e4m3fn).view(torch.uint8).clone()
    q[special | zero] = 0
    return _mx_join(q, _mx_scale_bytes(e, special), 1)


def adamw_state_pack(exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor) -> tuple:
    """The f32 moments of a shard -> the two uint8 buffers of ``state_format="mxfp8_e4m3"`` (docs/collectives.md
    "8-bit AdamW state"): ``exp_avg`` as ``mx_quantize_reference(exp_avg, 1)`` has it, ``exp_avg_sq`` as the wire of
    its f32 square root in which a positive root is never stored as code 0. Plain torch on any device."""
    for t in (exp_avg, exp_avg_sq):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != exp_avg.numel():
            raise ValueError("adamw_state_pack: two float32 tensors of one size expected")
    return _adamw_pack_one(exp_avg, False), _adamw_pack_one(exp_avg_sq.detach().sqrt(), True)


def adamw_state_unpack(exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, numel: int) -> tuple:
    """The two uint8 buffers of :func:`adamw_state_pack` -> ``(m, v)`` in f32, ``v = s * s`` (one rounding) from the
    stored root ``s``. Plain torch on any device."""
    out = []
    for w in (exp_avg, exp_avg_sq):
        if w.numel() != mx_wire_bytes(numel, 1):
            raise ValueError(f"adamw_state_unpack: the state of {numel} elements has {mx_wire_bytes(numel, 1)} bytes, "
                             f"got {w.numel()}")
        out.append(_mx_dequantize_blocks(*_mx_split(w.detach(), 1)).reshape(-1)[:int(numel)])
    return out[0], out[1] * out[1]


def adamw_step_reference(grad: torch.Tensor, master: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, *,
                         lr: float, betas, eps: float, weight_decay: float, step: int,
                         param_out: torch.Tensor | None = None, total: torch.Tensor | None = None,
                         max_norm: float | None = None, state_format: str | None = None,
                         wire_out: torch.Tensor | None = None, wire: str = "mxfp8_e4m3",
                         wire_dtype: torch.dtype | None = None, state_offset: int | None = None) -> None:
    """Plain-PyTorch :func:`adamw_step`: the same sequence, one f32 operation per rounding, the scalars of the same
    function rounded to f32 once. With ``state_format`` the state is unpacked, stepped and packed again (with
    ``state_offset``: the span's blocks of it). ``wire_out`` receives
    ``mx_quantize_reference(p.to(wire_dtype), 1, wire=wire)`` of the new master ``p``."""
    who = "adamw_step_reference"
    packed = _adamw_state_format(state_format, who)
    _adamw_check(grad, master, exp_avg, exp_avg_sq, param_out, total, max_norm, who, packed, state_offset)
    wire_dtype = _adamw_check_wire(grad, param_out, wire_out, wire, wire_dtype, who)
    b1, omb1, b2, omb2, decay, step_size, inv_sqrt_bc2, e = (
        torch.tensor(x, dtype=torch.float32, device=grad.device) for x in _adamw_scalars(lr, betas, eps, weight_decay, step))
    g = grad.detach().to(torch.float32).reshape(-1)
    if total is not None:
        g = g * _clip_coef(total, max_norm)
    if state_offset is not None:  # the span's payload rows and scale bytes inside the two buffers
        spans = [_adamw_span(t, state_offset, g.numel()) for t in (exp_avg, exp_avg_sq)]
        m0, s0 = (_mx_dequantize_blocks(q, s).reshape(-1) for q, s in spans)
        v0 = s0 * s0
    else:
        m0, v0 = (adamw_state_unpack(exp_avg, exp_avg_sq, g.numel()) if packed
                  else (exp_avg.detach().reshape(-1), exp_avg_sq.detach().reshape(-1)))
    m = b1 * m0 + omb1 * g
    v = b2 * v0 + omb2 * (g * g)
    p = master.detach().reshape(-1) * decay
    s = v.sqrt()
    p = p - step_size * (m / (s * inv_sqrt_bc2 + e))
    if packed:
        m, v = _adamw_pack_one(m, False), _adamw_pack_one(s, True)
    if state_offset is not None:
        for (q, sc), new in zip(spans, (m, v)):
            nq, ns = _mx_split(new, 1)
            q.copy_(nq[:q.shape[0]]), sc.copy_(ns[:q.shape[0]])
        m = v = None
    for dst, src in ((exp_avg, m), (exp_avg_sq, v), (master, p)) + (() if param_out is None else ((param_out, p),)):
        if src is not None:
            dst.detach().copy_(src.view_as(dst))
    if wire_out is not None:
        wire_out.detach().copy_(mx_quantize_reference(p.to(wire_dtype), 1, wire=wire))


def _adamw_span(buf: torch.Tensor, state_offset: int, numel: int) -> tuple:
    """Views of the payload rows ``[blocks, 32]`` and the scale bytes of the span ``[state_offset, state_offset +
    numel)`` inside a packed state buffer of ``buf.numel() / 33`` blocks."""
    cb, b0, nb = buf.numel() // (MX_BLOCK + 1), state_offset // MX_BLOCK, numel // MX_BLOCK
    flat = buf.detach().view(-1)
    return flat[MX_BLOCK * b0:MX_BLOCK * (b0 + nb)].view(nb, MX_BLOCK), flat[MX_BLOCK * cb + b0:MX_BLOCK * cb + b0 + nb]


def adamw_step(grad: torch.Tensor, master: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, *,
               lr: float, betas, eps: float, weight_decay: float, step: int, param_out: torch.Tensor | None = None,
               total: torch.Tensor | None = None, max_norm: float | None = None, max_blocks: int = 0,
               state_format: str | None = None, wire_out: torch.Tensor | None = None, wire: str = "mxfp8_e4m3",
               wire_dtype: torch.dtype | None = None, state_offset: int | None = None) -> None:
    """One AdamW step (decoupled weight decay, torch's formula) on the float32 ``master``, ``exp_avg`` and
    ``exp_avg_sq`` in place, from a float32 / bfloat16 / float16 ``grad`` read once; ``step`` counts from 1.

    Per element, in f32 without contraction (docs/collectives.md "Fused AdamW step")::

        g = float(grad) * coef
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * (g * g)
        p = p * (1 - lr * wd)
        p = p - lr / (1 - b1^step) * (m / (sqrt(v) / sqrt(1 - b2^step) + eps))

    ``coef`` is 1, or with ``total`` (the float64 one-element sum of squares of :func:`sumsq`) and ``max_norm`` the
    coefficient of :func:`clip_scale`, evaluated on the device. ``param_out`` (float32 or ``grad``'s dtype) receives
    the new master rounded once. NaN and inf propagate as the arithmetic gives them. On the GPU this is one kernel
    and one pass (contiguous tensors, any alignment, no overlap between the five buffers; ``max_blocks`` caps the
    grid); CPU tensors: :func:`adamw_step_reference`.

    ``state_format="mxfp8_e4m3"`` (default ``None``: the f32 state above, the same kernels as ever): ``exp_avg`` and
    ``exp_avg_sq`` are the 16-byte aligned uint8 buffers of :func:`adamw_state_pack`, ``mx_wire_bytes(numel, 1)``
    bytes each, the second one holding ``sqrt(exp_avg_sq)``. The kernel dequantizes them (``v = s * s``), runs the
    sequence above, gives ``master`` and ``param_out`` the unquantized ``m`` and ``sqrt(v)`` of this step, and
    requantizes both moments in place in the same pass (docs/collectives.md "8-bit AdamW state").

    ``wire_out`` (default ``None``; docs/collectives.md "Parameter wire from the step"): a contiguous, 16-byte aligned
    uint8 tensor of ``mx_wire_bytes(numel, 1, wire=wire)`` bytes that the same kernel fills with the wire of the new
    master rounded once to ``wire_dtype`` -- byte for byte ``mx_quantize(p.to(wire_dtype), 1, wire=wire)``, blank tail
    blocks included -- so the parameter all-gather needs no quantizer. ``wire`` is any of ``MX_WIRES`` and ignored
    without ``wire_out``. ``wire_dtype`` is float32 or ``grad``'s dtype; it defaults to ``param_out.dtype``, is
    required when ``param_out`` is ``None`` and must agree with it when both are given. On the GPU every f32 side
    must then be 16-byte and every 16-bit side 8-byte aligned (``ValueError`` otherwise); ``numel`` is arbitrary.

    ``state_offset`` (with ``state_format`` only): ``grad``, ``master``, ``param_out`` and ``wire_out`` hold the
    elements ``[state_offset, state_offset + numel)`` of the shard whose packed state ``exp_avg`` / ``exp_avg_sq``
    are; the state buffers are then whole chunks of ``cb = bytes / 33`` blocks, ``state_offset`` and ``numel`` are
    multiples of 32 and ``state_offset + numel <= 32 cb``. Only the span's payload and scale bytes are touched."""
    packed = _adamw_state_format(state_format, "adamw_step")
    _adamw_check(grad, master, exp_avg, exp_avg_sq, param_out, total, max_norm, "adamw_step", packed, state_offset)
    wire_dtype = _adamw_check_wire(grad, param_out, wire_out, wire, wire_dtype, "adamw_step")
    if grad.device.type == "cpu":
        return adamw_step_reference(grad, master, exp_avg, exp_avg_sq, lr=lr, betas=betas, eps=eps,
                                    weight_decay=weight_decay, step=step, param_out=param_out, total=total,
                                    max_norm=max_norm, state_format=state_format, wire_out=wire_out, wire=wire,
                                    wire_dtype=wire_dtype, state_offset=state_offset)
    if not all(t.is_contiguous() for t in (grad, master, exp_avg, exp_avg_sq) + (() if param_out is None else (param_out,))):
        raise ValueError("adamw_step: the tensors must be contiguous")
    fn = _C().adamw8_step if packed else _C().adamw_step
    new = () if wire_out is None and state_offset is None else (
        (None if wire_out is None else wire_out.detach(), wire, "" if wire_dtype is None else str(wire_dtype)[6:])
        + ((state_offset,) if packed else ()))
    fn(grad.detach(), master.detach(), exp_avg.detach(), exp_avg_sq.detach(),
       list(_adamw_scalars(lr, betas, eps, weight_decay, step)),
       None if param_out is None else param_out.detach(), None if total is None else total.detach(),
       0.0 if max_norm is None else float(max_norm), int(max_blocks), *new)


__all__ = ["reduce_nway", "reduce_nway_reference", "multi_copy", "pack", "unpack",
           "sumsq", "clip_scale", "sumsq_reference", "clip_scale_reference",
           "adamw_step", "adamw_step_reference", "ADAMW_STATE_FORMATS", "adamw_state_pack", "adamw_state_unpack",
           "MX_WIRES", "MX_ROUNDINGS", "MX_ROTATIONS", "mx_sr_key", "mx_rotation_signs",
           "mx_quantize", "mx_reduce", "mx_dequantize", "mx_chunk_blocks", "mx_wire_bytes",
           "mx_owner_residual_numel",
           "mx_quantize_reference", "mx_reduce_reference", "mx_dequantize_reference",
           "mx_shard_blocks", "mx_shard_wire_bytes", "mx_quantize_shards", "mx_dequantize_shards", "mx_fold",
           "mx_quantize_shards_reference", "mx_dequantize_shards_reference", "mx_fold_reference"]
