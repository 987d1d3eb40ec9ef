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

Every function runs on the current HIP stream and raises if the native
extension is missing (no silent eager fallback). ``*_reference`` functions are
the plain-PyTorch fp32 references the tests compare against.
"""
from __future__ import annotations

from typing import Sequence

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
MX_WIRES = ("mxfp8_e4m3", "mxfp4_e2m1", "mxfp6_e2m3")
_MX_PAYLOAD = {"mxfp8_e4m3": 32, "mxfp4_e2m1": 16, "mxfp6_e2m3": 24}  # payload bytes per block; one scale byte follows


def _mx_payload(wire, who: str) -> int:
    """Payload bytes per block of a wire format; ValueError for a name that is not one."""
    if not isinstance(wire, str) or wire not in _MX_PAYLOAD:
        raise ValueError(f"{who}: unknown wire format {wire!r} (supported: {', '.join(MX_WIRES)})")
    return _MX_PAYLOAD[wire]


def mx_chunk_blocks(numel: int, world: int = 1, *, wire: str = "mxfp8_e4m3") -> int:
    """Blocks per chunk when ``numel`` elements are dealt to ``world`` chunks (csrc/kernels/mx_layout.h):
    a multiple of 16, and of 4096 once a chunk's wire (33, 17 or 25 bytes per block) reaches 1 MiB."""
    bw = _mx_payload(wire, "mx_chunk_blocks") + 1
    world = max(1, int(world))
    blocks = (int(numel) + MX_BLOCK - 1) // MX_BLOCK
    cb = max(16, ((blocks + world - 1) // world + 15) // 16 * 16)
    if bw * cb >= 1 << 20:
        cb = (cb + 4095) // 4096 * 4096
    return cb


def mx_wire_bytes(numel: int, world: int = 1, *, wire: str = "mxfp8_e4m3") -> int:
    """Bytes of the wire of ``numel`` elements in ``world`` chunks: ``world`` x (32 cb payload + cb scales);
    16 cb payload bytes for ``mxfp4_e2m1``, 24 cb for ``mxfp6_e2m3``."""
    return (_mx_payload(wire, "mx_wire_bytes") + 1) * mx_chunk_blocks(numel, world, wire=wire) * max(1, int(world))


def mx_shard_blocks(m: int, *, wire: str = "mxfp8_e4m3") -> int:
    """Blocks per chunk of a shard wire of ``m``-element shards: ``mx_chunk_blocks(m, 1)``. Chunk ``r`` of
    such a wire holds shard ``r`` alone, its blocks counted from the shard's first element."""
    return mx_chunk_blocks(m, 1, wire=wire)


def mx_shard_wire_bytes(m: int, world: int = 1, *, wire: str = "mxfp8_e4m3") -> int:
    """Bytes of the shard wire of ``world`` shards of ``m`` elements."""
    return (_mx_payload(wire, "mx_shard_wire_bytes") + 1) * mx_shard_blocks(m, wire=wire) * max(1, int(world))


def _mx_check_dtype(dt, who):
    if dt not in MX_DTYPES:
        raise TypeError(f"{who}: float32, bfloat16 or float16 tensors only, got {dt}")


def mx_owner_residual_numel(numel: int, world: int = 1, *, wire: str = "mxfp8_e4m3") -> int:
    """Elements of the owner residual of an all-reduce of ``numel`` elements over ``world`` ranks: one float
    per element of a rank's chunk, padding blocks included -- ``32 * mx_chunk_blocks(numel, world)``."""
    return MX_BLOCK * mx_chunk_blocks(numel, world, wire=wire)


def _mx_check_residual(residual, numel: int, device, who: str) -> None:
    """An error-feedback residual (docs/collectives.md "Error feedback") is updated in place, which rules
    out the copy the other arguments may go through: float32, ``numel`` elements, on ``device``,
    contiguous and 16-byte aligned."""
    if residual is None:
        return
    if not isinstance(residual, torch.Tensor) or residual.dtype != torch.float32:
        raise TypeError(f"{who}: the residual must be a float32 tensor, got "
                        f"{residual.dtype if isinstance(residual, torch.Tensor) else type(residual).__name__}")
    if residual.numel() != int(numel):
        raise ValueError(f"{who}: the residual has {residual.numel()} elements, {int(numel)} expected")
    if residual.device != device:
        raise ValueError(f"{who}: the residual is on {residual.device}, the data on {device}")
    if not residual.is_contiguous():
        raise ValueError(f"{who}: the residual must be contiguous")
    if residual.data_ptr() % 16:
        raise ValueError(f"{who}: the residual must be 16-byte aligned")


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


def _mx_check_rotation(rotation, rotation_seed, who: str) -> dict:
    """The rotation arguments (docs/collectives.md "Hadamard rotation") -> the keywords of the native call: none
    without a rotation, so that call is what it was. The seed is checked whatever the rotation is."""
    if rotation is not None and (not isinstance(rotation, str) or rotation not in MX_ROTATIONS):
        raise ValueError(f"{who}: unknown rotation {rotation!r} (supported: None, {', '.join(MX_ROTATIONS)})")
    if isinstance(rotation_seed, bool) or not isinstance(rotation_seed, int):
        raise TypeError(f"{who}: rotation_seed must be an int, got {type(rotation_seed).__name__}")
    if not 0 <= rotation_seed < 1 << 64:
        raise ValueError(f"{who}: rotation_seed must be in [0, 2^64), got {rotation_seed}")
    return {} if rotation is None else {"rot": True, "rot_seed": rotation_seed}


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
    _mx_payload(wire, "mx_quantize")
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_quantize")
    if _mx_check_rounding(rounding, seed, stream, index_offset, x.numel(), residual, "mx_quantize"):
        return _C().mx_quantize(x.detach().reshape(-1), int(world), out, wire, None, True, seed, stream, index_offset,
                                **rot)
    if residual is None:
        return _C().mx_quantize(x.detach().reshape(-1), int(world), out, wire, **rot)
    _mx_check_residual(residual, x.numel(), x.device, "mx_quantize")
    return _C().mx_quantize(x.detach().reshape(-1), int(world), out, wire, residual.detach(), **rot)


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
    pb = _mx_payload(wire, "mx_reduce")
    if _mx_check_rounding(rounding, seed, stream, 0, 0, residual, "mx_reduce"):
        return _C().mx_reduce(w, int(nsrc), op, out, wire, None, True, seed, stream)
    if residual is None:
        return _C().mx_reduce(w, int(nsrc), op, out, wire)
    _mx_check_residual(residual, w.numel() // ((pb + 1) * max(1, int(nsrc))) * MX_BLOCK, w.device, "mx_reduce")
    return _C().mx_reduce(w, int(nsrc), op, out, wire, residual.detach())


def mx_dequantize(w: torch.Tensor, /, numel: int, dtype: torch.dtype = torch.float32, world: int = 1,
                  out: torch.Tensor | None = None, *, wire: str = "mxfp8_e4m3", rotation: str | None = None,
                  rotation_seed: int = 0) -> torch.Tensor:
    """The first ``numel`` elements of a wire ``w`` of ``world`` chunks, rounded once to ``dtype``; written
    into ``out`` (``numel`` elements, any shape) when given -- exactly those elements and nothing else.
    ``rotation``, ``rotation_seed``: those of the :func:`mx_quantize` that made the wire; every dequantized
    block is rotated back before it is rounded."""
    _mx_payload(wire, "mx_dequantize")
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_dequantize")
    if out is None:
        _mx_check_dtype(dtype, "mx_dequantize")
        out = torch.empty(int(numel), dtype=dtype, device=w.device)
    else:
        _mx_check_dtype(out.dtype, "mx_dequantize")
        if out.numel() != int(numel):
            raise ValueError(f"mx_dequantize: out has {out.numel()} elements, numel is {numel}")
    _C().mx_dequantize(w, int(world), out, wire, **rot)
    return out


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
    _mx_payload(wire, "mx_quantize_shards")
    _mx_check_shards(x.numel(), world, "mx_quantize_shards")
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_quantize_shards")
    if _mx_check_rounding(rounding, seed, stream, index_offset, x.numel(), residual, "mx_quantize_shards"):
        return _C().mx_quantize_shards(x.detach().reshape(-1), int(world), out, wire, None, True, seed, stream,
                                       index_offset, **rot)
    if residual is None:
        return _C().mx_quantize_shards(x.detach().reshape(-1), int(world), out, wire, **rot)
    _mx_check_residual(residual, x.numel(), x.device, "mx_quantize_shards")
    return _C().mx_quantize_shards(x.detach().reshape(-1), int(world), out, wire, residual.detach(), **rot)


def mx_dequantize_shards(w: torch.Tensor, /, shard_numel: int, dtype: torch.dtype = torch.float32, world: int = 1,
                         out: torch.Tensor | None = None, *, wire: str = "mxfp8_e4m3", rotation: str | None = None,
                         rotation_seed: int = 0) -> torch.Tensor:
    """A shard wire ``w`` of ``world`` chunks -> ``world * shard_numel`` elements: chunk ``r`` fills
    ``out[r * m:(r + 1) * m]``, rounded once to the dtype; nothing outside ``out`` is written.
    ``rotation``, ``rotation_seed``: as in :func:`mx_dequantize`."""
    _mx_payload(wire, "mx_dequantize_shards")
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
    _C().mx_dequantize_shards(w, int(world), out, wire, **rot)
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
    _mx_payload(wire, "mx_fold")
    rot = _mx_check_rotation(rotation, rotation_seed, "mx_fold")
    if out is None:
        _mx_check_dtype(dtype, "mx_fold")
        out = torch.empty(int(numel), dtype=dtype, device=w.device)
    else:
        _mx_check_dtype(out.dtype, "mx_fold")
        if out.numel() != int(numel):
            raise ValueError(f"mx_fold: out has {out.numel()} elements, numel is {numel}")
    _C().mx_fold(w, int(nsrc), op, out, wire, **rot)
    return out


def _mx_exp2(e: torch.Tensor) -> torch.Tensor:
    """2^e as f32 for integer -126 <= e <= 127, built from the exponent field (exact)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def _mx_quantize_blocks(xb: torch.Tensor):
    """(blocks, 32) f32 -> ((blocks, 32) uint8 payload, (blocks,) uint8 scales), the FP8 contract's Q."""
    amax = xb.abs().amax(dim=1)
    special = ~torch.isfinite(xb).all(dim=1)
    zero = (amax == 0) & ~special
    # amax = m 2^k with 1 <= m < 2: frexp returns m / 2 and k + 1 (for a subnormal amax the true
    # exponent, below -126 either way: the clamp decides)
    m, ex = torch.frexp(torch.where(special | zero, torch.ones_like(amax), amax))
    e = (ex.to(torch.int64) - 1) - 8 + (m > 0.875).to(torch.int64)
    e = e.clamp(-117, 120)
    e[zero] = 0
    q = (xb * _mx_exp2(-e)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).clone()
    q[special | zero] = 0
    s = (e + 127).to(torch.uint8)
    s[special] = 255
    return q, s


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
    amax = xb.abs().amax(dim=1)
    special = ~torch.isfinite(xb).all(dim=1)
    zero = (amax == 0) & ~special
    m, ex = torch.frexp(torch.where(special | zero, torch.ones_like(amax), amax))
    e = (ex.to(torch.int64) - 1) - 2 + (m > 0.75).to(torch.int64)  # m here is half the contract's m
    e = e.clamp(-125, 126)
    e[zero] = 0
    a = (xb * _mx_exp2(-e)[:, None]).abs()  # exact, or far below 0.25 where the product is subnormal
    # nearest code, ties to the even one: a midpoint belongs to the even neighbour
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8)
            + (a >= 1.75).to(torch.uint8) + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8)
            + (a > 5.0).to(torch.uint8))
    code = code | (torch.signbit(xb).to(torch.uint8) << 3)
    code[special | zero] = 0
    q = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    s = (e + 127).to(torch.uint8)
    s[special] = 255
    return q, s


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
    amax = xb.abs().amax(dim=1)
    special = ~torch.isfinite(xb).all(dim=1)
    zero = (amax == 0) & ~special
    m, ex = torch.frexp(torch.where(special | zero, torch.ones_like(amax), amax))
    e = (ex.to(torch.int64) - 1) - 2 + (m > 0.9375).to(torch.int64)  # m here is half the contract's m
    e = e.clamp(-123, 126)
    e[zero] = 0
    # e2m3 is e4m3 with the exponent field cut to two bits: for |s| <= 7.5 the float8_e4m3fn byte of s / 64
    # (nearest even; both products exact, or far below half a grid step where they are subnormal) has bits 5
    # and 6 clear, and the code is its low five bits with its sign in bit 5
    b = ((xb * _mx_exp2(-e)[:, None]) * 0.015625).to(torch.float8_e4m3fn).view(torch.uint8).to(torch.int32)
    code = (b & 31) | ((b >> 7) << 5)
    code[special | zero] = 0
    s = (e + 127).to(torch.uint8)
    s[special] = 255
    return _mx6_pack(code), s


def _mx6_dequantize_blocks(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """The FP6 contract's D: (blocks, 24) payload bytes and (blocks,) scale bytes -> (blocks, 32) f32."""
    code = _mx6_unpack(q)
    mant, ex = (code & 7).to(torch.float32), (code >> 3) & 3
    v = torch.where(ex == 0, mant / 8, (1 + mant / 8) * _mx_exp2(torch.clamp(ex - 1, min=0)))
    v = torch.where((code & 32) != 0, -v, v)
    return v * _mx_scale_values(s)[:, None]  # 4 2^126 and above -> inf: one f32 product


# ---- stochastic rounding (docs/collectives.md "Stochastic rounding"), integer arithmetic on int64 tensors
_M32 = 0xFFFFFFFF
# per payload size: mantissa bits, f32 exponent field of the smallest normal magnitude, the scale rule's
# (exponent bias, switch point of frexp's mantissa, lower and upper clamp of e)
_MX_SR_FORMAT = {32: (3, 121, 8, 0.875, -117, 120), 16: (1, 127, 2, 0.75, -125, 126),
                 24: (3, 127, 2, 0.9375, -123, 126)}
_MX_SR_SIGN = {32: 7, 16: 3, 24: 5}  # the sign's bit in a code


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


def _mx_sr_quantize_blocks(xb: torch.Tensor, u: torch.Tensor, pb: int):
    """(blocks, 32) f32 and (blocks, 32) words -> (payload, scale bytes): the contract's Q with the payload
    rounded stochastically. The scale is the nearest path's; the code of |s| is that of the grid point below
    it plus one where u < T, T = floor(t 2^32), read off the f32 bits of s."""
    mb, fmin, bias, switch, emin, emax = _MX_SR_FORMAT[pb]
    amax = xb.abs().amax(dim=1)
    special = ~torch.isfinite(xb).all(dim=1)
    zero = (amax == 0) & ~special
    m, ex = torch.frexp(torch.where(special | zero, torch.ones_like(amax), amax))
    e = ((ex.to(torch.int64) - 1) - bias + (m > switch).to(torch.int64)).clamp(emin, emax)
    e[zero] = 0
    bits = (xb * _mx_exp2(-e)[:, None]).view(torch.int32).to(torch.int64) & _M32  # one f32 product
    a = bits & 0x7FFFFFFF
    field, mant = a >> 23, (a & 0x7FFFFF) | 0x800000
    normal = field >= fmin
    sh = 23 - mb + (fmin - field).clamp(0, 40)
    lo = torch.where(normal, (field - fmin) << mb, torch.zeros_like(a)) + (mant >> sh)
    thr = ((mant & ((torch.ones_like(sh) << sh) - 1)) << 32) >> sh
    code = (lo + (u < thr).to(torch.int64)) | ((bits >> 31) << _MX_SR_SIGN[pb])
    code[special | zero] = 0
    code = code.to(torch.uint8)
    q = code if pb == 32 else (_mx6_pack(code) if pb == 24 else (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous())
    s = (e + 127).to(torch.uint8)
    s[special] = 255
    return q, s


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
    """(payload bytes per block, Q, D) of a format."""
    pb = _mx_payload(wire, who)
    return {32: (pb, _mx_quantize_blocks, _mx_dequantize_blocks), 16: (pb, _mx4_quantize_blocks, _mx4_dequantize_blocks),
            24: (pb, _mx6_quantize_blocks, _mx6_dequantize_blocks)}[pb]


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
    pb, Q, D = _mx_blocks_fns(wire, "mx_quantize_reference")
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
        return _mx_join(*_mx_sr_quantize_blocks(xb.view(total, MX_BLOCK), u.view(total, MX_BLOCK), pb), world)
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
    pb, Q, D = _mx_blocks_fns(wire, "mx_reduce_reference")
    q, s = _mx_split(w, nsrc, pb)
    cb = s.numel() // nsrc
    d = D(q, s).view(nsrc, cb, MX_BLOCK)
    acc = d[0].clone()
    for r in range(1, nsrc):
        acc = acc + d[r]
    if op == "avg":
        acc = acc / torch.tensor(float(nsrc), dtype=torch.float32)
    if _mx_check_rounding(rounding, seed, stream, 0, 0, residual, "mx_reduce_reference"):
        u = _mx_sr_words(mx_sr_key(seed, stream), 0, cb * MX_BLOCK).view(cb, MX_BLOCK)
        return _mx_join(*_mx_sr_quantize_blocks(acc, u, pb), 1)
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
    pb, _, D = _mx_blocks_fns(wire, "mx_dequantize_reference")
    world = max(1, int(world))
    if w.numel() != mx_wire_bytes(numel, world, wire=wire):
        raise ValueError(f"the wire of {numel} elements in {world} chunks has "
                         f"{mx_wire_bytes(numel, world, wire=wire)} bytes, got {w.numel()}")
    q, s = _mx_split(w, world, pb)
    d = D(q, s)
    if rot:
        d = _mx_rot_inverse(d, mx_rotation_signs(rotation_seed))
    return d.reshape(-1)[:int(numel)].to(dtype)


def mx_quantize_shards_reference(x: torch.Tensor, world: int, *, wire: str = "mxfp8_e4m3",
                                 residual: torch.Tensor | None = None, rounding: str = "nearest", seed: int = 0,
                                 stream: int = 0, index_offset: int = 0, rotation: str | None = None,
                                 rotation_seed: int = 0) -> torch.Tensor:
    """Plain-PyTorch :func:`mx_quantize_shards` on a CPU tensor (``residual``: updated in place; ``rounding``,
    ``seed``, ``stream``, ``index_offset``, ``rotation``, ``rotation_seed``: as in :func:`mx_quantize_shards`)."""
    _mx_check_dtype(x.dtype, "mx_quantize_shards_reference")
    _mx_payload(wire, "mx_quantize_shards_reference")
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
    pb, _, D = _mx_blocks_fns(wire, "mx_dequantize_shards_reference")
    m, world = int(shard_numel), int(world)
    _mx_check_shards(m * world, world, "mx_dequantize_shards_reference")
    if w.numel() != mx_shard_wire_bytes(m, world, wire=wire):
        raise ValueError(f"the wire of {world} shards of {m} elements has "
                         f"{mx_shard_wire_bytes(m, world, wire=wire)} bytes, got {w.numel()}")
    q, s = _mx_split(w, world, pb)
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
    pb, _, D = _mx_blocks_fns(wire, "mx_fold_reference")
    nsrc, numel = int(nsrc), int(numel)
    if numel < 1 or w.numel() != mx_shard_wire_bytes(numel, nsrc, wire=wire):
        raise ValueError(f"{nsrc} chunk wires of {numel} elements have "
                         f"{mx_shard_wire_bytes(numel, nsrc, wire=wire)} bytes, got {w.numel()}")
    q, s = _mx_split(w, nsrc, pb)
    d = D(q, s).view(nsrc, -1)
    acc = d[0].clone()
    for r in range(1, nsrc):
        acc = acc + d[r]
    if op == "avg":
        acc = acc / torch.tensor(float(nsrc), dtype=torch.float32)
    if rot:
        acc = _mx_rot_inverse(acc.view(-1, MX_BLOCK), mx_rotation_signs(rotation_seed)).reshape(-1)
    return acc[:numel].to(dtype)


__all__ = ["reduce_nway", "reduce_nway_reference", "multi_copy", "pack", "unpack",
           "MX_WIRES", "MX_ROUNDINGS", "MX_ROTATIONS", "mx_sr_key", "mx_rotation_signs",
           "mx_quantize", "mx_reduce", "mx_dequantize", "mx_chunk_blocks", "mx_wire_bytes",
           "mx_owner_residual_numel",
           "mx_quantize_reference", "mx_reduce_reference", "mx_dequantize_reference",
           "mx_shard_blocks", "mx_shard_wire_bytes", "mx_quantize_shards", "mx_dequantize_shards", "mx_fold",
           "mx_quantize_shards_reference", "mx_dequantize_shards_reference", "mx_fold_reference"]
