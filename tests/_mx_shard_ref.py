"""The independent reference of the shard layout and of the two collectives built on it
(docs/collectives.md "Compressed reduce-scatter and all-gather"), for the tests only.

numpy on top of tests/_mx_ref.py's block functions (`q_blocks`, `d_blocks`, `fold_blocks`,
`pad_blocks`, `join`); it shares no code with `ops.*_reference` or the kernels. A shard wire of W
shards of m elements is W chunks of `shard_blocks(m)` blocks, and chunk r is shard r alone: its
blocks are counted from the shard's first element, and what lies past its end is +0.
"""
import numpy as np
import torch

from tests import _mx_ref as R


def shard_blocks(m):
    return R.chunk_blocks(m, 1)


def shard_wire_bytes(m, world):
    return 33 * shard_blocks(m) * world


def quantize_shards(x, W):
    """flat numpy f32 of W * m elements -> shard wire (uint8 array)."""
    assert x.size % W == 0 and x.size >= W, (x.size, W)
    m = x.size // W
    cb = shard_blocks(m)
    return np.concatenate([R.join(*R.q_blocks(R.pad_blocks(x[r * m:(r + 1) * m], cb)), 1) for r in range(W)])


def _chunks(wire, n, cb):
    """(n, cb, 32) payload and (n, cb) scales of n chunk wires back to back."""
    wire = np.asarray(wire, dtype=np.uint8)
    assert wire.size == 33 * cb * n, (wire.size, n, cb)
    w = wire.reshape(n, 33 * cb)
    return w[:, :32 * cb].reshape(n, cb, 32), w[:, 32 * cb:]


def dequantize_shards(wire, m, W, dtype=torch.float32):
    """shard wire -> torch tensor of W * m elements, rounded once to `dtype`."""
    q, s = _chunks(wire, W, shard_blocks(m))
    v = np.concatenate([R.d_blocks(q[r], s[r]).reshape(-1)[:m] for r in range(W)])
    return torch.from_numpy(v.copy()).to(dtype)


def fold(wire, nsrc, numel, op="sum", dtype=torch.float32):
    """`nsrc` chunk wires of shard_blocks(numel) blocks -> torch tensor of `numel` elements: the f32
    fold in source order (AVG: one true f32 division), rounded once to `dtype`."""
    q, s = _chunks(wire, nsrc, shard_blocks(numel))
    acc = R.fold_blocks([R.d_blocks(q[r], s[r]) for r in range(nsrc)], op)
    return torch.from_numpy(acc.reshape(-1)[:numel].copy()).to(dtype)


def reduce_scatter(xs, rank, op="sum", dtype=torch.float32):
    """What rank `rank` holds after reduce_scatter_compressed of `xs` (one torch tensor of W * m
    elements per rank, rank order): cast(fold_r D(Q(x_r[rank m:(rank + 1) m])))."""
    W = len(xs)
    m = xs[0].numel() // W
    blocks = -(-m // R.BLOCK)
    ds = [R.d_blocks(*R.q_blocks(R.pad_blocks(R.f32(x)[rank * m:(rank + 1) * m], blocks))) for x in xs]
    y = R.fold_blocks(ds, op).reshape(-1)[:m]
    return torch.from_numpy(y.copy()).to(dtype)


def all_gather(shards, dtype=torch.float32):
    """What every rank holds after all_gather_compressed of `shards` (rank order): cat_r cast(D(Q(x_r)))."""
    out = []
    for x in shards:
        v = R.f32(x)
        out.append(R.d_blocks(*R.q_blocks(R.pad_blocks(v, -(-v.size // R.BLOCK)))).reshape(-1)[:v.size])
    return torch.from_numpy(np.concatenate(out)).to(dtype)


def same_shard_wire(got, ref, nchunks):
    """Wires equal byte for byte, except the payload under scale 255 (unspecified)."""
    got, ref = np.asarray(got, dtype=np.uint8), np.asarray(ref, dtype=np.uint8)
    if got.shape != ref.shape or got.size % (33 * nchunks):
        return False
    cb = got.size // (33 * nchunks)
    gq, gs = _chunks(got, nchunks, cb)
    rq, rs = _chunks(ref, nchunks, cb)
    return bool(np.array_equal(gs, rs) and np.array_equal(gq[rs != 255], rq[rs != 255]))
