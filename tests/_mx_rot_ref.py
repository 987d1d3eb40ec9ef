"""Independent numpy reference of the Hadamard rotation (docs/collectives.md "Hadamard rotation") for the tests
of all three block-scaled wires: the sign word, R and R^-1 written as explicit index pairs on np.float32
columns, and the rotated quantize / dequantize / fold and collectives composed from the wires' own independent
references (tests/_mx_ref.py, _mx4_ref.py, _mx6_ref.py, _mx_sr_ref.py). It shares no code with the ops twins.
"""
import numpy as np
import torch

from tests import _mx4_ref as R4
from tests import _mx6_ref as R6
from tests import _mx_ref as R8
from tests import _mx_sr_ref as SR

BLOCK = 32
STREAM = 0x52484431
WIRES = {"mxfp8_e4m3": R8, "mxfp4_e2m1": R4, "mxfp6_e2m3": R6}
DTYPES = R8.DTYPES
BOUND_C = {"mxfp8_e4m3": 16.0, "mxfp4_e2m1": 3.0, "mxfp6_e2m3": 16.0}  # one nearest quantization: amax(t) / c
f32 = R8.f32


def signs(seed):
    """The sign word: the word of index 0 under the key of (seed, STREAM)."""
    return int(SR.words(SR.key(seed, STREAM), np.array([0], dtype=np.uint64))[0])


def hadamard():
    """H[i][j] = (-1)^popcount(i & j) as float64."""
    return np.array([[(-1.0) ** bin(i & j).count("1") for j in range(BLOCK)] for i in range(BLOCK)])


def flip(yb, sg):
    yb = np.ascontiguousarray(yb, dtype=np.float32)
    mask = np.array([0x80000000 if (sg >> j) & 1 else 0 for j in range(BLOCK)], dtype=np.uint32)
    return (yb.view(np.uint32) ^ mask[None, :]).view(np.float32)


def butterfly(yb):
    """(B, 32) f32 -> the five stages, pair by pair; every add and subtract is one np.float32 operation."""
    y = [np.ascontiguousarray(yb[:, j], dtype=np.float32).copy() for j in range(BLOCK)]
    with np.errstate(all="ignore"):
        for h in (1, 2, 4, 8, 16):
            for j in range(BLOCK):
                if j & h == 0:
                    a, b = y[j], y[j + h]
                    y[j], y[j + h] = (a + b).astype(np.float32), (a - b).astype(np.float32)
    return np.stack(y, axis=1)


def forward(xb, sg):
    return butterfly(flip(xb, sg))


def inverse(db, sg):
    with np.errstate(all="ignore"):
        return flip((butterfly(db) * np.float32(0.03125)).astype(np.float32), sg)


# ------------------------------------------------------------------ blocks of one wire
def q_blocks(tb, wire, ub=None):
    if ub is None:
        return WIRES[wire].q_blocks(tb)
    return R6.q_blocks(tb, ub) if wire == "mxfp6_e2m3" else SR.q_blocks(tb, ub, wire)


def _words(sr, first, blocks):
    """sr = (seed, stream, index_offset) or None."""
    if sr is None:
        return None
    idx = np.uint64(sr[2] + first) + np.arange(blocks * BLOCK, dtype=np.uint64)
    return SR.words(SR.key(sr[0], sr[1]), idx).reshape(blocks, BLOCK)


def _q_rot(x, blocks, wire, seed, res=None, ub=None):
    """flat f32 x -> (payload, scales, new residual or None): R on the padded blocks, then + residual, then Q."""
    R = WIRES[wire]
    tb = forward(R.pad_blocks(x, blocks), signs(seed))
    if res is not None:
        rb = R.pad_blocks(np.asarray(res, dtype=np.float32), blocks)
        with np.errstate(all="ignore"):
            tb = (tb + rb).astype(np.float32)
    q, s = q_blocks(tb, wire, ub)
    new = None
    if res is not None:
        with np.errstate(all="ignore"):
            r = (tb - R.d_blocks(q, s)).astype(np.float32)
        new = np.where(np.isfinite(r), r, np.float32(0)).astype(np.float32).reshape(-1)[:x.size].copy()
    return q, s, new


def quantize(x, world, wire, seed, res=None, sr=None):
    """Dealt layout. Returns the wire, or (wire, new residual) with `res`."""
    R = WIRES[wire]
    blocks = R.chunk_blocks(x.size, world) * world
    q, s, new = _q_rot(x, blocks, wire, seed, res, _words(sr, 0, blocks))
    w = R.join(q, s, world)
    return w if res is None else (w, new)


def quantize_shards(x, W, wire, seed, res=None, sr=None):
    R = WIRES[wire]
    m = x.size // W
    cb = R.chunk_blocks(m, 1)
    wires, news = [], []
    for r in range(W):
        q, s, new = _q_rot(x[r * m:(r + 1) * m], cb, wire, seed, None if res is None else res[r * m:(r + 1) * m],
                           _words(sr, r * m, cb))
        wires.append(R.join(q, s, 1))
        news.append(new)
    w = np.concatenate(wires)
    return w if res is None else (w, np.concatenate(news))


def _out(v, dtype):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dtype)


def dequantize(w, numel, world, wire, seed, dtype=torch.float32):
    R = WIRES[wire]
    return _out(inverse(R.d_blocks(*R.split(w, world)), signs(seed)).reshape(-1)[:numel], dtype)


def dequantize_shards(w, m, W, wire, seed, dtype=torch.float32):
    R = WIRES[wire]
    return _out(inverse(R.d_blocks(*R.split(w, W)), signs(seed)).reshape(W, -1)[:, :m].reshape(-1), dtype)


def _fold_blocks(w, nsrc, op, wire):
    R = WIRES[wire]
    d = R.d_blocks(*R.split(w, nsrc)).reshape(nsrc, -1, BLOCK)
    return R.fold_blocks([d[r] for r in range(nsrc)], op)


def fold(w, nsrc, numel, op, wire, seed, dtype=torch.float32):
    return _out(inverse(_fold_blocks(w, nsrc, op, wire), signs(seed)).reshape(-1)[:numel], dtype)


def reduce(w, nsrc, op, wire, res=None, sr=None):
    """The owner stage: no rotation argument. Returns the chunk wire, or (wire, new owner residual)."""
    R = WIRES[wire]
    acc = _fold_blocks(w, nsrc, op, wire)
    if res is not None:
        with np.errstate(all="ignore"):
            acc = (acc + res.reshape(acc.shape)).astype(np.float32)
    q, s = q_blocks(acc, wire, _words(sr, 0, acc.shape[0]))
    if res is None:
        return R.join(q, s, 1)
    with np.errstate(all="ignore"):
        r = (acc - R.d_blocks(q, s)).astype(np.float32)
    return R.join(q, s, 1), np.where(np.isfinite(r), r, np.float32(0)).astype(np.float32).reshape(-1)


# ------------------------------------------------------------------ the collectives
def all_reduce(xs, op, wire, seed, dtype=torch.float32, rs=None, r2s=None, sr_seeds=None):
    """cast(R^-1 D(Q(fold_r D(Q(R x_r))))). rs / r2s: local / owner residuals per rank (both or neither);
    sr_seeds: one stochastic seed per rank. Returns the result, with residuals (result, new rs, new r2s)."""
    W, n = len(xs), xs[0].numel()
    got = [quantize(f32(xs[k]), W, wire, seed, None if rs is None else rs[k],
                    None if sr_seeds is None else (sr_seeds[k], 2 * k, 0)) for k in range(W)]
    wires = got if rs is None else [g[0] for g in got]
    cbytes = wires[0].size // W
    chunks = [reduce(np.concatenate([w[k * cbytes:(k + 1) * cbytes] for w in wires]), W, op, wire,
                     None if r2s is None else r2s[k], None if sr_seeds is None else (sr_seeds[k], 2 * k + 1, 0))
              for k in range(W)]
    cw = chunks if r2s is None else [c[0] for c in chunks]
    y = dequantize(np.concatenate(cw), n, W, wire, seed, dtype)
    return y if rs is None else (y, [g[1] for g in got], [c[1] for c in chunks])


def reduce_scatter(xs, op, wire, seed, dtype=torch.float32, rs=None, sr_seeds=None):
    """[rank k's output], with residuals ([outputs], new rs)."""
    W = len(xs)
    m = xs[0].numel() // W
    got = [quantize_shards(f32(xs[k]), W, wire, seed, None if rs is None else rs[k],
                           None if sr_seeds is None else (sr_seeds[k], 2 * k, 0)) for k in range(W)]
    wires = got if rs is None else [g[0] for g in got]
    cbytes = wires[0].size // W
    outs = [fold(np.concatenate([w[k * cbytes:(k + 1) * cbytes] for w in wires]), W, m, op, wire, seed, dtype)
            for k in range(W)]
    return outs if rs is None else (outs, [g[1] for g in got])


def all_gather(shards, wire, seed, dtype=torch.float32, sr_seeds=None):
    W, m = len(shards), shards[0].numel()
    every = np.concatenate([quantize(f32(shards[r]), 1, wire, seed, None,
                                     None if sr_seeds is None else (sr_seeds[r], 2 * r, 0)) for r in range(W)])
    return dequantize_shards(every, m, W, wire, seed, dtype)


# ------------------------------------------------------------------ comparisons
same = R6.same
same_residual = R6.same_residual


def same_wire(got, ref, nchunks, wire):
    """Byte for byte, except the payload of NaN blocks (scale 255), which is unspecified."""
    R = WIRES[wire]
    got, ref = np.asarray(got, dtype=np.uint8), np.asarray(ref, dtype=np.uint8)
    if got.shape != ref.shape:
        return False
    gq, gs = R.split(got, nchunks)
    rq, rs = R.split(ref, nchunks)
    return bool(np.array_equal(gs, rs) and np.array_equal(gq[rs != 255], rq[rs != 255]))


def edge_tensor(wire):
    return WIRES[wire].edge_tensor()[0]
