"""An independent reference of stochastic rounding on the block-scaled wires (docs/collectives.md
"Stochastic rounding"), for the tests only.

The grids, `t` and `T`, `mix`, the keys and the words are written here from the contract, in numpy:
the magnitudes of a format are a table, `lo` and `hi` come out of a search in it, and `t` is formed in
float64, where `a - lo`, the division by the power of two `hi - lo` and the product with 2^32 are all
exact (the scaled value is `ldexp` of the f32 input, which equals the contract's f32 product wherever
that product is a normal f32; below 2^-126 `T` is 0 either way). Blocks, scales, layouts and `D` are
those of tests/_mx_ref.py and tests/_mx4_ref.py. Nothing is shared with `ops.*_reference`, the kernels
or csrc/kernels/mx_sr.h.
"""
import numpy as np
import torch

from tests import _mx4_ref as R4
from tests import _mx_ref as R8

BLOCK = 32
WIRES = {"mxfp8_e4m3": R8, "mxfp4_e2m1": R4}
DTYPES = R8.DTYPES
M32 = 0xFFFFFFFF

# magnitudes of the codes 0..126 of float8_e4m3fn (127 is NaN) and 0..7 of e2m1, ascending
GRID8 = np.array([k * 2.0 ** -9 for k in range(8)]
                 + [2.0 ** (ex - 7) * (1 + m / 8) for ex in range(1, 16) for m in range(8)][:119])
GRID4 = R4.MAGS.astype(np.float64)
GRIDS = {"mxfp8_e4m3": GRID8, "mxfp4_e2m1": GRID4}
assert GRID8.size == 127 and GRID8[-1] == 448.0 and GRID8[8] == 2.0 ** -6 and (np.diff(GRID8) > 0).all()
# the largest grid step (the top binade): G of the unbiasedness bound, in units of 2^e
STEP = {"mxfp8_e4m3": 32.0, "mxfp4_e2m1": 2.0}


# ------------------------------------------------------------------ random words
def mix(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def key(seed, stream):
    seed, stream = int(seed), int(stream)
    assert 0 <= seed < 1 << 64 and 0 <= stream < 1 << 32
    k = int(mix((seed & M32) ^ 0x9E3779B9))
    k = int(mix((k + (seed >> 32)) & M32))
    return int(mix((k + stream) & M32))


def words(k, idx):
    """u_i for the element indices `idx` (any shape, below 2^64) under the key k."""
    idx = np.asarray(idx, dtype=np.uint64)
    h = idx >> 32
    kh = np.where(h == 0, np.uint64(k), mix((np.uint64(k) + h) & M32))
    return mix((idx & M32) ^ kh)


# ------------------------------------------------------------------ one element
def split(a, wire):
    """a: float64 magnitudes within the grid -> (index of lo, T = floor(t 2^32) as uint64)."""
    g = GRIDS[wire]
    a = np.asarray(a, dtype=np.float64)
    assert (a >= 0).all() and (a <= g[-1]).all()
    lo = np.searchsorted(g, a, side="right") - 1
    hi = np.minimum(lo + 1, g.size - 1)
    width = np.where(hi > lo, g[hi] - g[lo], 1.0)
    t = (a - g[lo]) / width
    assert (t >= 0).all() and (t < 1).all()
    return lo, np.floor(t * 4294967296.0).astype(np.uint64)


def code_of(s, u, wire):
    """Scaled values s (float64) and words u -> codes: the index of the magnitude, the sign above it."""
    s = np.asarray(s, dtype=np.float64)
    lo, T = split(np.abs(s), wire)
    c = lo + (np.asarray(u, dtype=np.uint64) < T)
    return (c | (np.signbit(s).astype(np.int64) << (7 if wire == "mxfp8_e4m3" else 3))).astype(np.uint8)


def codes(xb, ub, wire):
    """(B, 32) f32 and (B, 32) words -> ((B, 32) codes, (B,) scale bytes)."""
    R = WIRES[wire]
    xb = np.ascontiguousarray(xb, dtype=np.float32)
    amax = (xb.view(np.uint32) & 0x7FFFFFFF).astype(np.int64).max(axis=1)
    special = amax >= 0x7F800000
    blank = special | (amax == 0)
    e = R.scale_exponent(amax)
    safe = np.where(blank[:, None], 0.0, xb.astype(np.float64))
    c = code_of(np.ldexp(safe, -e[:, None].astype(np.int64)), ub, wire)
    c[blank] = 0
    s = (e + 127).astype(np.uint8)
    s[special] = 255
    return c, s


def q_blocks(xb, ub, wire):
    """(B, 32) f32 and words -> (payload, scale bytes) in the layout of the format's own q_blocks."""
    c, s = codes(xb, ub, wire)
    if wire == "mxfp4_e2m1":
        c = (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)
    return c, s


def d_values(q, s, wire):
    return WIRES[wire].d_blocks(q, s)


# ------------------------------------------------------------------ wires
def quantize(x, world, wire, seed=0, stream=0, index_offset=0):
    """flat f32 x -> dealt wire of `world` chunks; element p of x draws the word of index_offset + p."""
    R = WIRES[wire]
    blocks = R.chunk_blocks(x.size, world) * world
    idx = np.uint64(index_offset) + np.arange(blocks * BLOCK, dtype=np.uint64)
    u = words(key(seed, stream), idx).reshape(blocks, BLOCK)
    return R.join(*q_blocks(R.pad_blocks(x, blocks), u, wire), world)


def quantize_shards(x, W, wire, seed=0, stream=0, index_offset=0):
    """flat f32 x of W * m elements -> shard wire; the words are those of the element's index in x."""
    R = WIRES[wire]
    assert x.size % W == 0 and x.size >= W
    m = x.size // W
    cb = R.chunk_blocks(m, 1)
    k = key(seed, stream)
    out = []
    for r in range(W):
        idx = np.uint64(index_offset + r * m) + np.arange(cb * BLOCK, dtype=np.uint64)
        out.append(R.join(*q_blocks(R.pad_blocks(x[r * m:(r + 1) * m], cb), words(k, idx).reshape(cb, BLOCK), wire), 1))
    return np.concatenate(out)


def reduce(wire_bytes, nsrc, op, wire, seed=0, stream=0):
    """`nsrc` chunk wires back to back -> one chunk wire; element j of the chunk draws the word of j."""
    R = WIRES[wire]
    q, s = R.split(wire_bytes, nsrc)
    cb = s.size // nsrc
    d = R.d_blocks(q, s).reshape(nsrc, cb, BLOCK)
    acc = R.fold_blocks([d[k] for k in range(nsrc)], op)
    u = words(key(seed, stream), np.arange(cb * BLOCK, dtype=np.uint64)).reshape(cb, BLOCK)
    return R.join(*q_blocks(acc, u, wire), 1)


# ------------------------------------------------------------------ the collectives, one process
def all_reduce(xs, op, wire, seeds, dtype=torch.float32):
    """all_reduce_compressed(rounding="stochastic"): rank r quantizes with (seeds[r], 2 r) and requantizes
    the chunk it owns with (seeds[r], 2 r + 1). Returns what every rank ends with."""
    R = WIRES[wire]
    W, n = len(xs), xs[0].numel()
    wires = [quantize(R.f32(xs[r]), W, wire, seeds[r], 2 * r) for r in range(W)]
    cbytes = wires[0].size // W
    chunks = [reduce(np.concatenate([w[r * cbytes:(r + 1) * cbytes] for w in wires]), W, op, wire, seeds[r], 2 * r + 1)
              for r in range(W)]
    return R.dequantize(np.concatenate(chunks), n, W, dtype)


def reduce_scatter(xs, rank, op, wire, seeds, dtype=torch.float32):
    """reduce_scatter_compressed(rounding="stochastic") as rank `rank` sees it: stream 2 r on rank r."""
    R = WIRES[wire]
    W = len(xs)
    m = xs[0].numel() // W
    cb = R.chunk_blocks(m, 1)
    got = [quantize_shards(R.f32(xs[r]), W, wire, seeds[r], 2 * r) for r in range(W)]
    cbytes = got[0].size // W
    recv = np.concatenate([g[rank * cbytes:(rank + 1) * cbytes] for g in got])
    d = R.d_blocks(*R.split(recv, W)).reshape(W, cb, BLOCK)
    acc = R.fold_blocks([d[j] for j in range(W)], op)
    return torch.from_numpy(acc.reshape(-1)[:m].copy()).to(dtype)


def all_gather(shards, wire, seeds, dtype=torch.float32):
    """all_gather_compressed(rounding="stochastic"): rank r quantizes its shard with (seeds[r], 2 r)."""
    R = WIRES[wire]
    W, m = len(shards), shards[0].numel()
    every = np.concatenate([quantize(R.f32(shards[r]), 1, wire, seeds[r], 2 * r) for r in range(W)])
    return torch.from_numpy(R.d_blocks(*R.split(every, W)).reshape(W, -1)[:, :m].reshape(-1).copy()).to(dtype)


def call_seed(seed, step, nbuckets, b):
    """The seed GradBucketer / ShardedOptimizer give bucket b at synchronised step `step` (0-based)."""
    return (int(seed) + step * nbuckets + b) % (1 << 64)


# ------------------------------------------------------------------ the scaled values of the host-program list
def f32_bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


def probe_values(wire):
    """f32 scaled values that exercise every branch of the rounding: every grid point, every midpoint, the
    f32 neighbours of every grid point, and 2^-k for k up to 40 with its neighbours; both signs."""
    g = GRIDS[wire].astype(np.float32)
    mids = ((GRIDS[wire][1:] + GRIDS[wire][:-1]) / 2).astype(np.float32)
    top = g[-1]
    up = np.nextafter(g[:-1], np.float32(np.inf))
    down = np.nextafter(g[1:], np.float32(0))
    small = np.ldexp(np.float32(1), -np.arange(1, 41)).astype(np.float32)
    small = np.concatenate([small, np.nextafter(small, np.float32(np.inf)), np.nextafter(small, np.float32(0)),
                            (1.5 * small).astype(np.float32), np.array([1e-38, 1e-45, 2.0 ** -126], dtype=np.float32)])
    v = np.concatenate([g, mids, up, down, small])
    v = v[v <= top]
    return np.concatenate([v, -v]).astype(np.float32)


def probe_words(T):
    """The words the contract's decision turns on for a value with threshold T: {0, 1, T-1, T, T+1, 2^32-1}."""
    T = int(T)
    return sorted({0, 1, max(T - 1, 0), min(T, M32), min(T + 1, M32), M32})


def same_wire(got, ref, nchunks, wire):
    return WIRES[wire].same_wire(got, ref, nchunks)
