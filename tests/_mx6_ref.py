"""An independent reference of the `mxfp6_e2m3` wire format (docs/collectives.md "The `mxfp6_e2m3`
wire format"), for the tests only.

It shares no code with `ops.*_reference` or the kernels. The 32 magnitudes of the e2m3 codes are a
float64 table; the scaled value `x 2^-e` is `ldexp` in float64 (exact), the nearest code is found by
comparing distances to the table, the even code at a tie. Dequantization is the table and `ldexp`,
rounded once to f32. The payload is packed and unpacked bit by bit: the code of element j occupies bits
6j .. 6j + 5 of the block's 192, bit n of the stream being bit n % 8 of byte n / 8. The error-feedback and
the stochastic variants are built on the same pieces (the random words come from tests/_mx_sr_ref.py,
`t` is formed in float64 against the table). torch appears only for the final cast to a tensor's dtype.
"""
import numpy as np
import torch

from tests._mx_sr_ref import key as sr_key
from tests._mx_sr_ref import words as sr_words

BLOCK = 32
PAYLOAD = 24
BLOCK_WIRE = PAYLOAD + 1
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
WIRE = "mxfp6_e2m3"
# magnitudes of the codes 0..31: m / 8, then (1 + m / 8) 2^k for k = 0, 1, 2
MAGS = np.array([m / 8 for m in range(8)] + [(1 + m / 8) * 2.0 ** k for k in range(3) for m in range(8)])
assert MAGS.size == 32 and MAGS[-1] == 7.5 and MAGS[8] == 1.0 and (np.diff(MAGS) > 0).all()
STEP = 0.5         # the largest grid step (the top binade), in units of 2^e
BOUND_DIV = 15.0   # error feedback: |r| <= A / 15 (1 + 2^-10)


def chunk_blocks(numel, world=1):
    per = -(-(-(-numel // BLOCK)) // world)
    cb = max(16, -(-per // 16) * 16)
    if cb * BLOCK_WIRE >= 1048576:
        cb = -(-cb // 4096) * 4096
    return cb


def wire_bytes(numel, world=1):
    return BLOCK_WIRE * chunk_blocks(numel, world) * world


def shard_blocks(m):
    return chunk_blocks(m, 1)


def shard_wire_bytes(m, world):
    return BLOCK_WIRE * shard_blocks(m) * world


def shard_payload_byte(m, i):
    """wire byte that holds the lowest bit of the code of element i of a shard wire of m-element shards."""
    r, p = divmod(i, m)
    return r * BLOCK_WIRE * shard_blocks(m) + (p // BLOCK) * PAYLOAD + (6 * (p % BLOCK)) // 8


def shard_scale_byte(m, i):
    r, p = divmod(i, m)
    return r * BLOCK_WIRE * shard_blocks(m) + PAYLOAD * shard_blocks(m) + p // BLOCK


def f32(t):
    """torch tensor of a supported dtype -> flat numpy f32 (exact widening)."""
    return t.detach().reshape(-1).to(torch.float32).numpy().copy()


# ------------------------------------------------------------------ the bit stream
def pack_codes(code):
    """(B, 32) six-bit codes -> (B, 24) payload bytes."""
    code = np.asarray(code, dtype=np.uint8)
    bits = (code[:, :, None] >> np.arange(6, dtype=np.uint8)) & 1           # (B, 32, 6): bit 6j + b of the stream
    return np.packbits(bits.reshape(code.shape[0], 192), axis=1, bitorder="little")


def unpack_codes(q):
    """(B, 24) payload bytes -> (B, 32) six-bit codes."""
    q = np.asarray(q, dtype=np.uint8)
    bits = np.unpackbits(q, axis=1, bitorder="little").reshape(q.shape[0], 32, 6)
    return (bits << np.arange(6, dtype=np.uint8)).sum(axis=2).astype(np.uint8)


# ------------------------------------------------------------------ blocks
def scale_exponent(amax_bits):
    """e of the contract from max |x| as f32 bits; 0 for an all-zero block."""
    a = np.asarray(amax_bits).astype(np.int64)
    e = (a >> 23) - 127 - 2 + ((a & 0x7FFFFF) > 0x700000)
    e = np.minimum(np.maximum(e, -123), 126)
    e[a == 0] = 0
    return e


def _scaled(xb):
    """(B, 32) f32 -> (float64 x 2^-e with 0 in blank blocks, e, special, blank)."""
    xb = np.ascontiguousarray(xb, dtype=np.float32)
    amax = (xb.view(np.uint32) & 0x7FFFFFFF).astype(np.int64).max(axis=1)
    special = amax >= 0x7F800000
    blank = special | (amax == 0)
    e = scale_exponent(amax)
    safe = np.where(blank[:, None], 0.0, xb.astype(np.float64))
    return np.ldexp(safe, -e[:, None]), e, special, blank


def _finish(code, xb, e, special, blank):
    code = code.astype(np.uint8) | (np.signbit(np.asarray(xb, dtype=np.float32)).astype(np.uint8) << 5)
    code[blank] = 0
    s = (e + 127).astype(np.uint8)
    s[special] = 255
    return code, s


def _nearest_even(dist):
    """(32, B, 32) distances to the 32 magnitudes -> the index of the smallest, the even one of two equal ones."""
    best = dist.min(axis=0)
    hit = dist == best[None]                      # one code, or two neighbours at a tie
    first = hit.argmax(axis=0)
    last = 31 - hit[::-1].argmax(axis=0)
    return np.where(first % 2 == 0, first, last)  # (neighbouring codes: exactly one of the two is even)


def codes(xb):
    """(B, 32) f32 -> ((B, 32) e2m3 codes with the sign in bit 5, (B,) scale bytes): nearest, ties to even."""
    sc, e, special, blank = _scaled(xb)
    code = np.empty(sc.shape, dtype=np.int64)
    for b0 in range(0, sc.shape[0], 2048):  # (slabs: the distances are 32 float64 per element)
        dist = np.abs(np.abs(sc[b0:b0 + 2048])[None] - MAGS[:, None, None])   # (32, B, 32), exact in float64
        code[b0:b0 + 2048] = _nearest_even(dist)
    return _finish(code, xb, e, special, blank)


def codes_sr(xb, ub):
    """... rounded stochastically: code(lo) + 1 iff u < floor(t 2^32)."""
    sc, e, special, blank = _scaled(xb)
    a = np.abs(sc)
    assert (a <= MAGS[-1]).all()
    lo = np.searchsorted(MAGS, a, side="right") - 1
    hi = np.minimum(lo + 1, 31)
    t = (a - MAGS[lo]) / np.where(hi > lo, MAGS[hi] - MAGS[lo], 1.0)
    assert (t >= 0).all() and (t < 1).all()
    T = np.floor(t * 4294967296.0).astype(np.uint64)
    return _finish(lo + (np.asarray(ub, dtype=np.uint64) < T), xb, e, special, blank)


def q_blocks(xb, ub=None):
    """(B, 32) f32 (and words: stochastic) -> ((B, 24) uint8 payload, (B,) uint8 scale bytes)."""
    code, s = codes(xb) if ub is None else codes_sr(xb, ub)
    return pack_codes(code), s


def d_blocks(q, s):
    """(B, 24) payload and (B,) scale bytes -> (B, 32) f32."""
    c = unpack_codes(q).astype(np.int64)
    v = np.where(c & 32, -MAGS[c & 31], MAGS[c & 31])
    with np.errstate(all="ignore"):
        v = np.ldexp(v, (np.asarray(s).astype(np.int32) - 127)[:, None]).astype(np.float32)  # 4 2^126 and up -> inf
    v[np.asarray(s) == 255] = np.nan
    return v


# ------------------------------------------------------------------ wires
def join(q, s, nchunks):
    cb = s.size // nchunks
    return np.concatenate([q.reshape(nchunks, PAYLOAD * cb), s.reshape(nchunks, cb)], axis=1).reshape(-1)


def split(wire, nchunks):
    wire = np.asarray(wire, dtype=np.uint8)
    assert wire.size % (BLOCK_WIRE * 16 * nchunks) == 0, (wire.size, nchunks)
    cb = wire.size // (BLOCK_WIRE * nchunks)
    w = wire.reshape(nchunks, BLOCK_WIRE * cb)
    return w[:, :PAYLOAD * cb].reshape(nchunks * cb, PAYLOAD), w[:, PAYLOAD * cb:].reshape(nchunks * cb)


def pad_blocks(x, blocks):
    xb = np.zeros(blocks * BLOCK, dtype=np.float32)
    xb[:x.size] = x
    return xb.reshape(blocks, BLOCK)


def _words(seed, stream, first, blocks):
    idx = np.uint64(first) + np.arange(blocks * BLOCK, dtype=np.uint64)
    return sr_words(sr_key(seed, stream), idx).reshape(blocks, BLOCK)


def quantize(x, world=1, sr=None):
    """flat numpy f32 -> dealt wire of `world` chunks. sr = (seed, stream, index_offset): stochastic."""
    blocks = chunk_blocks(x.size, world) * world
    ub = None if sr is None else _words(sr[0], sr[1], sr[2], blocks)
    return join(*q_blocks(pad_blocks(x, blocks), ub), world)


def dequantize(wire, numel, world=1, dtype=torch.float32):
    assert len(wire) == wire_bytes(numel, world), (len(wire), numel, world)
    v = d_blocks(*split(wire, world)).reshape(-1)[:numel]
    return torch.from_numpy(v.copy()).to(dtype)


def quantize_shards(x, W, sr=None):
    """flat numpy f32 of W * m elements -> shard wire; stochastic: an element draws the word of its index in x."""
    assert x.size % W == 0 and x.size >= W, (x.size, W)
    m = x.size // W
    cb = shard_blocks(m)
    return np.concatenate([join(*q_blocks(pad_blocks(x[r * m:(r + 1) * m], cb),
                                          None if sr is None else _words(sr[0], sr[1], sr[2] + r * m, cb)), 1)
                           for r in range(W)])


def dequantize_shards(wire, m, W, dtype=torch.float32):
    assert len(wire) == shard_wire_bytes(m, W), (len(wire), m, W)
    v = d_blocks(*split(wire, W)).reshape(W, -1)[:, :m].reshape(-1)
    return torch.from_numpy(v.copy()).to(dtype)


def fold_blocks(ds, op):
    """f32 fold in list order; AVG: one true f32 division by len(ds)."""
    with np.errstate(all="ignore"):
        acc = ds[0].astype(np.float32)
        for d in ds[1:]:
            acc = (acc + d).astype(np.float32)
        if op == "avg":
            acc = (acc / np.float32(len(ds))).astype(np.float32)
    return acc


def _sources(wire, nsrc):
    q, s = split(wire, nsrc)
    d = d_blocks(q, s).reshape(nsrc, -1, BLOCK)
    return [d[r] for r in range(nsrc)]


def reduce(wire, nsrc, op="sum", sr=None):
    """`nsrc` chunk wires back to back -> one chunk wire. sr = (seed, stream): element j draws the word of j."""
    acc = fold_blocks(_sources(wire, nsrc), op)
    return join(*q_blocks(acc, None if sr is None else _words(sr[0], sr[1], 0, acc.shape[0])), 1)


def fold(wire, nsrc, numel, op="sum", dtype=torch.float32):
    assert len(wire) == shard_wire_bytes(numel, nsrc), (len(wire), numel, nsrc)
    acc = fold_blocks(_sources(wire, nsrc), op)
    return torch.from_numpy(acc.reshape(-1)[:numel].copy()).to(dtype)


# ------------------------------------------------------------------ error feedback
def _add(x, r):
    with np.errstate(all="ignore"):
        return (x.astype(np.float32) + r.astype(np.float32)).astype(np.float32)


def _feed_back(v, d):
    with np.errstate(all="ignore"):
        r = (v.astype(np.float32) - d.astype(np.float32)).astype(np.float32)
    return np.where(np.isfinite(r), r, np.float32(0)).astype(np.float32)


def quantize_ef(x, r, world=1):
    """flat f32 x and residual r -> (dealt wire, new residual)."""
    vb = pad_blocks(_add(x, r), chunk_blocks(x.size, world) * world)
    q, s = q_blocks(vb)
    return join(q, s, world), _feed_back(vb, d_blocks(q, s)).reshape(-1)[:x.size].copy()


def quantize_shards_ef(x, r, W):
    m = x.size // W
    cb = shard_blocks(m)
    wires, rs = [], []
    for k in range(W):
        vb = pad_blocks(_add(x[k * m:(k + 1) * m], r[k * m:(k + 1) * m]), cb)
        q, s = q_blocks(vb)
        wires.append(join(q, s, 1))
        rs.append(_feed_back(vb, d_blocks(q, s)).reshape(-1)[:m])
    return np.concatenate(wires), np.concatenate(rs).astype(np.float32)


def reduce_ef(wire, nsrc, op, r2):
    """`nsrc` chunk wires and the owner residual (32 cb) -> (one chunk wire, new residual)."""
    acc = fold_blocks(_sources(wire, nsrc), op)
    acc = _add(acc, r2.reshape(acc.shape))
    q, s = q_blocks(acc)
    return join(q, s, 1), _feed_back(acc, d_blocks(q, s)).reshape(-1).copy()


# ------------------------------------------------------------------ the collectives
def _dq(v, ub=None):
    return d_blocks(*q_blocks(pad_blocks(v, -(-v.size // BLOCK)), ub))


def all_reduce(xs, op="sum", dtype=torch.float32):
    """D(Q(fold_r D(Q(x_r)))) rounded once to `dtype`; blocks are independent of the chunking."""
    n = xs[0].numel()
    y = d_blocks(*q_blocks(fold_blocks([_dq(f32(x)) for x in xs], op))).reshape(-1)[:n]
    return torch.from_numpy(y.copy()).to(dtype)


def reduce_scatter(xs, rank, op="sum", dtype=torch.float32):
    m = xs[0].numel() // len(xs)
    y = fold_blocks([_dq(f32(x)[rank * m:(rank + 1) * m]) for x in xs], op).reshape(-1)[:m]
    return torch.from_numpy(y.copy()).to(dtype)


def all_gather(shards, dtype=torch.float32):
    out = [_dq(f32(x)).reshape(-1)[:x.numel()] for x in shards]
    return torch.from_numpy(np.concatenate(out)).to(dtype)


def all_reduce_ef(xs, rs, r2s, op, dtype=torch.float32):
    """One all_reduce_compressed call with both residuals: (result, new local residuals, new owner residuals)."""
    W, n = len(xs), xs[0].numel()
    got = [quantize_ef(f32(xs[k]), rs[k], W) for k in range(W)]
    cbytes = got[0][0].size // W
    chunks = [reduce_ef(np.concatenate([g[0][k * cbytes:(k + 1) * cbytes] for g in got]), W, op, r2s[k]) for k in range(W)]
    return dequantize(np.concatenate([c[0] for c in chunks]), n, W, dtype), [g[1] for g in got], [c[1] for c in chunks]


def reduce_scatter_ef(xs, rs, op, dtype=torch.float32):
    """([rank k's output], new local residuals)."""
    W = len(xs)
    m = xs[0].numel() // W
    got = [quantize_shards_ef(f32(xs[k]), rs[k], W) for k in range(W)]
    cbytes = got[0][0].size // W
    outs = [fold(np.concatenate([g[0][k * cbytes:(k + 1) * cbytes] for g in got]), W, m, op, dtype) for k in range(W)]
    return outs, [g[1] for g in got]


def all_reduce_sr(xs, op, seeds, dtype=torch.float32):
    """rounding="stochastic": rank r quantizes with (seeds[r], 2 r) and requantizes its chunk with (seeds[r], 2 r + 1)."""
    W, n = len(xs), xs[0].numel()
    wires = [quantize(f32(xs[r]), W, (seeds[r], 2 * r, 0)) for r in range(W)]
    cbytes = wires[0].size // W
    chunks = [reduce(np.concatenate([w[r * cbytes:(r + 1) * cbytes] for w in wires]), W, op, (seeds[r], 2 * r + 1))
              for r in range(W)]
    return dequantize(np.concatenate(chunks), n, W, dtype)


def reduce_scatter_sr(xs, rank, op, seeds, dtype=torch.float32):
    W = len(xs)
    m = xs[0].numel() // W
    got = [quantize_shards(f32(xs[r]), W, (seeds[r], 2 * r, 0)) for r in range(W)]
    cbytes = got[0].size // W
    return fold(np.concatenate([g[rank * cbytes:(rank + 1) * cbytes] for g in got]), W, m, op, dtype)


def all_gather_sr(shards, seeds, dtype=torch.float32):
    W, m = len(shards), shards[0].numel()
    every = np.concatenate([quantize(f32(shards[r]), 1, (seeds[r], 2 * r, 0)) for r in range(W)])
    return dequantize_shards(every, m, W, dtype)


def same(a, b):
    """Equal as values (rtol = atol = 0), NaN exactly where the reference has NaN."""
    a, b = a.detach().cpu().to(torch.float32).reshape(-1), b.detach().cpu().to(torch.float32).reshape(-1)
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def same_wire(got, ref, nchunks):
    """Wires equal byte for byte, except the payload of NaN blocks (scale 255), which is unspecified."""
    got, ref = np.asarray(got, dtype=np.uint8), np.asarray(ref, dtype=np.uint8)
    if got.shape != ref.shape:
        return False
    gq, gs = split(got, nchunks)
    rq, rs = split(ref, nchunks)
    return bool(np.array_equal(gs, rs) and np.array_equal(gq[rs != 255], rq[rs != 255]))


def same_residual(got, ref):
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float32).reshape(-1)
    ref = np.asarray(ref, dtype=np.float32).reshape(-1)
    return got.shape == ref.shape and bool(np.isfinite(got).all()) and bool((got == ref).all())


# ------------------------------------------------------------------ inputs
def _bits(u):
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def edge_blocks():
    """{name: (32,) f32 block}: every branch of Q."""
    rng = np.random.default_rng(20261021)
    out = {}

    def block(amax, name, fill=True):
        b = np.zeros(BLOCK, dtype=np.float32)
        if fill:
            with np.errstate(all="ignore"):
                b[:] = (rng.uniform(-1, 1, BLOCK) * np.float64(amax)).astype(np.float32)
        b[5] = amax
        out[name] = b

    out["zero"] = np.zeros(BLOCK, dtype=np.float32)
    out["minus_zero"] = np.full(BLOCK, -0.0, dtype=np.float32)
    nan = rng.uniform(-4, 4, BLOCK).astype(np.float32)
    nan[17] = np.nan
    out["one_nan"] = nan
    inf = rng.uniform(-4, 4, BLOCK).astype(np.float32)
    inf[3], inf[20] = -np.inf, np.inf
    out["both_inf"] = inf
    # the m = 1.875 switch of e: mantissa 0x700000 and one ulp to either side, over a few binades
    for j in (-100, -20, 0, 9, 100):
        base = 0x3FF00000 + (j << 23)  # 1.875 2^j
        block(_bits(base), f"amax_1.875_2^{j}")
        block(_bits(base + 1), f"amax_1.875_2^{j}_plus_ulp")
        block(_bits(base - 1), f"amax_1.875_2^{j}_minus_ulp")
    block(-_bits(0x3FF00001), "mant_700001_negative")
    # amax 7.5 -> e = 0, the block is its own scaled value: midpoints (ties) in both signs, values a hair to
    # either side, below half the smallest step in both signs (the signed zero codes), and both zeros
    mids = (MAGS[1:] + MAGS[:-1]) / 2
    t = mids[[0, 1, 7, 8, 15, 16, 23, 30]].astype(np.float32)
    ties = np.concatenate([[7.5], t, -t, np.nextafter(t[:3], np.float32(0)), -np.nextafter(t[:3], np.float32(9)),
                           [0.0624, -0.0624, 1e-30, -1e-30, -0.0, 0.0, -7.5, 4.0, -3.75]]).astype(np.float32)
    assert ties.size == BLOCK, ties.size
    out["ties"] = ties
    with np.errstate(all="ignore"):
        out["ties_2^40"] = np.ldexp(ties.astype(np.float64), 40).astype(np.float32)
        out["ties_2^-60"] = np.ldexp(ties.astype(np.float64), -60).astype(np.float32)
    # the lower clamp: e = -123 whatever amax is below 2^-121
    block(np.float32(2.0 ** -118), "amax_2^-118")
    block(np.float32(2.0 ** -122), "amax_2^-122")
    block(np.float32(2.0 ** -126), "amax_2^-126")
    block(_bits(0x00000123), "amax_subnormal", fill=False)
    block(_bits(0x007FFFFF), "amax_largest_subnormal")
    # the top: e = 126 and a payload of 4 or more dequantizes to inf, from amax 1.9375 2^127 on (it rounds to 4)
    block(_bits(0x7F7FFFFF), "amax_f32_max")
    block(_bits(0x7F780000), "amax_1.9375_2^127")
    block(_bits(0x7F77FFFF), "amax_below_1.9375_2^127")
    block(_bits(0x7F700000), "amax_1.875_2^127")
    block(np.float32(65504.0), "amax_f16_max")
    block(np.float32(2.0 ** -24), "amax_f16_min_subnormal", fill=False)
    block(np.float32(2.0 ** -14), "amax_f16_min_normal")
    block(_bits(0x7F7F0000), "amax_bf16_max")
    return out


def random_binades(blocks, seed, lo=-40, hi=40):
    """(blocks, 32) f32: per-block magnitude 2^U[lo, hi], elements spread over a few binades below it."""
    rng = np.random.default_rng(seed)
    mag = np.ldexp(1.0, rng.integers(lo, hi + 1, size=(blocks, 1)))
    x = rng.standard_normal((blocks, BLOCK)) * mag * np.ldexp(1.0, -rng.integers(0, 4, size=(blocks, BLOCK)))
    return x.astype(np.float32)


def edge_tensor():
    """Every edge block and 96 random blocks over 80 binades, flat f32 (numpy), plus the names."""
    eb = edge_blocks()
    x = np.concatenate([np.stack(list(eb.values())), random_binades(96, 13)])
    return x.reshape(-1).copy(), list(eb)


def position_sweep(e=0):
    """(64, 32) f32: block `shift` holds in element j the grid value of code (j + shift) % 32 times 2^e, and block
    32 + shift the same negated, so every code passes through every bit position of the stream. Code 31 (7.5) is
    in every block, so every block's amax is 7.5 2^e."""
    j = np.arange(32)
    blocks = np.stack([MAGS[(j + sh) % 32] for sh in range(32)])
    return np.ldexp(np.concatenate([blocks, -blocks]), e).astype(np.float32)


def rounding_probe():
    """f32 scaled values (|s| <= 7.5) for the exhaustive rounding test: every grid point, every midpoint, the f32
    neighbours of both, 2^-k down to f32 subnormals with neighbours, and 4096 random values per binade from
    2^-12 to the top; both signs. The count is a multiple of 31."""
    g = MAGS.astype(np.float32)
    mids = ((MAGS[1:] + MAGS[:-1]) / 2).astype(np.float32)
    pts = np.concatenate([g, mids])
    near = np.concatenate([np.nextafter(pts, np.float32(np.inf)), np.nextafter(pts[1:], np.float32(0))])
    small = np.ldexp(np.float32(1), -np.arange(1, 150)).astype(np.float32)
    small = np.concatenate([small, np.nextafter(small, np.float32(np.inf)), np.nextafter(small[:-1], np.float32(0)),
                            (1.5 * small).astype(np.float32)])
    rng = np.random.default_rng(6)
    rnd = np.concatenate([np.ldexp(rng.uniform(1, 2, 4096), k) for k in range(-12, 3)]).astype(np.float32)
    v = np.concatenate([pts, near, small, rnd])
    v = v[v <= np.float32(7.5)]
    v = np.concatenate([v, -v]).astype(np.float32)
    return np.concatenate([v, np.zeros(-v.size % 31, dtype=np.float32)])


def probe_blocks(v, e=0):
    """values v (count a multiple of 31) -> (B, 32) blocks of 31 values times 2^e and a last element 7.5 2^e that
    pins the scale: the block's scaled values are v itself."""
    b = np.concatenate([v.reshape(-1, 31), np.full((v.size // 31, 1), 7.5, dtype=np.float32)], axis=1)
    with np.errstate(all="ignore"):
        return np.ldexp(b.astype(np.float64), e).astype(np.float32)
