"""An independent reference of the `mxfp4_e2m1` wire format (docs/collectives.md "The `mxfp4_e2m1`
wire format"), for the tests only.

It shares no code with `ops.*_reference` or the kernels. Quantization is integer arithmetic on the
f32 bit patterns: |x| = mant 2^expo, the scaled magnitude is compared in quarter units against the
table of the eight e2m1 magnitudes, and the nearest code wins, the even one at a tie. Dequantization
is the table and `ldexp` in f64 (exact), rounded once to f32. torch appears only for the final cast
to the tensor's dtype.
"""
import numpy as np
import torch

BLOCK = 32
PAYLOAD = 16  # bytes per block: element 2j in the low nibble of byte j, element 2j + 1 in the high one
BLOCK_WIRE = PAYLOAD + 1
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
WIRE = "mxfp4_e2m1"
MAGS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])  # magnitudes of the codes 0..7
MAG4 = (MAGS * 4).astype(np.int64)                           # ... in quarter units: ties are integers too


def chunk_blocks(numel, world=1):
    per = -(-(-(-numel // BLOCK)) // world)  # ceil(ceil(numel / 32) / world)
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


def f32(t):
    """torch tensor of a supported dtype -> flat numpy f32 (exact widening)."""
    return t.detach().reshape(-1).to(torch.float32).numpy().copy()


# ------------------------------------------------------------------ blocks
def scale_exponent(amax_bits):
    """e of the contract from max |x| as f32 bits; 0 for an all-zero block."""
    a = amax_bits.astype(np.int64)
    e = (a >> 23) - 127 - 2 + ((a & 0x7FFFFF) > 0x400000)
    e = np.minimum(np.maximum(e, -125), 126)
    e[a == 0] = 0
    return e


def codes(xb):
    """(B, 32) f32 -> ((B, 32) e2m1 codes with the sign in bit 3, (B,) scale bytes, (B,) blank)."""
    xb = np.ascontiguousarray(xb, dtype=np.float32)
    bits = xb.view(np.uint32).astype(np.int64)
    mag, sign = bits & 0x7FFFFFFF, bits >> 31
    amax = mag.max(axis=1)
    special = amax >= 0x7F800000
    blank = special | (amax == 0)
    e = scale_exponent(amax)
    field, frac = mag >> 23, mag & 0x7FFFFF
    mant = np.where(field == 0, frac, frac | 0x800000)   # |x| = mant 2^expo
    expo = np.where(field == 0, 1, field) - 150
    # |x| 2^-e = mant 2^-ns. Finite blocks have |x| 2^-e <= 6, so ns >= 21; past 40 the value is below
    # 2^-14 and the answer is code 0 either way, so ns is capped to keep the shifts inside int64.
    ns = np.clip(e[:, None] - expo, 0, 40)
    dist = np.abs((mant * 4)[None] - (MAG4[:, None, None] << ns[None]))  # (8, B, 32), quarter units
    key = dist * 2 + (np.arange(8) & 1)[:, None, None]                    # a tie goes to the even code
    code = key.argmin(axis=0) | (sign << 3)
    code[blank] = 0
    s = (e + 127).astype(np.uint8)
    s[special] = 255
    return code.astype(np.uint8), s, blank


def q_blocks(xb):
    """(B, 32) f32 -> ((B, 16) uint8 payload, (B,) uint8 scale bytes)."""
    code, s, _ = codes(xb)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8), s


def unpack_codes(q):
    """(B, 16) payload -> (B, 32) codes."""
    q = np.asarray(q, dtype=np.uint8)
    return np.stack([q & 15, q >> 4], axis=2).reshape(q.shape[0], BLOCK)


def d_blocks(q, s):
    """(B, 16) payload and (B,) scale bytes -> (B, 32) f32."""
    c = unpack_codes(q).astype(np.int64)
    v = np.where(c & 8, -MAGS[c & 7], MAGS[c & 7])
    with np.errstate(all="ignore"):
        v = np.ldexp(v, (s.astype(np.int32) - 127)[:, None]).astype(np.float32)  # 4 2^126 and 6 2^126 -> inf
    v[s == 255] = np.nan
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


def quantize(x, world=1):
    """flat numpy f32 -> dealt wire (uint8 array) of `world` chunks, padding blocks included."""
    return join(*q_blocks(pad_blocks(x, chunk_blocks(x.size, world) * world)), world)


def dequantize(wire, numel, world=1, dtype=torch.float32):
    """dealt wire -> torch tensor of `numel` elements, rounded once to `dtype` (torch's CPU cast)."""
    assert len(wire) == wire_bytes(numel, world), (len(wire), numel, world)
    v = d_blocks(*split(wire, world)).reshape(-1)[:numel]
    return torch.from_numpy(v.copy()).to(dtype)


def quantize_shards(x, W):
    """flat numpy f32 of W * m elements -> shard wire: chunk r is shard r alone, blocks from its start."""
    assert x.size % W == 0 and x.size >= W, (x.size, W)
    m = x.size // W
    cb = shard_blocks(m)
    return np.concatenate([join(*q_blocks(pad_blocks(x[r * m:(r + 1) * m], cb)), 1) for r in range(W)])


def dequantize_shards(wire, m, W, dtype=torch.float32):
    """shard wire -> torch tensor of W * m elements, rounded once to `dtype`."""
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


def reduce(wire, nsrc, op="sum"):
    """`nsrc` chunk wires back to back -> one chunk wire (the fold, quantized again)."""
    return join(*q_blocks(fold_blocks(_sources(wire, nsrc), op)), 1)


def fold(wire, nsrc, numel, op="sum", dtype=torch.float32):
    """`nsrc` chunk wires of shard_blocks(numel) blocks -> `numel` elements, rounded once to `dtype`."""
    assert len(wire) == shard_wire_bytes(numel, nsrc), (len(wire), numel, nsrc)
    acc = fold_blocks(_sources(wire, nsrc), op)
    return torch.from_numpy(acc.reshape(-1)[:numel].copy()).to(dtype)


# ------------------------------------------------------------------ the collectives
def _dq(v):
    return d_blocks(*q_blocks(pad_blocks(v, -(-v.size // BLOCK))))


def all_reduce(xs, op="sum", dtype=torch.float32):
    """D(Q(fold_r D(Q(x_r)))) rounded once to `dtype`; blocks are independent of the chunking."""
    n = xs[0].numel()
    y = d_blocks(*q_blocks(fold_blocks([_dq(f32(x)) for x in xs], op))).reshape(-1)[:n]
    return torch.from_numpy(y.copy()).to(dtype)


def reduce_scatter(xs, rank, op="sum", dtype=torch.float32):
    """cast(fold_r D(Q(x_r[rank m:(rank + 1) m]))), blocks counted from the shard's start."""
    m = xs[0].numel() // len(xs)
    y = fold_blocks([_dq(f32(x)[rank * m:(rank + 1) * m]) for x in xs], op).reshape(-1)[:m]
    return torch.from_numpy(y.copy()).to(dtype)


def all_gather(shards, dtype=torch.float32):
    """cat_r cast(D(Q(x_r)))."""
    out = [_dq(f32(x)).reshape(-1)[:x.numel()] for x in shards]
    return torch.from_numpy(np.concatenate(out)).to(dtype)


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


# ------------------------------------------------------------------ the edge blocks
def _bits(u):
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)  # scaled values halfway between two codes


def edge_blocks():
    """{name: (32,) f32 block}: every branch of Q."""
    rng = np.random.default_rng(20250114)
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
    # the m = 1.5 switch of e: mantissa 0x400000 and one ulp to either side, over a few binades
    for j in (-100, -20, 0, 9, 100):
        base = 0x3FC00000 + (j << 23)  # 1.5 2^j
        block(_bits(base), f"amax_1.5_2^{j}")
        block(_bits(base + 1), f"amax_1.5_2^{j}_plus_ulp")
        block(_bits(base - 1), f"amax_1.5_2^{j}_minus_ulp")
    block(-_bits(0x3FC00001), "mant_400001_negative")
    # amax 6 -> e = 0, so the block is its own scaled value: every tie in both signs, values a hair to
    # either side of each, just below 0.25 in both signs (the signed zero codes), and both zeros
    t = np.array(TIES, dtype=np.float32)
    ties = np.concatenate([[6.0], t, -t, np.nextafter(t[:4], np.float32(0)), -np.nextafter(t[:4], np.float32(9)),
                           [0.2499, -0.2499, 1e-30, -1e-30, -0.0, 0.0, -6.0, 4.0, -3.0]]).astype(np.float32)
    assert ties.size == BLOCK, ties.size
    out["ties"] = ties
    with np.errstate(all="ignore"):
        out["ties_2^40"] = np.ldexp(ties.astype(np.float64), 40).astype(np.float32)
        out["ties_2^-60"] = np.ldexp(ties.astype(np.float64), -60).astype(np.float32)
    # the lower clamp: e = -125 whatever amax is below 2^-123
    block(np.float32(2.0 ** -120), "amax_2^-120")
    block(np.float32(2.0 ** -124), "amax_2^-124")
    block(np.float32(2.0 ** -126), "amax_2^-126")
    block(_bits(0x00000123), "amax_subnormal", fill=False)
    block(_bits(0x007FFFFF), "amax_largest_subnormal")
    # the top: e = 126 and a payload of 4 dequantizes to 2^128 = inf; 1.5 2^127 is the largest amax that
    # comes back finite
    block(_bits(0x7F7FFFFF), "amax_f32_max")
    block(_bits(0x7F400000), "amax_1.5_2^127")
    # the other dtypes' extremes: f16's largest and smallest values, bf16's largest
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
