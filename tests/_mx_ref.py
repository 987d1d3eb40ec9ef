"""An independent reference of the `mxfp8_e4m3` wire format (docs/collectives.md "Compressed
all-reduce"), for the tests only.

It shares no code with `ops.*_reference` or the kernels: everything is numpy integer arithmetic on
the bit patterns (`ldexp` moves exponents, exactly, in f64), and torch appears only as the f32 ->
float8_e4m3fn cast the contract names. Payload bytes are decoded by hand.
"""
import numpy as np
import torch

BLOCK = 32
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def chunk_blocks(numel, world=1):
    per = -(-(-(-numel // BLOCK)) // world)  # ceil(ceil(numel / 32) / world)
    cb = max(16, -(-per // 16) * 16)
    if cb * 33 >= 1048576:
        cb = -(-cb // 4096) * 4096
    return cb


def wire_bytes(numel, world=1):
    return 33 * chunk_blocks(numel, world) * world


def f32(t):
    """torch tensor of a supported dtype -> flat numpy f32 (exact widening)."""
    return t.detach().reshape(-1).to(torch.float32).numpy().copy()


# ------------------------------------------------------------------ blocks
def scale_exponent(amax_bits):
    """e of the contract from max |x| as f32 bits (uint32 array); 0 for an all-zero block."""
    a = amax_bits.astype(np.int64)
    e = (a >> 23) - 127 - 8 + ((a & 0x7FFFFF) > 0x600000)
    e = np.minimum(np.maximum(e, -117), 120)
    e[a == 0] = 0
    return e


def q_blocks(xb):
    """(B, 32) f32 -> ((B, 32) uint8 payload, (B,) uint8 scale bytes)."""
    xb = np.ascontiguousarray(xb, dtype=np.float32)
    amax = (xb.view(np.uint32) & np.uint32(0x7FFFFFFF)).max(axis=1)
    special = amax >= 0x7F800000
    blank = special | (amax == 0)
    e = scale_exponent(amax)
    with np.errstate(all="ignore"):
        # exact in f64; the one rounding to f32 is the f32 product's (it matters for subnormal
        # products only, and those all round to an FP8 zero)
        scaled = np.ldexp(xb.astype(np.float64), (-e)[:, None].astype(np.int32))
        scaled[blank] = 0.0
        s32 = scaled.astype(np.float32)
    q = torch.from_numpy(s32).to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
    q[blank] = 0
    s = (e + 127).astype(np.uint8)
    s[special] = 255
    return q, s


def decode_e4m3(q):
    """uint8 array -> f64 values of float8_e4m3fn (NaN for 0x7f / 0xff), decoded from the fields."""
    q = q.astype(np.int64)
    ex, man = (q >> 3) & 15, q & 7
    mag = np.where(ex == 0, np.ldexp(man.astype(np.float64), -9), np.ldexp((8 + man).astype(np.float64), ex - 10))
    mag = np.where((q & 0x7F) == 0x7F, np.nan, mag)
    return np.where(q & 0x80, -mag, mag)


def d_blocks(q, s):
    """(B, 32) payload and (B,) scale bytes -> (B, 32) f32."""
    with np.errstate(all="ignore"):
        v = np.ldexp(decode_e4m3(q), (s.astype(np.int32) - 127)[:, None]).astype(np.float32)
    v[s == 255] = np.nan
    return v


# ------------------------------------------------------------------ wires
def join(q, s, nchunks):
    cb = s.size // nchunks
    return np.concatenate([q.reshape(nchunks, 32 * cb), s.reshape(nchunks, cb)], axis=1).reshape(-1)


def split(wire, nchunks):
    wire = np.asarray(wire, dtype=np.uint8)
    assert wire.size % (33 * 16 * nchunks) == 0, (wire.size, nchunks)
    cb = wire.size // (33 * nchunks)
    w = wire.reshape(nchunks, 33 * cb)
    return w[:, :32 * cb].reshape(nchunks * cb, 32), w[:, 32 * cb:].reshape(nchunks * cb)


def pad_blocks(x, blocks):
    xb = np.zeros(blocks * BLOCK, dtype=np.float32)
    xb[:x.size] = x
    return xb.reshape(blocks, BLOCK)


def quantize(x, world=1):
    """flat numpy f32 -> wire (uint8 array) of `world` chunks, padding blocks included."""
    return join(*q_blocks(pad_blocks(x, chunk_blocks(x.size, world) * world)), world)


def dequantize(wire, numel, world=1, dtype=torch.float32):
    """wire -> torch tensor of `numel` elements, rounded once to `dtype` (torch's CPU cast)."""
    assert len(wire) == wire_bytes(numel, world), (len(wire), numel, world)
    v = d_blocks(*split(wire, world)).reshape(-1)[:numel]
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


def reduce(wire, nsrc, op="sum"):
    """`nsrc` chunk wires back to back -> one chunk wire."""
    q, s = split(wire, nsrc)
    cb = s.size // nsrc
    d = d_blocks(q, s).reshape(nsrc, cb, BLOCK)
    return join(*q_blocks(fold_blocks([d[r] for r in range(nsrc)], op)), 1)


def all_reduce(xs, op="sum", dtype=torch.float32):
    """What every rank holds after all_reduce_compressed of `xs` (one torch tensor per rank, rank
    order): D(Q(fold_r D(Q(x_r)))) rounded once to `dtype`. Blocks are independent, so the chunking
    does not enter."""
    n = xs[0].numel()
    blocks = -(-n // BLOCK)
    ds = [d_blocks(*q_blocks(pad_blocks(f32(x), blocks))) for x in xs]
    y = d_blocks(*q_blocks(fold_blocks(ds, op))).reshape(-1)[:n]
    return torch.from_numpy(y.copy()).to(dtype)


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


def edge_blocks():
    """{name: (32,) f32 block}: every branch of Q. Blocks hold small values around the one that
    sets amax, so ties, FP8 subnormals and underflow after scaling occur too."""
    rng = np.random.default_rng(20240607)
    out = {}

    def block(amax, name, fill=True):
        b = np.zeros(BLOCK, dtype=np.float32)
        if fill:
            with np.errstate(all="ignore"):
                b[:] = (rng.uniform(-1, 1, BLOCK) * np.float64(amax)).astype(np.float32)
        b[5] = amax
        out[name] = b

    out["zero"] = np.zeros(BLOCK, dtype=np.float32)
    pm = np.zeros(BLOCK, dtype=np.float32)
    pm[1::2] = -0.0
    out["pm_zero"] = pm
    for j in (-100, -20, 0, 7, 100):
        a = np.float32(np.ldexp(448.0, j))  # 448 2^j = 1.75 2^(j+8): mantissa 0x600000
        block(a, f"amax_448_2^{j}")
        block(np.nextafter(a, np.float32(np.inf), dtype=np.float32), f"amax_448_2^{j}_plus_ulp")
    block(_bits(0x3FE00000), "mant_600000")   # 1.75
    block(_bits(0x3FE00001), "mant_600001")
    block(-_bits(0x3FE00001), "mant_600001_negative")
    block(np.float32(2.0 ** -120), "amax_2^-120")
    block(np.float32(2.0 ** -126), "amax_2^-126")
    block(_bits(0x00000123), "amax_subnormal", fill=False)
    block(np.float32(3e38), "amax_3e38")
    nan = (rng.uniform(-4, 4, BLOCK)).astype(np.float32)
    nan[17] = np.nan
    out["one_nan"] = nan
    inf = (rng.uniform(-4, 4, BLOCK)).astype(np.float32)
    inf[3] = -np.inf
    out["one_inf"] = inf
    # scaled values at FP8 ties and in the FP8 subnormal range: amax 448 -> e = 0, so x is its own
    # scaled value. Ties between neighbours (x.5 steps), half the smallest subnormal (2^-10, a tie
    # to zero), just above and below it, the subnormals themselves, -0 next to a non-zero amax.
    ties = np.array([448, 17, 19, 21, 23, 25, 27, 29, 31, -17, -19, 2.0 ** -10, -(2.0 ** -10), 2.0 ** -10 * 1.0001,
                     2.0 ** -10 * 0.9999, 2.0 ** -9, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 7 * 2.0 ** -9, 2.0 ** -6,
                     -0.0, 0.0, 1.0625, 1.1875, 432, 416 + 16 - 1e-3, 2.0 ** -30, 2.0 ** -140, -(2.0 ** -149),
                     0.0146484375, 0.0166015625, 440], dtype=np.float32)
    assert ties.size == BLOCK
    out["ties_and_subnormals"] = ties
    with np.errstate(all="ignore"):
        out["ties_scaled_2^40"] = np.ldexp(ties.astype(np.float64), 40).astype(np.float32)
    return out


def random_binades(blocks, seed, lo=-40, hi=40):
    """(blocks, 32) f32: per-block magnitude 2^U[lo, hi], elements spread over a few binades below it."""
    rng = np.random.default_rng(seed)
    mag = np.ldexp(1.0, rng.integers(lo, hi + 1, size=(blocks, 1)))
    x = rng.standard_normal((blocks, BLOCK)) * mag * np.ldexp(1.0, -rng.integers(0, 12, size=(blocks, BLOCK)))
    return x.astype(np.float32)


def edge_tensor():
    """Every edge block and 96 random blocks over 80 binades, flat f32 (numpy), plus the names."""
    eb = edge_blocks()
    x = np.concatenate([np.stack(list(eb.values())), random_binades(96, 11)])
    return x.reshape(-1).copy(), list(eb)
