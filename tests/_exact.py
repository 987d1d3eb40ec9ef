"""The exact-value reference of every reduction test, and the inputs those tests use. CPU only.

One contract per dtype class (docs/collectives.md), sources always combined in list order (rank order):

* float16 / bfloat16 / FP8: every element widened to fp32, folded in fp32, AVG divided by W in fp32, the
  result rounded once by torch's CPU cast (nearest even, subnormals kept, no saturation). MIN / MAX compare
  in fp32 the way `dev::apply_op` does: `(a > b or a is NaN) ? a : b`, so a NaN in any source wins;
* float32 / float64: the same fold in the dtype's own precision, AVG = folded sum / W in that precision;
* int8 / uint8 / int16 / int32 / int64: integer arithmetic only. SUM / PRODUCT wrap (two's complement at the
  element width), AVG is the *wrapped* sum divided by W truncating toward zero, MIN / MAX use the dtype's own
  signedness, BAND / BOR / BXOR are bitwise;
* bool: SUM = MAX = BOR = or, PRODUCT = MIN = BAND = and, BXOR = xor, result bytes exactly 0 / 1; AVG raises.

`fold` shares no code with the kernels or the host reduction: torch CPU arithmetic for floats, numpy
`uint64` arithmetic masked to the element width for integers.
"""
import functools

import numpy as np
import torch

NARROW = {"float16": torch.float16, "bfloat16": torch.bfloat16,
          "float8_e4m3fn": torch.float8_e4m3fn, "float8_e5m2": torch.float8_e5m2}
WIDE = {"float32": torch.float32, "float64": torch.float64}
INTS = {"int8": torch.int8, "uint8": torch.uint8, "int16": torch.int16, "int32": torch.int32,
        "int64": torch.int64}
DTYPES = {**NARROW, **WIDE, **INTS, "bool": torch.bool}
_NAME = {v: k for k, v in DTYPES.items()}

FLOAT_OPS = ("SUM", "AVG", "PRODUCT", "MIN", "MAX")
INT_OPS = FLOAT_OPS + ("BAND", "BOR", "BXOR")
BOOL_OPS = tuple(op for op in INT_OPS if op != "AVG")
# the spelling of ops.reduce_nway
K1_OP = {"SUM": "sum", "AVG": "avg", "PRODUCT": "prod", "MIN": "min", "MAX": "max", "BAND": "band",
         "BOR": "bor", "BXOR": "bxor"}


def ops_for(dt):
    if dt == torch.bool:
        return BOOL_OPS
    return FLOAT_OPS if dt.is_floating_point else INT_OPS


# ---------------------------------------------------------------------------------------------- fold
def _fold_float(xs, op, dt):
    acc_dt = dt if dt in (torch.float32, torch.float64) else torch.float32
    acc = xs[0].to(acc_dt)
    for x in xs[1:]:
        s = x.to(acc_dt)
        if op in ("SUM", "AVG"):
            acc = acc + s
        elif op == "PRODUCT":
            acc = acc * s
        elif op == "MAX":
            acc = torch.where((acc > s) | acc.isnan(), acc, s)
        elif op == "MIN":
            acc = torch.where((acc < s) | acc.isnan(), acc, s)
        else:
            raise ValueError(f"{op} on {dt}")
    if op == "AVG":
        acc = acc / torch.tensor(float(len(xs)), dtype=acc_dt)
    assert acc.dtype == acc_dt
    return acc.to(dt)


def _fold_int(xs, op, dt):
    sdt = np.dtype(_NAME[dt])                      # the element type
    udt = np.dtype(f"uint{8 * sdt.itemsize}")      # its bit pattern
    mask = np.uint64((1 << (8 * sdt.itemsize)) - 1) if sdt.itemsize < 8 else np.uint64(0xFFFFFFFFFFFFFFFF)
    arrs = [np.ascontiguousarray(x.numpy()) for x in xs]
    assert all(a.dtype == sdt for a in arrs)
    if op in ("SUM", "AVG", "PRODUCT"):
        acc = arrs[0].view(udt).astype(np.uint64)
        for a in arrs[1:]:
            s = a.view(udt).astype(np.uint64)
            with np.errstate(over="ignore"):
                acc = ((acc + s) if op != "PRODUCT" else (acc * s)) & mask  # uint64 wraps; the mask wraps narrower types
        res = acc.astype(udt).view(sdt)
        if op == "AVG":
            w = sdt.type(len(xs))
            q = res // w                                   # floors ...
            q = q + ((res % w != 0) & (res < 0)).astype(sdt)   # ... so negative inexact quotients move up to truncation
            res = q.astype(sdt)
    elif op in ("MIN", "MAX"):
        acc = arrs[0]
        for a in arrs[1:]:
            acc = np.maximum(acc, a) if op == "MAX" else np.minimum(acc, a)
        res = acc
    elif op in ("BAND", "BOR", "BXOR"):
        f = {"BAND": np.bitwise_and, "BOR": np.bitwise_or, "BXOR": np.bitwise_xor}[op]
        acc = arrs[0]
        for a in arrs[1:]:
            acc = f(acc, a)
        res = acc
    else:
        raise ValueError(f"{op} on {dt}")
    assert res.dtype == sdt
    return torch.from_numpy(np.ascontiguousarray(res).copy())


def _fold_bool(xs, op):
    if op not in BOOL_OPS:
        raise ValueError(f"{op} on bool")
    arrs = [x.numpy() for x in xs]
    assert all(a.dtype == np.bool_ for a in arrs)
    f = (np.logical_or if op in ("SUM", "MAX", "BOR") else
         np.logical_and if op in ("PRODUCT", "MIN", "BAND") else np.logical_xor)
    acc = arrs[0].copy()
    for a in arrs[1:]:
        acc = f(acc, a)
    return torch.from_numpy(acc)


def fold(xs, op, dt):
    """The reference: `op` over the CPU tensors `xs` of dtype `dt`, in list order."""
    assert all(x.dtype == dt and x.device.type == "cpu" for x in xs), (dt, [x.dtype for x in xs])
    if dt == torch.bool:
        return _fold_bool(xs, op)
    if dt.is_floating_point:
        return _fold_float(xs, op, dt)
    return _fold_int(xs, op, dt)


def same(got, ref):
    """Equal as values. Floats: ±0 and the NaN encodings do not matter, NaN positions do (compared in fp64,
    which holds every value of every float dtype here). Integers: torch.equal. bool: the bytes are equal,
    so a "true" stored as anything but 1 differs."""
    g, r = got.detach().cpu(), ref.detach().cpu()
    if g.dtype != r.dtype or g.shape != r.shape:
        return False
    if g.dtype == torch.bool:
        return bool(torch.equal(g.contiguous().view(torch.uint8), r.contiguous().view(torch.uint8)))
    if not g.dtype.is_floating_point:
        return bool(torch.equal(g, r))
    g, r = g.double(), r.double()
    return bool(((g == r) | (g.isnan() & r.isnan())).all())


def mismatch(got, ref, srcs, k=6):
    """(count, the first k (index, inputs, got, want)) for a failure message."""
    g, r = got.detach().cpu().reshape(-1), ref.reshape(-1)
    if g.dtype == torch.bool:
        g, r = g.view(torch.uint8), r.view(torch.uint8)
    conv = (lambda t: t.double()) if g.dtype.is_floating_point else (lambda t: t)
    gd, rd = conv(g), conv(r)
    bad = ~((gd == rd) | ((gd != gd) & (rd != rd)))
    idx = bad.nonzero().flatten()[:k].tolist()
    ss = [conv(s.reshape(-1).view(torch.uint8) if s.dtype == torch.bool else s.reshape(-1)) for s in srcs]
    return int(bad.sum()), [(i, [s[i].item() for s in ss], gd[i].item(), rd[i].item()) for i in idx]


# ------------------------------------------------------------------------------------ input builders
def random_bits(n, dt, seed):
    """n elements of full-range random bit patterns (bool: random 0 / 1). For floats that is every class
    of value: NaNs, infinities, subnormals, both zeros."""
    rng = np.random.default_rng(seed)
    if dt == torch.bool:
        return torch.from_numpy(rng.integers(0, 2, size=n, dtype=np.uint8).astype(np.bool_))
    es = torch.empty(0, dtype=dt).element_size()
    raw = torch.from_numpy(rng.integers(0, 256, size=n * es, dtype=np.uint8))
    return raw.view(dt).clone()


def random_values(n, dt, seed, lo=-4.0, hi=4.0):
    """Seeded finite floats in [lo, hi], rounded to dt."""
    g = torch.Generator().manual_seed(seed)
    x = lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)
    return x.to(torch.float32).to(dt) if dt in NARROW.values() else x.to(dt)


@functools.lru_cache(maxsize=None)
def byte_pairs(dtn):
    """All 65 536 pairs of an 8-bit dtype: a[i] = byte(i >> 8), b[i] = byte(i & 255) (16 tiles)."""
    dt = DTYPES[dtn]
    i = torch.arange(65536, dtype=torch.int32)
    return (i >> 8).to(torch.uint8).view(dt).clone(), (i & 255).to(torch.uint8).view(dt).clone()


def int_edges(dtn):
    """The edge values of a signed integer dtype (python ints)."""
    bits = 8 * np.dtype(dtn).itemsize
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    e = [0, 1, -1, 2, -2, lo, lo + 1, hi, hi - 1, 3, -3, lo // 2, hi // 2 + 1]
    if bits == 64:
        e += [0xFFFFFFFF, 0x1_0000_0000, -0x1_0000_0000, 0x7FFFFFFF_00000000, 0x00000000_80000000,
              # pairs that differ only in the low dword, one of them with its bit 31 set: a compare of
              # signed low dwords, or of the high dwords alone, orders them wrongly or not at all
              0x12345678_80000000, 0x12345678_7FFFFFFF, 0x12345678_00000001, 0x12345678_FFFFFFFF,
              -0x12345678_80000000, -0x12345678_7FFFFFFF - 0x1_0000_0000, -0x12345679_00000000 + 1,
              # ... and pairs that differ only in the high dword
              0x00000001_00000005, -0x00000001_00000000 + 5, 0x7FFFFFFF_FFFFFFFF - 0xFFFFFFFF]
    if bits == 32:
        e += [0xFFFF, 0x1_0000, -0x1_0000, 0x7FFF_0000, 0x0000_8000, 46341, -46341, 65536 + 1]
    return e


@functools.lru_cache(maxsize=None)
def int_pairs(dtn, seed=1234):
    """int16 / int32 / int64: the all-pairs square of `int_edges`, repeated to two 4-KiB tiles plus a ragged
    tail of 5 elements, followed by 4096 + 3 full-range random elements. Returns (a, b)."""
    dt = DTYPES[dtn]
    e = torch.tensor(int_edges(dtn), dtype=torch.int64).to(dt)
    assert e.to(torch.int64).tolist() == int_edges(dtn)
    m = len(e)
    ea, eb = e.repeat_interleave(m), e.repeat(m)
    n = max(2 * 4096 // e.element_size() + 5, m * m)
    idx = torch.arange(n) % (m * m)
    ra, rb = random_bits(4099, dt, seed), random_bits(4099, dt, seed + 1)
    return torch.cat([ea[idx], ra]), torch.cat([eb[idx], rb])


NARROW_PARTNERS = ("+0", "-0", "min_subnormal", "1", "max", "inf", "nan", "a*h", "a*h/2", "a*3h/2",
                   "p(a)*h", "p(a)*h/2", "p(a)*3h/2")


@functools.lru_cache(maxsize=None)
def narrow_pairs(dtn):
    """float16 / bfloat16: source `a` is every one of the 65 536 encodings, once per partner row; partner `b`
    is, row by row (NARROW_PARTNERS): ±0, the smallest subnormal, 1, the largest finite value, inf, NaN,
    then three partners scaled from a, then three scaled from p(a). h is half an ulp of 1 in dt (2^-8 for
    bfloat16, 2^-11 for float16) and p(a) is a with its mantissa bits cleared: the power of two at or below
    |a|, signed. a + p(a)·h lies exactly on a rounding tie for every normal a (both parities of the kept
    mantissa), a + p(a)·h/2 a quarter ulp above a (rounds back to a) and a + p(a)·3h/2 three quarters
    (rounds away). The partners scaled from a itself (a·h, a·h/2, a·3h/2, each rounded to dt) land on a tie
    only where a is a power of two, and elsewhere at every other distance from one.
    Returns (a, b), 13 x 65536 elements each."""
    dt = DTYPES[dtn]
    assert dt in (torch.float16, torch.bfloat16)
    a = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt)
    af = a.float()
    fi = torch.finfo(dt)
    h = fi.eps / 2
    pa = (af.view(torch.int32) & -0x00800000).view(torch.float32)  # sign and exponent kept: NaN becomes inf
    const = lambda v: torch.full((65536,), v, dtype=torch.float32)  # noqa: E731
    rows = [const(0.0), const(-0.0), const(fi.smallest_normal * fi.eps), const(1.0), const(fi.max),
            const(float("inf")), const(float("nan")), af * h, af * (h / 2), af * (3 * h / 2),
            pa * h, pa * (h / 2), pa * (3 * h / 2)]
    assert len(rows) == len(NARROW_PARTNERS)
    b = torch.cat([r.to(dt) for r in rows])
    return a.repeat(len(rows)).clone(), b


def float_edges(dt):
    fi = torch.finfo(dt)
    sub = fi.smallest_normal * fi.eps        # the smallest subnormal
    big_sub = fi.smallest_normal - sub       # the largest one
    inf, nan = float("inf"), float("nan")
    return [0.0, -0.0, sub, -sub, big_sub, -big_sub, 3 * sub, fi.smallest_normal, -fi.smallest_normal, 0.5, 1.0,
            -1.0, 1.0 + fi.eps, 1.5, fi.eps, fi.max, -fi.max, fi.max / 2, inf, -inf, nan]


@functools.lru_cache(maxsize=None)
def wide_pairs(dtn, seed=99):
    """float32 / float64: the all-pairs square of `float_edges` (±0, subnormals, the largest finite value --
    SUM and PRODUCT overflow --, ±inf, inf + -inf, NaN in either position), repeated to two 4-KiB tiles plus
    a ragged tail of 5, followed by 4096 + 3 random values in [-4, 4]. Returns (a, b)."""
    dt = DTYPES[dtn]
    e = torch.tensor(float_edges(dt), dtype=dt)
    m = len(e)
    ea, eb = e.repeat_interleave(m), e.repeat(m)
    n = max(2 * 4096 // e.element_size() + 5, m * m)
    idx = torch.arange(n) % (m * m)
    return (torch.cat([ea[idx], random_values(4099, dt, seed)]),
            torch.cat([eb[idx], random_values(4099, dt, seed + 1)]))


def mixed_magnitudes(n, dt, nsrc, seed):
    """nsrc float sources of mixed magnitude and sign whose sum, folded in the accumulator's precision and
    cast to dt, depends on the order of the additions (tests/test_exact_cpu.py counts the elements in which
    the reversed fold and a pairwise tree differ from the fold in list order).

    float32 / float64: magnitudes up to 2^12 apart from source to source; nearly every partial sum rounds.

    float16 / bfloat16: the values carry 11 / 8 mantissa bits, so fp32 partial sums of sources that close
    together are exact and no order can show. Here some sources are big (B in 2^E·[1, 2), random sign, E = 22
    for bfloat16 and 14 for float16, where fp32 has an ulp of 2^(E-23)) and each is cancelled by its exact
    negative later in the list; the others are small, up to 8 such ulps. A small value added while a big one
    is in the accumulator keeps 3 or 4 of its bits, one added before or after keeps them all, and once the
    big ones have cancelled the difference is far above an ulp of the narrow result."""
    if dt in WIDE.values():
        scale = [1.0, 2.0 ** -7, 2.0 ** 5, 2.0 ** -3, 2.0 ** 4, 2.0 ** -9, 2.0 ** 2, 2.0 ** -5]
        return [random_values(n, dt, seed + 17 * k, -scale[k % 8], scale[k % 8]) for k in range(nsrc)]
    assert dt in (torch.float16, torch.bfloat16) and nsrc >= 3
    big = 2.0 ** (22 if dt == torch.bfloat16 else 14)
    small = big * 2.0 ** -20
    # s marks a small source, +k / -k a big one and its negative
    layout = {3: "s +1 -1", 4: "s +1 s -1", 5: "s +1 s -1 s", 6: "s +1 s -1 +2 -2", 7: "s +1 s -1 +2 s -2",
              8: "s +1 s -1 +2 s -2 s"}[nsrc].split()
    g = torch.Generator().manual_seed(seed + 5)
    bigs = {}
    xs = []
    for k, what in enumerate(layout):
        if what == "s":
            xs.append(random_values(n, dt, seed + 17 * k, -small, small))
        elif what[0] == "+":
            sign = torch.randint(0, 2, (n,), generator=g).to(torch.float64) * 2 - 1
            bigs[what[1:]] = (sign * random_values(n, torch.float64, seed + 17 * k, big, 2 * big)).float().to(dt)
            xs.append(bigs[what[1:]])
        else:
            xs.append(-bigs[what[1:]])
    return xs


def collective_inputs(n, dt, seed, world, lo=-4.0, hi=4.0):
    """Every rank's CPU input for a collective of n elements, the same on whichever rank builds it.
    Integers and bool: full-range random bits. Floats: seeded values in [lo, hi] with specials at the head
    and at the tail: NaN on one rank (head: rank 0, tail: the last rank), the largest finite value on every
    rank (SUM overflows), inf on one rank (head: the last rank, tail: rank 0)."""
    xs = []
    for r in range(world):
        if not dt.is_floating_point:
            xs.append(random_bits(n, dt, seed + 31 * r))
            continue
        x = random_values(n, torch.float64, seed + 31 * r, lo, hi)
        big = torch.finfo(dt).max
        if n > 1:
            x[1] = big
        if n > 2 and r == world - 1:
            x[2] = float("inf")
        if n >= 8:
            x[n - 2] = big
            if r == 0:
                x[n - 3] = float("inf")
            if r == world - 1:
                x[n - 1] = float("nan")
        if r == 0:
            x[0] = float("nan")
        xs.append(x.to(torch.float32).to(dt) if dt in NARROW.values() else x.to(dt))
    return xs


# ------------------------------------------------------------------------------------------ guard bands
def pattern(nbytes, salt=0):
    """A position-dependent byte pattern (a multiplicative hash of the byte's index: a copy shifted by any
    vector, tile or row offset differs from it nearly everywhere)."""
    h = ((torch.arange(nbytes, dtype=torch.int64) + salt + 1) * 0x9E3779B1) & 0xFFFFFFFF
    return (((h >> 24) ^ (h >> 11)) & 0xFF).to(torch.uint8)
