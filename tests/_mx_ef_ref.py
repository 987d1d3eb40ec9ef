"""An independent reference of error feedback on the block-scaled wires (docs/collectives.md "Error
feedback"), for the tests only.

`Q_ef` and the residual reduce are built here in numpy on top of the `Q` / `D` of tests/_mx_ref.py
(`mxfp8_e4m3`) and tests/_mx4_ref.py (`mxfp4_e2m1`); nothing is shared with `ops.*_reference` or the
kernels. A residual is a flat numpy f32 array; every function returns the new one instead of writing
into its argument, so a test can keep both.
"""
import numpy as np
import torch

from tests import _mx4_ref as R4
from tests import _mx_ref as R8

BLOCK = 32
WIRES = {"mxfp8_e4m3": R8, "mxfp4_e2m1": R4}
DTYPES = R8.DTYPES
# |r| <= A / (K - 1) * (1 + 2^-10) with K = 16 (FP8: a quantization errs by at most amax / 16) or 3 (FP4)
BOUND_DIV = {"mxfp8_e4m3": 15.0, "mxfp4_e2m1": 2.0}


def owner_numel(numel, world, wire):
    return BLOCK * WIRES[wire].chunk_blocks(numel, world)


def _shard_blocks(m, wire):
    return WIRES[wire].chunk_blocks(m, 1)


def _feed_back(v, d):
    """r' = v - d in f32 where that is finite, +0 elsewhere."""
    with np.errstate(all="ignore"):
        r = (v.astype(np.float32) - d.astype(np.float32)).astype(np.float32)
    return np.where(np.isfinite(r), r, np.float32(0)).astype(np.float32)


def q_ef_blocks(vb, wire):
    """(B, 32) f32 v -> (payload, scale bytes, (B, 32) new residual)."""
    R = WIRES[wire]
    q, s = R.q_blocks(vb)
    return q, s, _feed_back(vb, R.d_blocks(q, s))


def _add(x, r):
    with np.errstate(all="ignore"):
        return (x.astype(np.float32) + r.astype(np.float32)).astype(np.float32)


def quantize(x, r, world, wire):
    """flat f32 x and residual r (same size) -> (dealt wire of `world` chunks, new residual)."""
    R = WIRES[wire]
    n = x.size
    assert r.size == n and r.dtype == np.float32
    q, s, rb = q_ef_blocks(R.pad_blocks(_add(x, r), R.chunk_blocks(n, world) * world), wire)
    return R.join(q, s, world), rb.reshape(-1)[:n].copy()


def quantize_shards(x, r, W, wire):
    """flat f32 x of W * m elements and its residual -> (shard wire, new residual)."""
    R = WIRES[wire]
    assert x.size % W == 0 and x.size >= W and r.size == x.size
    m = x.size // W
    cb = _shard_blocks(m, wire)
    wires, rs = [], []
    for k in range(W):
        q, s, rb = q_ef_blocks(R.pad_blocks(_add(x[k * m:(k + 1) * m], r[k * m:(k + 1) * m]), cb), wire)
        wires.append(R.join(q, s, 1))
        rs.append(rb.reshape(-1)[:m])
    return np.concatenate(wires), np.concatenate(rs).astype(np.float32)


def reduce(wire_bytes, nsrc, op, r2, wire):
    """`nsrc` chunk wires back to back and the owner residual (32 cb) -> (one chunk wire, new residual)."""
    R = WIRES[wire]
    q, s = R.split(wire_bytes, nsrc)
    cb = s.size // nsrc
    assert r2.size == BLOCK * cb
    d = R.d_blocks(q, s).reshape(nsrc, cb, BLOCK)
    acc = _add(R.fold_blocks([d[k] for k in range(nsrc)], op), r2.reshape(cb, BLOCK))
    q, s, rb = q_ef_blocks(acc, wire)
    return R.join(q, s, 1), rb.reshape(-1).copy()


# ------------------------------------------------------------------ the collectives, one process
def all_reduce(xs, rs, r2s, op, wire, dtype=torch.float32):
    """One all_reduce_compressed call with error feedback. `xs`: one torch tensor per rank; `rs`: per rank
    the local residual (numpy, or None: no local feedback on any rank); `r2s`: per rank the owner residual
    (or None). Returns (result every rank holds, new rs, new r2s)."""
    R = WIRES[wire]
    W, n = len(xs), xs[0].numel()
    cb = R.chunk_blocks(n, W)
    wires, new_rs = [], []
    for k in range(W):
        x = R.f32(xs[k])
        if rs is None:
            wires.append(R.quantize(x, W))
        else:
            w, r = quantize(x, rs[k], W, wire)
            wires.append(w)
            new_rs.append(r)
    cbytes = wires[0].size // W
    chunks, new_r2s = [], []
    for k in range(W):  # owner k folds chunk k of every rank, in rank order
        recv = np.concatenate([w[k * cbytes:(k + 1) * cbytes] for w in wires])
        if r2s is None:
            chunks.append(R.reduce(recv, W, op))
        else:
            c, r2 = reduce(recv, W, op, r2s[k], wire)
            chunks.append(c)
            new_r2s.append(r2)
    assert cb * W * (cbytes // cb) == sum(c.size for c in chunks)
    return R.dequantize(np.concatenate(chunks), n, W, dtype), (None if rs is None else new_rs), \
        (None if r2s is None else new_r2s)


def reduce_scatter(xs, rs, op, wire, dtype=torch.float32):
    """One reduce_scatter_compressed call with error feedback: `xs` one tensor of W * m elements per rank,
    `rs` the local residuals. Returns ([rank k's output], new rs)."""
    R = WIRES[wire]
    W = len(xs)
    m = xs[0].numel() // W
    cb = _shard_blocks(m, wire)
    got = [quantize_shards(R.f32(xs[k]), rs[k], W, wire) for k in range(W)]
    cbytes = got[0][0].size // W
    outs = []
    for k in range(W):
        recv = np.concatenate([g[0][k * cbytes:(k + 1) * cbytes] for g in got])
        q, s = R.split(recv, W)
        d = R.d_blocks(q, s).reshape(W, cb, BLOCK)
        acc = R.fold_blocks([d[j] for j in range(W)], op)
        outs.append(torch.from_numpy(acc.reshape(-1)[:m].copy()).to(dtype))
    return outs, [g[1] for g in got]


# ------------------------------------------------------------------ comparisons and inputs
def same_residual(got, ref):
    """Equal as f32 values (+0 and -0 are not told apart), and finite."""
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float32).reshape(-1)
    ref = np.asarray(ref, dtype=np.float32).reshape(-1)
    return got.shape == ref.shape and bool(np.isfinite(got).all()) and bool((got == ref).all())


def random_residual(n, seed, scale=0.05):
    """A non-zero incoming residual: normal, a few binades below the data."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * scale).astype(np.float32)


def bound_series(kind, seed=20251021, n=16384, T=64):
    """The inputs of the bound / telescoping test: x_t = base on even t, base + 0.1 randn on odd t, with
    base normal or log-normal (randn * exp(2 randn)). Returns a (T, n) f32 array."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(n)
    if kind == "lognormal":
        base = base * np.exp(2.0 * rng.standard_normal(n))
    else:
        assert kind == "normal", kind
    xs = np.empty((T, n), dtype=np.float32)
    for t in range(T):
        xs[t] = (base if t % 2 == 0 else base + 0.1 * rng.standard_normal(n)).astype(np.float32)
    return xs


def check_bound(xs, step, wire):
    """Runs `step(x_t, use_residual) -> (sent_t, residual after the call or None)` (flat f32 numpy arrays)
    over the series with and without feedback and returns the three figures of the contract's bound, each as a
    fraction of the derived bound A_b / (K - 1) * (1 + 2^-10) per element, A_b the largest block amax of x
    seen so far: (a) the worst |r_t| after any call, (b) the worst |sum sent - sum x| at the end with feedback,
    (c) the same without. No element is left out."""
    T, n = xs.shape
    assert n % BLOCK == 0
    A = np.zeros(n // BLOCK, dtype=np.float64)
    sum_x = np.zeros(n, dtype=np.float64)
    sum_ef = np.zeros(n, dtype=np.float64)
    sum_plain = np.zeros(n, dtype=np.float64)
    worst_r = 0.0
    bound = None
    for t in range(T):
        x = xs[t]
        A = np.maximum(A, np.abs(x.astype(np.float64)).reshape(-1, BLOCK).max(axis=1))
        assert (A >= 2.0 ** -100).all()
        bound = np.repeat(A / BOUND_DIV[wire] * (1 + 2.0 ** -10), BLOCK)
        sent, r = step(x, True)
        plain, _ = step(x, False)
        assert np.isfinite(r).all() and np.isfinite(sent).all()
        worst_r = max(worst_r, float((np.abs(r.astype(np.float64)) / bound).max()))
        sum_x += x.astype(np.float64)
        sum_ef += sent.astype(np.float64)
        sum_plain += plain.astype(np.float64)
    return worst_r, float((np.abs(sum_ef - sum_x) / bound).max()), float((np.abs(sum_plain - sum_x) / bound).max())
