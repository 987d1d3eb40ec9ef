"""The block-scaled FP6 wire format `mxfp6_e2m3` on the GPU: the kernels (dealt and shard layout, reduce,
fold; nearest, error feedback, stochastic), the three collectives, the bucketer and the sharded optimizer
(docs/collectives.md "The `mxfp6_e2m3` wire format").

The reference is always tests/_mx6_ref.py (a float64 table on the CPU), never a GPU cast: wires must equal it
byte for byte (the payload under a NaN block, scale 255, is unspecified), values exactly -- rtol = atol = 0,
NaN where the reference has NaN. The sizes are the ones at which the lanes that share three payload dwords
(a quad for f32, a pair for bf16 / f16) can go wrong: ragged ends inside a quad, whole padding chunks, more
than one workgroup, and one chunk past the 1 MiB rule.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _mx6_ref as R
from tests import _workers_mx as M8
from tests import _workers_mx6 as M
from tests._workers_mx_shard import shard_inputs
from tests.test_backend_gpu import _gpu_launch

pytestmark = pytest.mark.gpu

W6 = R.WIRE
SR = dict(rounding="stochastic")
NUMELS = (1, 31, 32, 33, 63, 65, 255, 257, 511, 513, 4095, 4097, 4113, 65553)
# 64, 96 and 4096 start every shard 16-byte aligned in every dtype (the vector path); the others do not
SHARDS = (1, 5, 31, 33, 64, 96, 511, 513, 4096, 4113)
WORLDS = (1, 3, 8)
BIG = 45056 * 32 - 7  # cb = 45056: the first multiple of 4096 past the 1 MiB threshold (41952 blocks)


def _ops():
    from pytorch_distributed_collective_communication_amd import ops

    return ops


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _inputs(dtn):
    """[(name, CPU tensor of dtype dtn)]: the edge blocks, then every ragged size."""
    dt = R.DTYPES[dtn]
    out = [("edge", torch.from_numpy(R.edge_tensor()[0]).to(dt))]
    out += [(f"n{n}", M8.rank_inputs(n, 2, 600 + n, dt)[1]) for n in NUMELS]
    return out


@functools.lru_cache(maxsize=None)
def _ref_wire(dtn, name, world):
    return R.quantize(R.f32(dict(_inputs(dtn))[name]), world)


@functools.lru_cache(maxsize=None)
def _shard_inputs(dtn, W):
    dt = R.DTYPES[dtn]
    out = [(f"m{m}", shard_inputs(m, max(W, 2), 600 + m, dt)[1][:W * m].clone(), m) for m in SHARDS]
    edge = torch.from_numpy(R.edge_tensor()[0])
    m = edge.numel()
    x = shard_inputs(m, max(W, 2), 7)[0][:W * m].clone()
    x[(W - 1) * m:] = edge
    out.append(("edge", x.to(dt), m))
    return out


@functools.lru_cache(maxsize=None)
def _ref_shard_wire(dtn, W, name):
    x = {n: t for n, t, _ in _shard_inputs(dtn, W)}[name]
    return R.quantize_shards(R.f32(x), W)


def _assert_wire(got, ref, nchunks, what):
    got = got.cpu().numpy()
    if not R.same_wire(got, ref, nchunks):
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        gq, gs = R.split(got, nchunks)
        rq, rs = R.split(ref, nchunks)
        bad = np.nonzero((gs != rs) | ((gq != rq).any(axis=1) & (rs != 255)))[0]
        first = [(int(b), int(gs[b]), int(rs[b]), R.unpack_codes(gq[b:b + 1])[0].tolist(),
                  R.unpack_codes(rq[b:b + 1])[0].tolist()) for b in bad[:2]]
        pytest.fail(f"{what}: {len(bad)} blocks differ; (block, s, want s, codes, want codes): {first}")


def _same_bits(got, want):
    """Values equal, NaN where the reference has NaN, and for float32 and bfloat16 every zero with the reference's
    sign. (The contract compares values. In the float16 output path of every wire the compiler fuses the product
    with the scale and the conversion into x * s + 0, v_fma_mixlo_f16, which gives +0 for a -0 code.)"""
    signs = got.dtype != torch.float16
    got, want = got.detach().cpu().to(torch.float32), want.detach().cpu().to(torch.float32)
    return R.same(got, want) and (not signs or bool((torch.signbit(got) == torch.signbit(want))[~want.isnan()].all()))


# ------------------------------------------------------------------ quantize / dequantize, dealt layout
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("dtn", list(R.DTYPES))
def test_quantize(dtn, world):
    ops = _ops()
    for name, x in _inputs(dtn):
        ref = _ref_wire(dtn, name, world)
        got = ops.mx_quantize(x.to(_dev()), world, wire=W6)
        assert got.dtype == torch.uint8 and got.numel() == ops.mx_wire_bytes(x.numel(), world, wire=W6) == ref.size
        _assert_wire(got, ref, world, f"{dtn} {name} world={world}")


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("dtn", list(R.DTYPES))
def test_dequantize(dtn, world):
    # (dtn: the dtype the wire was quantized from; every output dtype is checked)
    ops = _ops()
    for name, x in _inputs(dtn):
        ref = _ref_wire(dtn, name, world)
        w = torch.from_numpy(ref).to(_dev())
        for odt in R.DTYPES.values():
            got = ops.mx_dequantize(w, x.numel(), odt, world, wire=W6)
            assert got.dtype == odt and got.numel() == x.numel()
            assert R.same(got, R.dequantize(ref, x.numel(), world, odt)), (dtn, name, world, odt)


def test_a_chunk_past_the_1_mib_rule():
    ops = _ops()
    assert ops.mx_chunk_blocks(BIG, 1, wire=W6) == 45056 == R.chunk_blocks(BIG, 1)
    x = torch.from_numpy(R.random_binades(BIG // 32 + 1, 3, -10, 10).reshape(-1)[:BIG].copy())
    ref = R.quantize(R.f32(x), 1)
    _assert_wire(ops.mx_quantize(x.to(_dev()), 1, wire=W6), ref, 1, "big")
    got = ops.mx_dequantize(torch.from_numpy(ref).to(_dev()), BIG, torch.float32, 1, wire=W6)
    assert R.same(got, R.dequantize(ref, BIG, 1))


# ------------------------------------------------------------------ every code in every position
@pytest.mark.parametrize("dtn", list(R.DTYPES))
def test_position_sweep(dtn):
    """Blocks in which element j holds grid code (j + shift) % 32, all 32 shifts and both signs, the amax pinned
    to 7.5 2^e: every code passes through every bit position, dword boundaries included; through quantize,
    dequantize, reduce and fold."""
    ops = _ops()
    dt = R.DTYPES[dtn]
    for e in ((0, -20, 30, -123, 126 - 3) if dtn == "float32" else (0, -9 if dtn == "float16" else -20)):
        x = R.position_sweep(e)
        xt = torch.from_numpy(x.reshape(-1).copy()).to(dt)
        assert np.array_equal(R.f32(xt), x.reshape(-1))  # the grid values survive the dtype
        ref = R.quantize(x.reshape(-1), 1)
        q, s = R.split(ref, 1)
        assert (s[:64] == 127 + e).all()
        codes = R.unpack_codes(q[:64])
        for j in range(32):  # every position sees every code, both signs
            assert sorted(codes[:32, j].tolist()) == list(range(32)) and sorted(codes[32:, j].tolist()) == list(range(32, 64))
        _assert_wire(ops.mx_quantize(xt.to(_dev()), 1, wire=W6), ref, 1, f"{dtn} e={e}")
        w = torch.from_numpy(ref).to(_dev())
        got = ops.mx_dequantize(w, x.size, dt, 1, wire=W6)
        assert _same_bits(got, xt), (dtn, e)
        _assert_wire(ops.mx_reduce(w, 1, "sum", wire=W6), R.reduce(ref, 1, "sum"), 1, f"reduce {dtn} e={e}")
        assert np.array_equal(R.reduce(ref, 1, "sum"), ref)
        assert _same_bits(ops.mx_fold(w, 1, x.size, dt, "sum", wire=W6), xt), (dtn, e)
        both = torch.from_numpy(np.concatenate([ref, ref])).to(_dev())  # x + x: the same codes one binade up
        if e < 120:
            two = R.reduce(np.concatenate([ref, ref]), 2, "sum")
            assert np.array_equal(R.split(two, 1)[0], q) and (R.split(two, 1)[1][:64] == 128 + e).all()
            _assert_wire(ops.mx_reduce(both, 2, "sum", wire=W6), two, 1, f"reduce 2 {dtn} e={e}")
            assert R.same(ops.mx_fold(both, 2, x.size, torch.float32, "avg", wire=W6), torch.from_numpy(x.reshape(-1)))


@pytest.mark.parametrize("dtn", list(R.DTYPES))
def test_every_payload_pattern_dequantizes_to_its_table_value(dtn):
    # each of the 64 codes in each of the 32 positions, the neighbours filled with other codes; a few scales,
    # the lower clamp (4), the inf edge (253) and NaN (255) among them
    ops = _ops()
    dt = R.DTYPES[dtn]
    c, p, j = np.meshgrid(np.arange(64), np.arange(32), np.arange(32), indexing="ij")
    code = ((c + 17 * (j - p)) % 64).reshape(2048, 32).astype(np.uint8)
    for k in range(64):
        for pos in range(32):
            assert code[k * 32 + pos, pos] == k
    q = R.pack_codes(code)
    for s in (4, 100, 127, 200, 252, 253, 255):
        wire = R.join(q, np.full(2048, s, dtype=np.uint8), 1)
        got = ops.mx_dequantize(torch.from_numpy(wire).to(_dev()), 2048 * 32, dt, 1, wire=W6)
        want = R.dequantize(wire, 2048 * 32, 1, dt)
        assert R.same(got, want), s
        assert s == 255 or _same_bits(got, want), s  # -0 stays -0
        if s == 253:
            assert bool(want.isinf().any()) and bool(want.isfinite().any())
        wires = torch.from_numpy(np.concatenate([wire, wire])).to(_dev())
        assert R.same(ops.mx_dequantize_shards(wires, 2048 * 32, dt, 2, wire=W6), torch.cat([want, want])), s
        assert R.same(ops.mx_fold(wires[:wire.size], 1, 2048 * 32, dt, "sum", wire=W6), want), s


# ------------------------------------------------------------------ exhaustive rounding
@functools.lru_cache(maxsize=None)
def _probe(e):
    return R.probe_blocks(R.rounding_probe(), e).reshape(-1)


@pytest.mark.parametrize("e", [0, -123, 100, 125])
def test_exhaustive_rounding(e):
    """Every grid point, every midpoint and the f32 neighbours of both, small values down to f32 subnormals and
    4096 random values per binade from 2^-12 up, both signs, as the scaled values of blocks whose amax is pinned to
    7.5 2^e: nearest, and stochastic under 8 seeds; through the quantize lanes (f32: quads, 4 elements a lane) and,
    by way of a residual added to a zero wire, through the reduce lane (32 elements a lane). This is the gate of
    whatever convert path the kernels use."""
    ops = _ops()
    x = _probe(e)
    assert x.size > 120000
    xt = torch.from_numpy(x).to(_dev())
    ref = R.quantize(x, 1)
    _assert_wire(ops.mx_quantize(xt, 1, wire=W6), ref, 1, f"nearest e={e}")
    for seed in range(8):
        want = R.quantize(x, 1, (seed, 1, 0))
        _assert_wire(ops.mx_quantize(xt, 1, wire=W6, seed=seed, stream=1, **SR), want, 1, f"stochastic e={e} seed={seed}")
        assert seed or not np.array_equal(want, ref)
    # the reduce lane: one source of zero blocks, the values come in as the owner residual
    cb = R.chunk_blocks(x.size, 1)
    zero = R.quantize(np.zeros(x.size, dtype=np.float32), 1)
    r2 = np.zeros(32 * cb, dtype=np.float32)
    r2[:x.size] = x
    want_w, want_r = R.reduce_ef(zero, 1, "sum", r2)
    assert np.array_equal(R.d_blocks(*R.split(want_w, 1)), R.d_blocks(*R.split(ref, 1)))  # (0 + -0 is +0)
    res = torch.from_numpy(r2.copy()).to(_dev())
    _assert_wire(ops.mx_reduce(torch.from_numpy(zero).to(_dev()), 1, "sum", wire=W6, residual=res), want_w, 1, f"reduce e={e}")
    assert R.same_residual(res, want_r), e


@pytest.mark.parametrize("dtn", ["bfloat16", "float16"])
def test_rounding_of_the_16_bit_lanes(dtn):
    # the pair lanes (8 elements a lane): every bf16 / f16 value among the probe's, nearest and stochastic
    ops = _ops()
    dt = R.DTYPES[dtn]
    xt = torch.from_numpy(_probe(0)).to(dt)
    x = R.f32(xt)
    assert np.unique(x).size > 3000
    _assert_wire(ops.mx_quantize(xt.to(_dev()), 1, wire=W6), R.quantize(x, 1), 1, dtn)
    for seed in (0, 5):
        _assert_wire(ops.mx_quantize(xt.to(_dev()), 1, wire=W6, seed=seed, **SR), R.quantize(x, 1, (seed, 0, 0)), 1,
                     f"{dtn} seed={seed}")


# ------------------------------------------------------------------ the shard layout
@pytest.mark.parametrize("W", WORLDS)
@pytest.mark.parametrize("dtn", list(R.DTYPES))
def test_quantize_shards(dtn, W):
    ops = _ops()
    vec = [m for m in SHARDS if m * R.DTYPES[dtn].itemsize % 16 == 0]
    assert vec and len(vec) < len(SHARDS) and 1 in SHARDS, vec  # both paths
    for name, x, m in _shard_inputs(dtn, W):
        ref = _ref_shard_wire(dtn, W, name)
        got = ops.mx_quantize_shards(x.to(_dev()), W, wire=W6)
        assert got.dtype == torch.uint8 and got.numel() == ops.mx_shard_wire_bytes(m, W, wire=W6) == ref.size
        _assert_wire(got, ref, W, f"{dtn} {name} W={W}")


@pytest.mark.parametrize("W", WORLDS)
@pytest.mark.parametrize("dtn", list(R.DTYPES))
def test_dequantize_shards(dtn, W):
    ops = _ops()
    for name, x, m in _shard_inputs(dtn, W):
        ref = _ref_shard_wire(dtn, W, name)
        w = torch.from_numpy(ref).to(_dev())
        for odt in R.DTYPES.values():
            got = ops.mx_dequantize_shards(w, m, odt, W, wire=W6)
            assert got.dtype == odt and got.numel() == W * m
            assert R.same(got, R.dequantize_shards(ref, m, W, odt)), (dtn, name, W, odt)


# ------------------------------------------------------------------ reduce and fold
@functools.lru_cache(maxsize=None)
def _sources(nsrc, n):
    """(the sources' chunk wires back to back, the same in reversed source order)."""
    xs = M8.rank_inputs(n, nsrc, 40 + nsrc)
    xs[nsrc - 1][:1024] = torch.from_numpy(R.edge_tensor()[0][:1024])  # NaN, inf, zero blocks on the last source
    wires = [R.quantize(R.f32(x), 1) for x in xs]
    return np.concatenate(wires), np.concatenate(wires[::-1])


@pytest.mark.parametrize("nsrc", range(1, 9))
def test_reduce_folds_in_source_order(nsrc):
    ops = _ops()
    for n in (48 * 32, 65553):  # one workgroup, and several with a ragged end
        wire, back = _sources(nsrc, n)
        assert (R.split(wire, nsrc)[1] == 255).any()  # a scale-255 source block
        g = torch.from_numpy(wire).to(_dev())
        for op in ("sum", "avg"):
            _assert_wire(ops.mx_reduce(g, nsrc, op, wire=W6), R.reduce(wire, nsrc, op), 1, f"nsrc={nsrc} n={n} {op}")
            _assert_wire(ops.mx_reduce(g, nsrc, op, wire=W6, seed=nsrc, stream=3, **SR), R.reduce(wire, nsrc, op, (nsrc, 3)),
                         1, f"stochastic nsrc={nsrc} n={n} {op}")
        if nsrc >= 3:  # the inputs tell orders apart: a reversed fold gives another wire
            assert not R.same_wire(R.reduce(back, nsrc, "sum"), R.reduce(wire, nsrc, "sum"), 1)
        if nsrc == 3:  # AVG is a true division: a third is no multiplication by a rounded reciprocal
            assert not R.same_wire(R.reduce(wire, nsrc, "avg"), R.reduce(wire, nsrc, "sum"), 1)


def test_one_finite_source_comes_back_as_its_own_values():
    ops = _ops()
    x = M8.rank_inputs(4113, 2, 17)[0]
    w = R.quantize(R.f32(x), 1)
    g = torch.from_numpy(w).to(_dev())
    for kw in ({}, dict(seed=4, stream=9, **SR)):
        got = ops.mx_reduce(g, 1, "sum", wire=W6, **kw).cpu().numpy()
        assert np.array_equal(R.d_blocks(*R.split(got, 1)), R.d_blocks(*R.split(w, 1)))


@pytest.mark.parametrize("nsrc", [1, 2, 5, 8])
def test_reduce_with_the_owner_residual_over_three_calls(nsrc):
    ops = _ops()
    n = 4113
    cb = R.chunk_blocks(n, 1)
    sim = (np.random.default_rng(nsrc).standard_normal(32 * cb) * 0.05).astype(np.float32)
    res = torch.from_numpy(sim.copy()).to(_dev())
    for call, op in enumerate(("sum", "avg", "sum")):
        xs = M8.rank_inputs(n, nsrc, 90 + nsrc + call)
        if call == 1:
            xs[0][:1024] = torch.from_numpy(R.edge_tensor()[0][:1024])
        wire = np.concatenate([R.quantize(R.f32(x), 1) for x in xs])
        want, sim = R.reduce_ef(wire, nsrc, op, sim)
        got = ops.mx_reduce(torch.from_numpy(wire).to(_dev()), nsrc, op, wire=W6, residual=res)
        _assert_wire(got, want, 1, f"nsrc={nsrc} call={call}")
        assert R.same_residual(res, sim), (nsrc, call)


@pytest.mark.parametrize("op", ["sum", "avg"])
@pytest.mark.parametrize("nsrc", range(1, 9))
def test_fold(nsrc, op):
    ops = _ops()
    for n in (48 * 32, 65553):
        wire, back = _sources(nsrc, n)
        g = torch.from_numpy(wire).to(_dev())
        for dt in R.DTYPES.values():
            got = ops.mx_fold(g, nsrc, n, dt, op, wire=W6)
            assert got.dtype == dt and got.numel() == n
            assert R.same(got, R.fold(wire, nsrc, n, op, dt)), (nsrc, n, op, dt)
        assert bool(R.fold(wire, nsrc, n, op)[:1024].isnan().any())  # the NaN blocks are there
        if nsrc >= 3:
            assert not R.same(R.fold(back, nsrc, n, op), R.fold(wire, nsrc, n, op))


def test_fold_of_ragged_sizes():
    ops = _ops()
    for n in NUMELS[:-1]:  # the last lanes of a quad / a pair without their neighbours' elements
        xs = M8.rank_inputs(n, 3, 70 + n)
        wire = np.concatenate([R.quantize(R.f32(x), 1) for x in xs])
        for dt in R.DTYPES.values():
            got = ops.mx_fold(torch.from_numpy(wire).to(_dev()), 3, n, dt, "sum", wire=W6)
            assert R.same(got, R.fold(wire, 3, n, "sum", dt)), (n, dt)


# ------------------------------------------------------------------ error feedback in quantize, guard bands
def _arena(n, dtype, fill, off):
    a = torch.full((n + 2 * off,), fill, dtype=dtype, device=_dev())
    return a, a[off:off + n]


def _intact(arena, n, off, fill):
    a = arena.cpu()
    return bool((a[:off] == fill).all() and (a[off + n:] == fill).all())


@pytest.mark.parametrize("dtn", list(R.DTYPES))
def test_quantize_with_a_residual_in_patterned_arenas(dtn):
    """Dealt and shard layout: wire, residual and the unchanged tensor equal the reference over two calls; a
    residual that holds NaN restarts at +0; nothing outside tensor, wire and residual is written (patterned
    arenas around all three), and nothing past a shard's end enters the shard's last block."""
    ops = _ops()
    dt = R.DTYPES[dtn]
    for n, W, shard in ((33, 3, False), (4113, 1, False), (65553, 8, False), (5, 3, True), (33, 3, True), (96, 8, True),
                        (513, 2, True), (4113, 3, True)):
        total = n * W if shard else n
        x = (shard_inputs(n, max(W, 2), 11 + n, dt)[1][:total] if shard else M8.rank_inputs(n, 2, 11 + n, dt)[0]).clone()
        sim = (np.random.default_rng(n).standard_normal(total) * 0.05).astype(np.float32)
        sim[total // 2] = np.nan  # this element's block goes out as NaN once, its residual restarts at +0
        nbytes = R.shard_wire_bytes(n, W) if shard else R.wire_bytes(n, W)
        xa, xv = _arena(total, dt, -7.5, 64)
        xv.copy_(x)
        ra, rv = _arena(total, torch.float32, 123.0, 64)
        rv.copy_(torch.from_numpy(sim))
        for call in range(2):
            want_w, sim = (R.quantize_shards_ef if shard else R.quantize_ef)(R.f32(x), sim, W)
            wa, wv = _arena(nbytes, torch.uint8, 0xA5, 256)
            fn = ops.mx_quantize_shards if shard else ops.mx_quantize
            got = fn(xv, W, out=wv, wire=W6, residual=rv)
            assert got.data_ptr() == wv.data_ptr()
            _assert_wire(got, want_w, W, f"{dtn} n={n} W={W} shard={shard} call={call}")
            assert call or (R.split(want_w, W)[1] == 255).any()
            assert R.same_residual(rv, sim), (dtn, n, W, shard, call)
            assert _intact(wa, nbytes, 256, 0xA5) and _intact(ra, total, 64, 123.0) and _intact(xa, total, 64, -7.5)
            assert torch.equal(xv.cpu(), x)
        # plain and stochastic into an arena, and back out of it into one
        for kw, sr in (({}, None), (dict(seed=n, stream=2, index_offset=7, **SR), (n, 2, 7))):
            wa, wv = _arena(nbytes, torch.uint8, 0x5A, 256)
            (ops.mx_quantize_shards if shard else ops.mx_quantize)(xv, W, out=wv, wire=W6, **kw)
            want = R.quantize_shards(R.f32(x), W, sr) if shard else R.quantize(R.f32(x), W, sr)
            _assert_wire(wv, want, W, f"{dtn} n={n} W={W} shard={shard} {kw}")
            assert _intact(wa, nbytes, 256, 0x5A)
        for off in (64, 67):  # the output 16-byte aligned, and not (through a copy)
            oa, ov = _arena(total, dt, -7.5, off)
            if shard:
                ops.mx_dequantize_shards(wv, n, dt, W, out=ov, wire=W6)
                want_d = R.dequantize_shards(want, n, W, dt)
            else:
                ops.mx_dequantize(wv, n, dt, W, out=ov, wire=W6)
                want_d = R.dequantize(want, n, W, dt)
            assert R.same(ov, want_d) and _intact(oa, total, off, -7.5), (dtn, n, W, shard, off)


# ------------------------------------------------------------------ stochastic rounding: the words of an index
def test_both_layouts_draw_the_same_words():
    ops = _ops()
    W, m = 4, 96  # whole blocks per shard: the two layouts hold the same blocks
    x = shard_inputs(m, W, 5)[0][:W * m].clone()
    for off in (0, 12345, (1 << 32) - 100, (1 << 40) + 3):  # indices past 2^32: the key of the high word
        kw = dict(wire=W6, seed=77, stream=5, index_offset=off, **SR)
        dealt = ops.mx_quantize(x.to(_dev()), 1, **kw).cpu().numpy()
        shards = ops.mx_quantize_shards(x.to(_dev()), W, **kw).cpu().numpy()
        assert np.array_equal(dealt, R.quantize(R.f32(x), 1, (77, 5, off))), off
        assert np.array_equal(shards, R.quantize_shards(R.f32(x), W, (77, 5, off))), off
        dq, ds = R.split(dealt, 1)
        sq, ss = R.split(shards, W)
        nb = m // 32
        for r in range(W):
            assert np.array_equal(dq[r * nb:(r + 1) * nb], sq[r * 16:r * 16 + nb]), (off, r)
    a = ops.mx_quantize(x.to(_dev()), 1, wire=W6, seed=77, stream=5, **SR)
    assert not torch.equal(a, ops.mx_quantize(x.to(_dev()), 1, wire=W6, seed=77, stream=6, **SR))


def test_wrong_arguments_raise():
    ops = _ops()
    dev = _dev()
    for bad in ("mxfp6", "mxfp6_e3m2"):
        with pytest.raises(ValueError, match=f"unknown wire format '{bad}'.*mxfp6_e2m3"):
            ops.mx_quantize(torch.zeros(8, device=dev), wire=bad)
    with pytest.raises(TypeError, match="float64"):
        ops.mx_quantize(torch.zeros(8, dtype=torch.float64, device=dev), wire=W6)
    with pytest.raises(ValueError, match="'max'"):
        ops.mx_reduce(torch.zeros(25 * 16, dtype=torch.uint8, device=dev), 1, "max", wire=W6)
    for other in (33, 17):  # an FP8 or FP4 chunk is not an FP6 chunk
        with pytest.raises(RuntimeError, match="25 bytes per block"):
            ops.mx_reduce(torch.zeros(other * 16, dtype=torch.uint8, device=dev), 1, wire=W6)
        with pytest.raises(RuntimeError, match="400 bytes"):
            ops.mx_dequantize(torch.zeros(other * 16, dtype=torch.uint8, device=dev), 64, wire=W6)
        with pytest.raises(RuntimeError, match="400 bytes"):
            ops.mx_fold(torch.zeros(other * 16, dtype=torch.uint8, device=dev), 1, 32, wire=W6)
        with pytest.raises(RuntimeError, match="800 bytes"):
            ops.mx_dequantize_shards(torch.zeros(other * 16, dtype=torch.uint8, device=dev), 33, torch.float32, 2, wire=W6)


# ------------------------------------------------------------------ the collectives, ranks sharing GPU 0
def _check(res, cases):
    for r, got in enumerate(res):
        assert len(got) == cases, sorted(got)
        bad = [k for k, v in got.items() if not v[0]]
        assert not bad, (r, bad)
        same = {k: v[1] for k, v in got.items() if not k.startswith("rs")}  # the same bits on every rank
        assert same == {k: v[1] for k, v in res[0].items() if not k.startswith("rs")}, r


@pytest.mark.parametrize("async_op", [False, True])
@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_collectives(world, async_op):
    # 33: whole padding chunks; 4113: a ragged end; plain, residuals over three calls, stochastic
    numels = (33, 4113)
    dtypes = ("float32", "bfloat16") if world == 2 else ("float32",)
    res = _gpu_launch(M.collective_cases, world, args=("cuda", numels, dtypes, async_op), timeout_s=120)
    _check(res, len(dtypes) * len(numels) * M.CASES_PER_SIZE)


def test_collectives_float16():
    res = _gpu_launch(M.collective_cases, 2, args=("cuda", (1, 513), ("float16",)), timeout_s=120)
    _check(res, 2 * M.CASES_PER_SIZE)


def test_world_1_and_errors_on_the_gpu():
    got = _gpu_launch(M.world1_and_errors, 1)[0]
    assert len(got) == 9 + M.N_ERRORS and all(got.values()), got


@pytest.mark.parametrize("mode", ["plain", "ef", "sr"])
def test_grad_bucketer_with_the_fp6_wire(mode):
    res = _gpu_launch(M.bucketer, 2, args=("cuda", mode), timeout_s=120)
    for got in res:
        assert got["buckets"] >= 2 and got["handles"] == ["CompressedWork"] and len(got["steps"]) == 3, got
        for t, step in enumerate(got["steps"]):
            for i in range(got["buckets"]):
                assert step[i][0], (t, i, step[i])
                assert step[i][1] == res[0]["steps"][t][i][1]


@pytest.mark.parametrize("grad_wire,param_wire,mode", [(W6, W6, "plain"), ("mxfp4_e2m1", W6, "plain"), (W6, W6, "ef")])
def test_sharded_optimizer_with_fp6_wires(grad_wire, param_wire, mode):
    res = _gpu_launch(M.zero, 2, args=("cuda", grad_wire, param_wire, mode), timeout_s=120)
    for got in res:
        assert got["buckets"] >= 2 and got["handles"] == ["CompressedWork"] and len(got["steps"]) == 3, got
        for t, step in enumerate(got["steps"]):
            for i in range(got["buckets"]):
                assert step[i][0] and step[i][1], (t, i, step[i])
            assert step["digest"] == res[0]["steps"][t]["digest"]
        assert got["restored"] == got["original"], got
