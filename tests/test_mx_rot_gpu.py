"""The Hadamard rotation of the block-scaled wires on the GPU (docs/collectives.md "Hadamard rotation"): the
rotated instantiations of the quantize, dequantize and fold kernels in both layouts, the three collectives, the
bucketer and the sharded optimizer.

The reference is always tests/_mx_rot_ref.py (numpy on the CPU): wires must equal it byte for byte (the payload
under a NaN block, scale 255, is unspecified), values exactly -- rtol = atol = 0, NaN where the reference has NaN.
The sizes are those at which the lanes of a block can go wrong once they exchange values: a partial last block
(whose padding positions carry payload in the rotated domain), a partial last quad, more than one workgroup, the
vector and the element path of the shard layout, blocks clipped at shard ends, one FP6 chunk past the 1 MiB rule.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _mx_rot_ref as R
from tests import _workers_mx as M8
from tests import _workers_mx_rot as M
from tests._workers_mx_shard import shard_inputs
from tests.test_backend_gpu import _gpu_launch

pytestmark = pytest.mark.gpu

WIRES = tuple(R.WIRES)
SEED = M.RSEED
ROT = dict(rotation="hadamard", rotation_seed=SEED)
SR = dict(rounding="stochastic")
NUMELS = (1, 31, 32, 33, 63, 65, 255, 257, 4095, 4097, 65553)
# 64, 96 and 4096 start every shard 16-byte aligned in every dtype (the vector path); the others do not
SHARDS = (1, 5, 31, 33, 64, 96, 511, 4096, 4113)
WORLDS = (1, 3, 8)
BIG = 45056 * 32 - 7  # FP6: cb = 45056, the first multiple of 4096 past the 1 MiB threshold


def _ops():
    from pytorch_distributed_collective_communication_amd import ops

    return ops


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _inputs(wire, dtn):
    """[(name, CPU tensor of dtype dtn)]: the wire's edge blocks, then every ragged size."""
    dt = R.DTYPES[dtn]
    return [("edge", torch.from_numpy(R.edge_tensor(wire)).to(dt))] + \
        [(f"n{n}", M8.rank_inputs(n, 2, 900 + n, dt)[1]) for n in NUMELS]


@functools.lru_cache(maxsize=None)
def _ref_wire(wire, dtn, name, world):
    return R.quantize(R.f32(dict(_inputs(wire, dtn))[name]), world, wire, SEED)


@functools.lru_cache(maxsize=None)
def _shard_inputs(wire, dtn, W):
    dt = R.DTYPES[dtn]
    out = [(f"m{m}", shard_inputs(m, max(W, 2), 900 + m, dt)[1][:W * m].clone(), m) for m in SHARDS]
    edge = torch.from_numpy(R.edge_tensor(wire))
    m = edge.numel()
    x = shard_inputs(m, max(W, 2), 7)[0][:W * m].clone()
    x[(W - 1) * m:] = edge
    out.append(("edge", x.to(dt), m))
    return out


@functools.lru_cache(maxsize=None)
def _ref_shard_wire(wire, dtn, W, name):
    x = {n: t for n, t, _ in _shard_inputs(wire, dtn, W)}[name]
    return R.quantize_shards(R.f32(x), W, wire, SEED)


def _assert_wire(got, ref, nchunks, wire, what):
    got = got.cpu().numpy()
    if not R.same_wire(got, ref, nchunks, wire):
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        gq, gs = R.WIRES[wire].split(got, nchunks)
        rq, rs = R.WIRES[wire].split(ref, nchunks)
        bad = np.nonzero((gs != rs) | ((gq != rq).any(axis=1) & (rs != 255)))[0]
        first = [(int(b), int(gs[b]), int(rs[b]), gq[b].tolist(), rq[b].tolist()) for b in bad[:2]]
        pytest.fail(f"{what}: {len(bad)} blocks differ; (block, s, want s, payload, want payload): {first}")


def test_sign_word_of_the_extension():
    ops = _ops()
    for seed in (0, 1, 12345, SEED, (1 << 64) - 1):
        assert ops._C().mx_rotation_signs(seed) == ops.mx_rotation_signs(seed) == R.signs(seed)


# ------------------------------------------------------------------ quantize / dequantize, dealt layout
@pytest.mark.parametrize("dtn", list(R.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_quantize(wire, dtn):
    ops = _ops()
    for name, x in _inputs(wire, dtn):
        xg = x.to(_dev())
        for world in (1, 3):
            ref = _ref_wire(wire, dtn, name, world)
            got = ops.mx_quantize(xg, world, wire=wire, **ROT)
            assert got.dtype == torch.uint8 and got.numel() == ref.size
            _assert_wire(got, ref, world, wire, f"{wire} {dtn} {name} world={world}")
        want = R.quantize(R.f32(x), 1, wire, SEED, sr=(77, 5, 1 << 33))
        got = ops.mx_quantize(xg, 1, wire=wire, seed=77, stream=5, index_offset=1 << 33, **SR, **ROT)
        _assert_wire(got, want, 1, wire, f"stochastic {wire} {dtn} {name}")
        sim = (np.random.default_rng(x.numel()).standard_normal(x.numel()) * 0.05).astype(np.float32)
        res = torch.from_numpy(sim.copy()).to(_dev())
        for call in range(2):
            want, sim = R.quantize(R.f32(x), 1, wire, SEED, res=sim)
            _assert_wire(ops.mx_quantize(xg, 1, wire=wire, residual=res, **ROT), want, 1, wire,
                         f"residual {wire} {dtn} {name} call={call}")
            assert R.same_residual(res, sim), (wire, dtn, name, call)


@pytest.mark.parametrize("dtn", list(R.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_dequantize(wire, dtn):
    # (dtn: the dtype the wire was quantized from; every output dtype is checked)
    ops = _ops()
    for name, x in _inputs(wire, dtn):
        for world in (1, 3):
            ref = _ref_wire(wire, dtn, name, world)
            w = torch.from_numpy(ref).to(_dev())
            for odt in R.DTYPES.values():
                got = ops.mx_dequantize(w, x.numel(), odt, world, wire=wire, **ROT)
                assert got.dtype == odt and got.numel() == x.numel()
                assert R.same(got, R.dequantize(ref, x.numel(), world, wire, SEED, odt)), (wire, dtn, name, world, odt)


@pytest.mark.parametrize("wire", WIRES)
def test_partial_block_round_trip(wire):
    """33 and 4113 elements: the last block holds one (17) elements and padding zeros whose rotated coefficients
    are not zero. A dequantize that leaves the padding lanes out of the inverse butterfly fails here."""
    ops = _ops()
    for n in (33, 4113):
        for dtn, dt in R.DTYPES.items():
            x = M8.rank_inputs(n, 2, 30 + n, dt)[0]
            got = ops.mx_dequantize(ops.mx_quantize(x.to(_dev()), 1, wire=wire, **ROT), n, dt, 1, wire=wire, **ROT)
            ref = R.quantize(R.f32(x), 1, wire, SEED)
            assert R.WIRES[wire].split(ref, 1)[0][n // 32].any()
            assert R.same(got, R.dequantize(ref, n, 1, wire, SEED, dt)), (wire, n, dtn)
            plain = ops.mx_dequantize(ops.mx_quantize(x.to(_dev()), 1, wire=wire), n, dt, 1, wire=wire)
            assert not R.same(got, plain), (wire, n, dtn)


def test_a_chunk_past_the_1_mib_rule():
    ops = _ops()
    wire = "mxfp6_e2m3"
    assert ops.mx_chunk_blocks(BIG, 1, wire=wire) == 45056
    x = torch.from_numpy(R.R6.random_binades(BIG // 32 + 1, 3, -10, 10).reshape(-1)[:BIG].copy())
    ref = R.quantize(R.f32(x), 1, wire, SEED)
    _assert_wire(ops.mx_quantize(x.to(_dev()), 1, wire=wire, **ROT), ref, 1, wire, "big")
    got = ops.mx_dequantize(torch.from_numpy(ref).to(_dev()), BIG, torch.float32, 1, wire=wire, **ROT)
    assert R.same(got, R.dequantize(ref, BIG, 1, wire, SEED))


# ------------------------------------------------------------------ the shard layout
@pytest.mark.parametrize("W", WORLDS)
@pytest.mark.parametrize("dtn", list(R.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_shards(wire, dtn, W):
    ops = _ops()
    dt = R.DTYPES[dtn]
    vec = [m for m in SHARDS if m * dt.itemsize % 16 == 0]
    assert vec and len(vec) < len(SHARDS)  # both paths
    for name, x, m in _shard_inputs(wire, dtn, W):
        xg = x.to(_dev())
        ref = _ref_shard_wire(wire, dtn, W, name)
        got = ops.mx_quantize_shards(xg, W, wire=wire, **ROT)
        assert got.numel() == ops.mx_shard_wire_bytes(m, W, wire=wire) == ref.size
        _assert_wire(got, ref, W, wire, f"{wire} {dtn} {name} W={W}")
        out = ops.mx_dequantize_shards(torch.from_numpy(ref).to(_dev()), m, dt, W, wire=wire, **ROT)
        assert R.same(out, R.dequantize_shards(ref, m, W, wire, SEED, dt)), (wire, dtn, name, W)
        want = R.quantize_shards(R.f32(x), W, wire, SEED, sr=(9, 2, 7))
        _assert_wire(ops.mx_quantize_shards(xg, W, wire=wire, seed=9, stream=2, index_offset=7, **SR, **ROT), want, W, wire,
                     f"stochastic {wire} {dtn} {name} W={W}")
        sim = (np.random.default_rng(m).standard_normal(W * m) * 0.05).astype(np.float32)
        res = torch.from_numpy(sim.copy()).to(_dev())
        want, sim = R.quantize_shards(R.f32(x), W, wire, SEED, res=sim)
        _assert_wire(ops.mx_quantize_shards(xg, W, wire=wire, residual=res, **ROT), want, W, wire,
                     f"residual {wire} {dtn} {name} W={W}")
        assert R.same_residual(res, sim), (wire, dtn, name, W)


# ------------------------------------------------------------------ fold
@functools.lru_cache(maxsize=None)
def _sources(wire, nsrc, n):
    xs = M8.rank_inputs(n, nsrc, 940 + nsrc)
    if n > 1024:
        xs[nsrc - 1][:1024] = torch.from_numpy(R.edge_tensor(wire)[:1024])  # NaN, inf, zero blocks on the last source
    return np.concatenate([R.quantize(R.f32(x), 1, wire, SEED) for x in xs])


@pytest.mark.parametrize("op", ["sum", "avg"])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 8])
@pytest.mark.parametrize("wire", WIRES)
def test_fold(wire, nsrc, op):
    ops = _ops()
    for n in NUMELS:
        w = _sources(wire, nsrc, n)
        g = torch.from_numpy(w).to(_dev())
        for dt in R.DTYPES.values():
            got = ops.mx_fold(g, nsrc, n, dt, op, wire=wire, **ROT)
            assert got.dtype == dt and got.numel() == n
            assert R.same(got, R.fold(w, nsrc, n, op, wire, SEED, dt)), (wire, nsrc, n, op, dt)
    assert bool(R.fold(_sources(wire, nsrc, 65553), nsrc, 65553, op, wire, SEED)[:1024].isnan().any())


# ------------------------------------------------------------------ guard bands
def _arena(n, dtype, fill, off):
    a = torch.full((n + 2 * off,), fill, dtype=dtype, device=_dev())
    return a, a[off:off + n]


def _intact(arena, n, off, fill):
    a = arena.cpu()
    return bool((a[:off] == fill).all() and (a[off + n:] == fill).all())


@pytest.mark.parametrize("dtn", list(R.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_nothing_outside_the_outputs_is_written(wire, dtn):
    """Patterned arenas around the tensor, the wire, the residual and the outputs of dequantize and fold, in both
    layouts: the lanes of a partial block that take part in the butterfly store nothing, and the residual past the
    end of the tensor (the rotated coefficients of the padding positions) is dropped, not written."""
    ops = _ops()
    dt = R.DTYPES[dtn]
    for n, W, shard in ((33, 3, False), (4113, 1, False), (65553, 8, False), (5, 3, True), (33, 3, True), (96, 8, True),
                        (4113, 3, True)):
        total = n * W if shard else n
        x = (shard_inputs(n, max(W, 2), 21 + n, dt)[1][:total] if shard else M8.rank_inputs(n, 2, 21 + n, dt)[0]).clone()
        sim = (np.random.default_rng(n).standard_normal(total) * 0.05).astype(np.float32)
        xa, xv = _arena(total, dt, -7.5, 64)
        xv.copy_(x)
        ra, rv = _arena(total, torch.float32, 123.0, 64)
        rv.copy_(torch.from_numpy(sim))
        want, sim = (R.quantize_shards if shard else R.quantize)(R.f32(x), W, wire, SEED, res=sim)
        nbytes = want.size
        wa, wv = _arena(nbytes, torch.uint8, 0xA5, 256)
        (ops.mx_quantize_shards if shard else ops.mx_quantize)(xv, W, out=wv, wire=wire, residual=rv, **ROT)
        _assert_wire(wv, want, W, wire, f"{wire} {dtn} n={n} W={W} shard={shard}")
        assert R.same_residual(rv, sim), (wire, dtn, n, W, shard)
        assert _intact(wa, nbytes, 256, 0xA5) and _intact(ra, total, 64, 123.0) and _intact(xa, total, 64, -7.5)
        assert torch.equal(xv.cpu(), x)
        for off in (64, 67):  # the output 16-byte aligned, and not (through a copy)
            oa, ov = _arena(total, dt, -7.5, off)
            if shard:
                ops.mx_dequantize_shards(wv, n, dt, W, out=ov, wire=wire, **ROT)
                want_d = R.dequantize_shards(want, n, W, wire, SEED, dt)
            else:
                ops.mx_dequantize(wv, n, dt, W, out=ov, wire=wire, **ROT)
                want_d = R.dequantize(want, n, W, wire, SEED, dt)
            assert R.same(ov, want_d) and _intact(oa, total, off, -7.5), (wire, dtn, n, W, shard, off)
        if shard:  # the W chunks of a shard wire are W sources of n elements
            oa, ov = _arena(n, dt, -7.5, 64)
            ops.mx_fold(wv, W, n, dt, "avg", out=ov, wire=wire, **ROT)
            assert R.same(ov, R.fold(want, W, n, "avg", wire, SEED, dt)) and _intact(oa, n, 64, -7.5), (wire, dtn, n, W)


# ------------------------------------------------------------------ defaults
@pytest.mark.parametrize("wire", WIRES)
def test_no_rotation_is_the_call_without_the_keyword(wire):
    ops = _ops()
    x = M8.rank_inputs(4113, 2, 5)[0].to(_dev())
    none = dict(rotation=None, rotation_seed=SEED)
    w = ops.mx_quantize(x, 3, wire=wire)
    assert torch.equal(ops.mx_quantize(x, 3, wire=wire, **none), w)
    assert torch.equal(ops.mx_quantize(x, 3, wire=wire, seed=3, **SR, **none), ops.mx_quantize(x, 3, wire=wire, seed=3, **SR))
    r1, r2 = torch.zeros(4113, device=_dev()), torch.zeros(4113, device=_dev())
    assert torch.equal(ops.mx_quantize(x, 3, wire=wire, residual=r1, **none), ops.mx_quantize(x, 3, wire=wire, residual=r2))
    assert torch.equal(r1, r2) and bool(r1.any())
    assert torch.equal(ops.mx_dequantize(w, 4113, torch.float32, 3, wire=wire, **none),
                       ops.mx_dequantize(w, 4113, torch.float32, 3, wire=wire))
    s = ops.mx_quantize_shards(x, 3, wire=wire)
    assert torch.equal(ops.mx_quantize_shards(x, 3, wire=wire, **none), s)
    assert torch.equal(ops.mx_dequantize_shards(s, 1371, torch.float32, 3, wire=wire, **none),
                       ops.mx_dequantize_shards(s, 1371, torch.float32, 3, wire=wire))
    assert torch.equal(ops.mx_fold(s, 3, 1371, torch.float32, "avg", wire=wire, **none),
                       ops.mx_fold(s, 3, 1371, torch.float32, "avg", wire=wire))
    assert not torch.equal(ops.mx_quantize(x, 3, wire=wire, **ROT), w)


# ------------------------------------------------------------------ the collectives, ranks sharing GPU 0
def _check(res, cases):
    for r, got in enumerate(res):
        assert len(got) == cases, sorted(got)
        bad = [k for k, v in got.items() if not v[0]]
        assert not bad, (r, bad)
        same = {k: v[1] for k, v in got.items() if not k.startswith("rs")}  # the same bits on every rank
        assert same == {k: v[1] for k, v in res[0].items() if not k.startswith("rs")}, r


@pytest.mark.parametrize("async_op", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_collectives(world, async_op):
    # 33: whole padding chunks and a one-element block; 4113: a ragged end
    numels = (33, 4113)
    res = _gpu_launch(M.collective_cases, world, args=("cuda", numels, ("float32",), async_op), timeout_s=120)
    _check(res, len(WIRES) * len(numels) * M.CASES_PER_SIZE)


def test_collectives_16_bit():
    res = _gpu_launch(M.collective_cases, 2, args=("cuda", (513,), ("bfloat16", "float16"), True, ("mxfp4_e2m1", "mxfp6_e2m3")),
                      timeout_s=120)
    _check(res, 2 * 2 * M.CASES_PER_SIZE)


def test_world_1_and_errors_on_the_gpu():
    got = _gpu_launch(M.world1_and_errors, 1)[0]
    assert len(got) == 3 + M.N_ERRORS and all(got.values()), got


def test_grad_bucketer_with_a_rotated_fp4_wire():
    res = _gpu_launch(M.bucketer, 2, args=("cuda", "mxfp4_e2m1", "ef"), timeout_s=120)
    for got in res:
        assert got["buckets"] >= 2 and got["handles"] == ["CompressedWork"] and len(got["steps"]) == 3, got
        for t, step in enumerate(got["steps"]):
            for i in range(got["buckets"]):
                assert step[i][0], (t, i, step[i])
                assert step[i][1] == res[0]["steps"][t][i][1]


def test_sharded_optimizer_with_rotated_fp4_gradients_and_fp6_parameters():
    res = _gpu_launch(M.zero, 2, args=("cuda", "mxfp4_e2m1", "mxfp6_e2m3", "plain"), timeout_s=120)
    for got in res:
        assert got["buckets"] >= 2 and got["handles"] == ["CompressedWork"] and len(got["steps"]) == 3, got
        assert got["state_keys"] == []
        for t, step in enumerate(got["steps"]):
            for i in range(got["buckets"]):
                assert step[i][0] and step[i][1], (t, i, step[i])
            assert step["digest"] == res[0]["steps"][t]["digest"]
