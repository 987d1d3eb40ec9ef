"""The shard layout of the `mxfp8_e4m3` wire, `mx_fold`, and the compressed reduce-scatter /
all-gather without a GPU (docs/collectives.md "Compressed reduce-scatter and all-gather").

* `ops.mx_*_shards_reference` and `ops.mx_fold_reference` (plain PyTorch) against
  tests/_mx_shard_ref.py (numpy on tests/_mx_ref.py's block functions);
* the shard layout against the dealt one: the same bytes when a shard is whole chunks, other bytes
  when it is not;
* the derived error bound of the reduce-scatter against an f64 sum;
* `reduce_scatter_compressed` / `all_gather_compressed` on CPU tensors over the shm transport
  (worlds 2, 3, 4), world 1, the error cases; `ShardedOptimizer(grad_wire, param_wire)` at world 2;
* the shard offsets of the layout header under ASan + UBSan
  (tests/native/mx_shard_layout_check.cpp, a stand-alone program).

Every comparison is exact: rtol = atol = 0, NaN where the reference has NaN.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

from pytorch_distributed_collective_communication_amd import ops
from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _mx_ref as R
from tests import _mx_shard_ref as SR
from tests import _workers_mx_shard as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
BUILD = os.path.join(ROOT, "build", "san")
SRC = os.path.join(ROOT, "tests", "native", "mx_shard_layout_check.cpp")
HDR = os.path.join(CSRC, "kernels", "mx_layout.h")

SHARDS = (1, 31, 32, 33, 511, 512, 513, 4113)
WORLDS = (1, 2, 3, 8)


def _edge_as_a_shard(W, dt):
    """(x, m): W shards of the edge tensor's length, the edge tensor itself as the last one."""
    edge = torch.from_numpy(R.edge_tensor()[0])
    m = edge.numel()
    xs = MS.shard_inputs(m, max(W, 2), 7, torch.float32)[0][:W * m].clone()
    xs[(W - 1) * m:] = edge
    return xs.to(dt), m


# ------------------------------------------------------------------ the references against each other
@pytest.mark.parametrize("W", WORLDS)
@pytest.mark.parametrize("dtn", list(R.DTYPES))
def test_shard_references_agree(dtn, W):
    dt = R.DTYPES[dtn]
    cases = [(MS.shard_inputs(m, max(W, 2), 50 + m, dt)[1][:W * m], m) for m in SHARDS] + [_edge_as_a_shard(W, dt)]
    for x, m in cases:
        want = SR.quantize_shards(R.f32(x), W)
        got = ops.mx_quantize_shards_reference(x, W)
        assert got.dtype == torch.uint8
        assert got.numel() == ops.mx_shard_wire_bytes(m, W) == SR.shard_wire_bytes(m, W) == want.size
        assert ops.mx_shard_blocks(m) == SR.shard_blocks(m) == ops.mx_chunk_blocks(m, 1)
        assert np.array_equal(got.numpy(), want), (dtn, m, W)  # every byte (both write 0 under a NaN block)
        # chunk r is the wire of shard r alone: nothing of the next shard, padding as scale 127 / payload 0
        cb = ops.mx_shard_blocks(m)
        for r in range(W):
            chunk = got.numpy()[33 * cb * r:33 * cb * (r + 1)]
            assert np.array_equal(chunk, R.quantize(R.f32(x)[r * m:(r + 1) * m], 1)), (dtn, m, W, r)
            q, s = R.split(chunk, 1)
            first_pad = -(-m // 32)
            assert (s[first_pad:] == 127).all() and not q[first_pad:].any()
            if m % 32 and s[first_pad - 1] != 255:
                assert not q[first_pad - 1, m % 32:].any()
        for odt in R.DTYPES.values():
            d = ops.mx_dequantize_shards_reference(got, m, odt, W)
            assert d.dtype == odt and d.numel() == W * m
            assert R.same(d, SR.dequantize_shards(want, m, W, odt)), (dtn, m, W, odt)


@pytest.mark.parametrize("op", ["sum", "avg"])
@pytest.mark.parametrize("nsrc", WORLDS)
def test_fold_reference_folds_in_source_order(nsrc, op):
    edge = torch.from_numpy(R.edge_tensor()[0])
    for m in SHARDS + (edge.numel(),):
        xs = MS.rank_inputs(m, nsrc, 60 + m)
        if m == edge.numel():
            xs[nsrc - 1] = edge.clone()  # NaN, inf, zero and clamped blocks on the last source
        wire = np.concatenate([R.quantize(R.f32(x), 1) for x in xs])
        for dt in R.DTYPES.values():
            want = SR.fold(wire, nsrc, m, op, dt)
            got = ops.mx_fold_reference(torch.from_numpy(wire), nsrc, m, dt, op)
            assert got.dtype == dt and got.numel() == m
            assert R.same(got, want), (nsrc, m, op, dt)
        if m == edge.numel():
            nan_blocks = np.isnan(R.edge_tensor()[0].reshape(-1, 32)).any(axis=1) | np.isinf(
                R.edge_tensor()[0].reshape(-1, 32)).any(axis=1)
            got = ops.mx_fold_reference(torch.from_numpy(wire), nsrc, m, torch.float32, op).view(-1, 32)
            assert nan_blocks.any() and bool(got[torch.from_numpy(nan_blocks)].isnan().all())  # scale 255: 32 NaNs


def test_fold_rounds_once_and_f16_overflows_to_inf():
    # two sources of 40000 each: every D(Q(.)) is finite in f16, the f32 sum 80000 is not
    x = torch.full((64,), 40000.0)
    wire = np.concatenate([R.quantize(R.f32(x), 1)] * 2)
    want = SR.fold(wire, 2, 64, "sum", torch.float16)
    assert bool(want.isinf().all())
    assert R.same(ops.mx_fold_reference(torch.from_numpy(wire), 2, 64, torch.float16, "sum"), want)
    assert bool(torch.isfinite(SR.fold(wire, 2, 64, "avg", torch.float16)).all())  # divided before the rounding
    assert R.same(ops.mx_fold_reference(torch.from_numpy(wire), 2, 64, torch.float16, "avg"),
                  SR.fold(wire, 2, 64, "avg", torch.float16))


def test_inputs_tell_fold_orders_apart():
    # asserted on the reference alone: from 3 sources on a reversed fold gives other values for the
    # inputs the tests use, from 5 on a pairwise tree does too -- so equality pins the source order
    for W in (3, 4, 5, 8):
        for m in (33, 513):
            xs = MS.shard_inputs(m, W, MS._seed(m))
            for k in (0, W - 1):
                want = SR.reduce_scatter(xs, k, "sum")
                assert not R.same(SR.reduce_scatter(xs[::-1], k, "sum"), want), (W, m, k)
        xs = MS.rank_inputs(48 * 32, W, 40 + W)
        ds = [R.d_blocks(*R.q_blocks(R.pad_blocks(R.f32(x), 48))) for x in xs]
        seq = R.fold_blocks(ds, "sum")
        assert not np.array_equal(R.fold_blocks(ds[::-1], "sum"), seq)
        if W >= 5:
            level = ds
            while len(level) > 1:
                level = [R.fold_blocks(level[i:i + 2], "sum") for i in range(0, len(level), 2)]
            assert not np.array_equal(level[0], seq)
        # ... and the plain-PyTorch fold is the sequential one
        wire = torch.cat([ops.mx_quantize_reference(x, 1) for x in xs])
        assert R.same(ops.mx_fold_reference(wire, W, 48 * 32), torch.from_numpy(seq.reshape(-1)))


# ------------------------------------------------------------------ the shard layout against the dealt one
def test_shard_wire_is_the_dealt_wire_when_shards_are_whole_chunks():
    hits = 0
    for W in (1, 2, 3, 8):
        for m in (512, 1024, 512 * 5, 4096 * 32):
            assert 32 * ops.mx_chunk_blocks(W * m, W) == m
            x = MS.shard_inputs(m, max(W, 2), 3 + m)[0][:W * m]
            dealt = R.quantize(R.f32(x), W)
            assert np.array_equal(SR.quantize_shards(R.f32(x), W), dealt)
            assert np.array_equal(ops.mx_quantize_shards_reference(x, W).numpy(), dealt)
            hits += 1
    assert hits == 16


def test_shard_wire_differs_from_the_dealt_wire_when_they_are_not():
    # m = 33, W = 3: the dealt layout puts elements 32..63 into one block, the shard layout cuts at 33
    x = MS.shard_inputs(33, 3, 5)[0]
    dealt = R.quantize(R.f32(x), 3)
    mine = SR.quantize_shards(R.f32(x), 3)
    assert dealt.size == mine.size and not np.array_equal(mine, dealt)
    assert not R.same(SR.dequantize_shards(dealt, 33, 3), SR.dequantize_shards(mine, 33, 3))
    assert np.array_equal(ops.mx_quantize_shards_reference(x, 3).numpy(), mine)


# ------------------------------------------------------------------ the derived bound
@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_reduce_scatter_error_bound_against_the_f64_sum(world):
    # |result - exact| <= (sum_r amax_{r,b}) / 16 * (1 + 2^-10) per element of shard block b, before the
    # one rounding to the tensor dtype (f32 here: none): each contribution is quantized once and errs
    # by at most amax / 16 (3 mantissa bits, scaled amax <= 448; half an ulp of the top binade is 16 of
    # 448 ... 256), the f32 fold by far less (the 2^-10 slack), and nothing is quantized after the
    # fold -- one term fewer than the all-reduce's bound. Derived, not measured; for blocks with every
    # amax_r >= 2^-100.
    rng = np.random.default_rng(100 + world)
    m = 1024 * 32 + 17  # per shard: 1025 blocks, the last one clipped at the shard's end
    xs = []
    for r in range(world):
        normal = rng.standard_normal((world, m))
        lognormal = np.exp(rng.standard_normal((world, m)) * 3.0) * rng.choice([-1.0, 1.0], (world, m))
        x = np.where((np.arange(m) // 32 % 2 == 0)[None], normal, lognormal).astype(np.float32)
        xs.append(torch.from_numpy(x.reshape(-1)))
    worst = 0.0
    for k in range(world):
        parts = [R.pad_blocks(R.f32(x)[k * m:(k + 1) * m], 1025) for x in xs]
        exact = np.sum([p.astype(np.float64) for p in parts], axis=0)
        bound = np.sum([np.abs(p).max(axis=1).astype(np.float64) for p in parts], axis=0) / 16 * (1 + 2.0 ** -10)
        got = R.pad_blocks(SR.reduce_scatter(xs, k, "sum").numpy(), 1025)
        worst = max(worst, float((np.abs(got.astype(np.float64) - exact) / bound[:, None]).max()))
        # the torch references compute the same values
        wire = torch.cat([ops.mx_quantize_shards_reference(x, world)[33 * 1040 * k:33 * 1040 * (k + 1)] for x in xs])
        assert R.same(ops.mx_fold_reference(wire, world, m, torch.float32, "sum"), torch.from_numpy(got.reshape(-1)[:m]))
    print(f"world {world}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0, worst


def test_all_gather_error_is_one_quantization():
    # |D(Q(x)) - x| <= amax_b / 16 per element of block b (amax_b >= 2^-100)
    rng = np.random.default_rng(9)
    x = np.concatenate([rng.standard_normal((512, 32)), np.exp(rng.standard_normal((512, 32)) * 3.0)]).astype(np.float32)
    got = SR.all_gather([torch.from_numpy(x.reshape(-1))]).numpy().reshape(-1, 32)
    worst = (np.abs(got.astype(np.float64) - x) / (np.abs(x).max(axis=1, keepdims=True).astype(np.float64) / 16)).max()
    print(f"worst error / bound = {worst:.3f}")
    assert worst <= 1.0, worst
    xt = torch.from_numpy(x.reshape(-1))
    assert R.same(ops.mx_dequantize_shards_reference(ops.mx_quantize_reference(xt, 1), xt.numel(), torch.float32, 1),
                  torch.from_numpy(got.reshape(-1)))


# ------------------------------------------------------------------ the collectives on CPU tensors
@pytest.mark.parametrize("world", [2, 3, 4])
def test_collectives_on_cpu_tensors(world):
    ms = (1, 33, 513, 4113)
    res = launch(MS.collective_cases, world, args=("cpu", ms, tuple(R.DTYPES), ("sum", "avg")))
    for r, got in enumerate(res):
        assert len(got) == 3 * len(ms) * 3, sorted(got)
        bad = [k for k, v in got.items() if not v[0]]
        assert not bad, (r, bad)
        gathers = {k: v[1] for k, v in got.items() if k.startswith("ag/")}
        assert gathers == {k: v[1] for k, v in res[0].items() if k.startswith("ag/")}, r  # the same bits


def test_world_1_copies_bit_for_bit():
    got = launch(MS.world1_and_errors, 1, args=("cpu",))[0]
    assert len(got) == 7 + 14 and all(got.values()), got


def test_error_cases():
    for got in launch(MS.world1_and_errors, 2, args=("cpu",)):
        assert len(got) == 14 and all(got.values()), got
    with pytest.raises(ValueError, match="'max'"):
        ops.mx_fold_reference(torch.zeros(33 * 16, dtype=torch.uint8), 1, 32, torch.float32, "max")
    with pytest.raises(ValueError, match="528 bytes"):
        ops.mx_fold_reference(torch.zeros(33 * 32, dtype=torch.uint8), 1, 32)
    with pytest.raises(TypeError, match="float64"):
        ops.mx_quantize_shards_reference(torch.zeros(4, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="3 shards"):
        ops.mx_quantize_shards_reference(torch.zeros(4), 3)
    with pytest.raises(ValueError, match="1056 bytes"):
        ops.mx_dequantize_shards_reference(torch.zeros(33 * 16, dtype=torch.uint8), 33, torch.float32, 2)


def test_sharded_optimizer_with_compressed_wires_on_cpu_tensors():
    res = launch(MS.zero, 2, args=("cpu",))
    for got in res:
        assert got["buckets"] >= 2 and got["handles"] == ["CompressedWork"], got
        assert got["overlapped"] >= 1 and got["master_is_param_shard"], got
        for i in range(got["buckets"]):
            assert got[i][0] and got[i][1], (i, got[i])
        assert got["digest"] == res[0]["digest"]  # the same bits on both ranks
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    for kw in ({"grad_wire": "mxfp4"}, {"param_wire": "mxfp4"}):
        with pytest.raises(ValueError, match="mxfp4"):
            ShardedOptimizer(torch.nn.Linear(2, 2).parameters(), **kw)


# ------------------------------------------------------------------ the shard offsets, sanitized
def _build() -> str:
    exe = os.path.join(BUILD, "mx_shard_layout_check")
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(p) for p in (SRC, HDR)):
        return exe
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
           f"-I{CSRC}", SRC, "-o", exe + ".tmp"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-6000:]
    os.replace(exe + ".tmp", exe)
    return exe


def test_shard_layout_under_sanitizers():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    exe = _build()
    cases = [(m, w) for w in WORLDS for m in SHARDS + (65553, 1 << 20)]
    argv = [str(v) for c in cases for v in c]
    for args in ([], argv):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
        lines = r.stdout.strip().splitlines()
        assert lines[-1].split()[0] == "ok" and int(lines[-1].split()[1]) >= len(cases)
        for ln in lines[:-1]:  # "m world cb wire_bytes": the C++ layout and the Python one agree
            m, w, cb, nbytes = map(int, ln.split())
            assert ops.mx_shard_blocks(m) == cb and ops.mx_shard_wire_bytes(m, w) == nbytes, ln
