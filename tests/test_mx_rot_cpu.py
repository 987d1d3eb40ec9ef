"""The Hadamard rotation of the block-scaled wires without a GPU (docs/collectives.md "Hadamard rotation"):

* the transform itself: on integer-valued blocks, where every step is exact, R x is the explicit matrix product
  H diag(sigma) x and R^-1 R x is x bit for bit; the sign word; csrc/kernels/mx_rot.h through a stand-alone
  program under ASan + UBSan (tests/native/mx_rot_check.cpp);
* the plain-PyTorch twins of ops against the independent numpy reference (tests/_mx_rot_ref.py) byte for byte:
  every wire, dtype and layout, plain, with a residual and stochastic, the fold with 1..8 sources;
* the derived error bounds, and the measured benefit on heavy-tailed data under the caps the feature was
  accepted with;
* the three collectives on CPU tensors over the shm transport, the wrappers and the error cases.
"""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from pytorch_distributed_collective_communication_amd import ops
from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _mx_rot_ref as R
from tests import _workers_mx as M8
from tests import _workers_mx_rot as M
from tests._workers_mx_shard import shard_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
BUILD = os.path.join(ROOT, "build", "san")
SRC = os.path.join(ROOT, "tests", "native", "mx_rot_check.cpp")
HDRS = (os.path.join(CSRC, "kernels", "mx_rot.h"), os.path.join(CSRC, "kernels", "mx_sr.h"))

WIRES = tuple(R.WIRES)
SEED = M.RSEED
ROT = dict(rotation="hadamard", rotation_seed=SEED)
NUMELS = (1, 31, 32, 33, 63, 65, 511, 513, 4113)
SEEDS = (0, 1, 2, 12345, 1 << 32, SEED, (1 << 64) - 1)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _int_blocks(blocks, seed):
    return np.random.default_rng(seed).integers(-(1 << 18) + 1, 1 << 18, (blocks, 32)).astype(np.float32)


# ------------------------------------------------------------------ the transform
def test_rotation_is_the_signed_hadamard_matrix_on_integer_blocks():
    H = R.hadamard()
    assert np.array_equal(H @ H, 32 * np.eye(32)) and np.array_equal(H, H.T)
    for seed in SEEDS:
        sg = R.signs(seed)
        x = _int_blocks(64, seed % 1000)
        x[0] = 0
        x[1, :] = (1 << 18) - 1  # the largest sum: 32 (2^18 - 1) < 2^24, exact
        sigma = np.array([-1.0 if (sg >> j) & 1 else 1.0 for j in range(32)])
        want = (x.astype(np.float64) * sigma[None, :]) @ H.T
        assert np.abs(want).max() < 1 << 24
        got = R.forward(x, sg)
        assert np.array_equal(got.astype(np.float64), want), seed
        back = R.inverse(got, sg)
        nz = x != 0  # (a zero comes back as a zero of either sign: 0 - 0 and the sign word decide)
        assert np.array_equal(back, x) and np.array_equal(_bits(back)[nz], _bits(x)[nz]), seed
        tw = ops._mx_rot_forward(torch.from_numpy(x), sg)
        assert np.array_equal(_bits(tw.numpy()), _bits(got)), seed
        assert np.array_equal(_bits(ops._mx_rot_inverse(tw, sg).numpy()), _bits(back)), seed


def test_rotation_of_random_floats_rounds_like_the_reference():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((256, 32)) * np.exp(3 * rng.standard_normal((256, 32)))).astype(np.float32)
    x[0, 3], x[1, 7], x[2, 0] = np.inf, np.nan, -np.inf
    sg = R.signs(SEED)
    fwd = R.forward(x, sg)
    assert not np.isfinite(fwd[:3]).any() and np.isfinite(fwd[3:]).all()  # one inf / NaN reaches all 32 coefficients
    tw = ops._mx_rot_forward(torch.from_numpy(x), sg).numpy()
    assert np.array_equal(_bits(tw[3:]), _bits(fwd[3:])) and not np.isfinite(tw[:3]).any()
    assert np.array_equal(_bits(ops._mx_rot_inverse(torch.from_numpy(fwd[3:]), sg).numpy()), _bits(R.inverse(fwd[3:], sg)))


def test_sign_word():
    for seed in SEEDS:
        assert ops.mx_rotation_signs(seed) == R.signs(seed), seed
    assert len({R.signs(s) for s in SEEDS}) == len(SEEDS)
    assert R.signs(0) != int(R.SR.words(R.SR.key(0, 0), np.array([0], dtype=np.uint64))[0])  # no rank's stream
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError, match=r"2\^64"):
            ops.mx_rotation_signs(bad)
    with pytest.raises(TypeError):
        ops.mx_rotation_signs(1.0)


# ------------------------------------------------------------------ the shared header, under sanitizers
def _build() -> str:
    exe = os.path.join(BUILD, "mx_rot_check")
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(p) for p in (SRC,) + HDRS):
        return exe
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
           f"-I{CSRC}", SRC, "-o", exe + ".tmp"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-6000:]
    os.replace(exe + ".tmp", exe)
    return exe


def _ask(queries):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([_build()] + queries, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == (f"ok {len(queries)}" if queries else "ok"), lines[-1]
    return [[int(v, 16) for v in ln.split()] for ln in lines[:-1]]


def test_host_program_equals_the_reference():
    _ask([])  # the program's own check
    assert _ask([f"g:{s:x}" for s in SEEDS]) == [[R.signs(s)] for s in SEEDS]
    rng = np.random.default_rng(9)
    x = np.concatenate([_int_blocks(8, 3), (rng.standard_normal((8, 32)) * np.exp(3 * rng.standard_normal((8, 32))))
                        .astype(np.float32)])
    x[9, 0] = np.float32(2.0 ** -140)  # subnormals are kept
    for kind, fn in (("f", R.forward), ("i", R.inverse)):
        for seed in (0, SEED):
            got = _ask([f"{kind}:{seed:x}:" + ":".join(f"{int(b):x}" for b in _bits(row)) for row in x])
            assert np.array_equal(np.array(got, dtype=np.uint32), _bits(fn(x, R.signs(seed)))), (kind, seed)


# ------------------------------------------------------------------ the twins against the reference
@functools.lru_cache(maxsize=None)
def _inputs(wire, dtn):
    dt = R.DTYPES[dtn]
    return [("edge", torch.from_numpy(R.edge_tensor(wire)).to(dt))] + \
        [(f"n{n}", M8.rank_inputs(n, 2, 800 + n, dt)[1]) for n in NUMELS]


def _assert_wire(got, ref, nchunks, wire, what):
    assert R.same_wire(got.numpy(), ref, nchunks, wire), what


@pytest.mark.parametrize("dtn", list(R.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_twins_dealt_layout(wire, dtn):
    dt = R.DTYPES[dtn]
    for name, x in _inputs(wire, dtn):
        n = x.numel()
        for world in (1, 3):
            ref = R.quantize(R.f32(x), world, wire, SEED)
            _assert_wire(ops.mx_quantize_reference(x, world, wire=wire, **ROT), ref, world, wire, (name, world))
            got = ops.mx_dequantize_reference(torch.from_numpy(ref), n, dt, world, wire=wire, **ROT)
            assert R.same(got, R.dequantize(ref, n, world, wire, SEED, dt)), (name, world)
        sim = (np.random.default_rng(n).standard_normal(n) * 0.05).astype(np.float32)
        res = torch.from_numpy(sim.copy())
        for call in range(2):
            ref, sim = R.quantize(R.f32(x), 1, wire, SEED, res=sim)
            _assert_wire(ops.mx_quantize_reference(x, 1, wire=wire, residual=res, **ROT), ref, 1, wire, (name, "ef", call))
            assert R.same_residual(res, sim), (name, call)
        ref = R.quantize(R.f32(x), 3, wire, SEED, sr=(77, 5, 1 << 33))
        got = ops.mx_quantize_reference(x, 3, wire=wire, rounding="stochastic", seed=77, stream=5, index_offset=1 << 33, **ROT)
        _assert_wire(got, ref, 3, wire, (name, "sr"))
    # a different seed is a different rotation; no rotation is today's wire
    x = _inputs(wire, dtn)[-1][1]
    a = ops.mx_quantize_reference(x, 1, wire=wire, **ROT)
    assert not torch.equal(a, ops.mx_quantize_reference(x, 1, wire=wire, rotation="hadamard", rotation_seed=SEED + 1))
    assert torch.equal(ops.mx_quantize_reference(x, 1, wire=wire, rotation=None, rotation_seed=SEED),
                       ops.mx_quantize_reference(x, 1, wire=wire))


@pytest.mark.parametrize("dtn", list(R.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_twins_shard_layout(wire, dtn):
    dt = R.DTYPES[dtn]
    for W in (1, 3, 8):
        for m in (1, 5, 33, 96, 513):
            x = shard_inputs(m, max(W, 2), 800 + m, dt)[1][:W * m].clone()
            if m == 513:
                x[-513:] = torch.from_numpy(R.edge_tensor(wire)[:513]).to(dt)
            ref = R.quantize_shards(R.f32(x), W, wire, SEED)
            _assert_wire(ops.mx_quantize_shards_reference(x, W, wire=wire, **ROT), ref, W, wire, (W, m))
            got = ops.mx_dequantize_shards_reference(torch.from_numpy(ref), m, dt, W, wire=wire, **ROT)
            assert R.same(got, R.dequantize_shards(ref, m, W, wire, SEED, dt)), (W, m)
            sim = (np.random.default_rng(m).standard_normal(W * m) * 0.05).astype(np.float32)
            res = torch.from_numpy(sim.copy())
            ref, sim = R.quantize_shards(R.f32(x), W, wire, SEED, res=sim)
            _assert_wire(ops.mx_quantize_shards_reference(x, W, wire=wire, residual=res, **ROT), ref, W, wire, (W, m, "ef"))
            assert R.same_residual(res, sim), (W, m)
            ref = R.quantize_shards(R.f32(x), W, wire, SEED, sr=(9, 2, 7))
            got = ops.mx_quantize_shards_reference(x, W, wire=wire, rounding="stochastic", seed=9, stream=2, index_offset=7, **ROT)
            _assert_wire(got, ref, W, wire, (W, m, "sr"))


@pytest.mark.parametrize("nsrc", range(1, 9))
@pytest.mark.parametrize("wire", WIRES)
def test_twins_fold(wire, nsrc):
    for n in (33, 4113):
        xs = M8.rank_inputs(n, nsrc, 840 + nsrc)
        if n == 4113:
            xs[nsrc - 1][:1024] = torch.from_numpy(R.edge_tensor(wire)[:1024])
        w = np.concatenate([R.quantize(R.f32(x), 1, wire, SEED) for x in xs])
        for op in ("sum", "avg"):
            for dt in R.DTYPES.values():
                got = ops.mx_fold_reference(torch.from_numpy(w), nsrc, n, dt, op, wire=wire, **ROT)
                assert R.same(got, R.fold(w, nsrc, n, op, wire, SEED, dt)), (n, op, dt)
        # the owner stage takes no rotation: mx_reduce on rotated chunks, then the rotated dequantize
        red = ops.mx_reduce_reference(torch.from_numpy(w), nsrc, "sum", wire=wire)
        assert R.same_wire(red.numpy(), R.reduce(w, nsrc, "sum", wire), 1, wire)


def test_partial_block_round_trip_needs_the_padding_coefficients():
    # 33 elements: the second block holds one element and 31 padding zeros, whose rotated coefficients are not zero
    for wire in WIRES:
        x = M8.rank_inputs(33, 2, 3)[0]
        w = ops.mx_quantize_reference(x, 1, wire=wire, **ROT)
        y = ops.mx_dequantize_reference(w, 33, wire=wire, **ROT)
        assert R.same(y, R.dequantize(R.quantize(R.f32(x), 1, wire, SEED), 33, 1, wire, SEED))
        q, _ = R.WIRES[wire].split(w.numpy(), 1)
        assert q[1].any() and not q[2].any()  # payload in the padding positions of block 1; block 2 is padding
        assert abs(float(y[32]) - float(x[32])) <= abs(float(x[32])) / 3 * 1.001


# ------------------------------------------------------------------ bounds and benefit
def _data(kind, shape, rng):
    g = rng.standard_normal(shape)
    return (g * np.exp(rng.standard_normal(shape)) if kind == "lognormal" else g).astype(np.float32)


@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_derived_bounds(world):
    """With t = R x and c = 16 (FP8, FP6) or 3 (FP4): one nearest quantization errs by at most amax(t) / c per
    coefficient; after the inverse the error of an element is the signed mean of 32 of those, so |err_j| <=
    amax(t) / c and ||err||_2 <= amax(t) / c per block, times (1 + 2^-10) for the f32 roundings of the two
    butterflies. Reduce-scatter of W ranks: the sum of the ranks' bounds. Derived, not measured; fixed seed, every
    block has amax >= 2^-100, no element is excluded. Worst shares of the bound seen here over W = 2, 3, 4, 8, normal
    and log-normal halves together (per element / per block): one quantization FP8 0.161 / 0.342, FP4 0.131 / 0.252,
    FP6 0.158 / 0.333; reduce-scatter per element FP8 0.051 .. 0.118, FP4 0.041 .. 0.109, FP6 0.056 .. 0.104."""
    rng = np.random.default_rng(70 + world)
    blocks = 256
    slack = 1 + 2.0 ** -10
    for wire in WIRES:
        c = R.BOUND_C[wire]
        xs = [np.concatenate([_data("normal", (blocks // 2, 32), rng), _data("lognormal", (blocks // 2, 32), rng)])
              for _ in range(world)]
        sg = R.signs(SEED)
        bound = np.zeros(blocks)
        for x in xs:
            assert np.abs(x).max(axis=1).min() >= 2.0 ** -100
            bound += np.abs(R.forward(x, sg)).max(axis=1).astype(np.float64) / c * slack
        x0 = xs[0]
        b0 = np.abs(R.forward(x0, sg)).max(axis=1).astype(np.float64) / c * slack
        y = ops.mx_dequantize_reference(ops.mx_quantize_reference(torch.from_numpy(x0.reshape(-1)), 1, wire=wire, **ROT),
                                        x0.size, wire=wire, **ROT).numpy().reshape(blocks, 32)
        err = y.astype(np.float64) - x0
        el, l2 = float((np.abs(err) / b0[:, None]).max()), float((np.sqrt((err ** 2).sum(axis=1)) / b0).max())
        ts = [torch.from_numpy(x.reshape(-1)) for x in xs]
        m = blocks * 32 // world // 32 * 32
        outs = R.reduce_scatter([t[:m * world] for t in ts], "sum", wire, SEED)
        got = torch.cat(outs).numpy().astype(np.float64)
        exact = np.sum([x.reshape(-1)[:m * world].astype(np.float64) for x in xs], axis=0)
        rs = float((np.abs(got - exact) / np.repeat(bound, 32)[:m * world]).max())
        print(f"world {world} {wire}: one quantization {el:.3f} per element, {l2:.3f} per block; reduce-scatter {rs:.3f}")
        assert el <= 1.0 and l2 <= 1.0 and rs <= 1.0, (wire, el, l2, rs)


def _nmse(x, wire, **kw):
    w = ops.mx_quantize_reference(x, 1, wire=wire, **kw)
    y = ops.mx_dequantize_reference(w, x.numel(), wire=wire, **kw)
    return float(((y.double() - x.double()) ** 2).sum() / (x.double() ** 2).sum())


def test_benefit_on_heavy_tailed_data():
    """NMSE with rotation / NMSE without on 65536 elements, fixed seed. The caps: <= 0.75 on randn * exp(randn) for
    mxfp4_e2m1 and mxfp6_e2m3, <= 1.25 on randn for every wire. The references give (log-normal, normal):
    mxfp8_e4m3 1.072, 0.988; mxfp4_e2m1 0.496, 1.055; mxfp6_e2m3 0.531, 0.983."""
    rng = np.random.default_rng(20261021)
    heavy = torch.from_numpy(_data("lognormal", 65536, rng))
    normal = torch.from_numpy(_data("normal", 65536, rng))
    for wire in WIRES:
        h = _nmse(heavy, wire, **ROT) / _nmse(heavy, wire)
        g = _nmse(normal, wire, **ROT) / _nmse(normal, wire)
        print(f"{wire}: rotated / plain NMSE: log-normal {h:.3f}, normal {g:.3f}")
        assert g <= 1.25, (wire, g)
        if wire != "mxfp8_e4m3":
            assert h <= 0.75, (wire, h)


# ------------------------------------------------------------------ the collectives on CPU tensors, the wrappers
@pytest.mark.parametrize("world", [2, 3, 4])
def test_collectives_on_cpu_tensors(world):
    numels = (33, 513)
    dtypes = ("float32", "bfloat16") if world == 2 else ("float32",)
    res = launch(M.collective_cases, world, args=("cpu", numels, dtypes))
    for r, got in enumerate(res):
        assert len(got) == len(WIRES) * len(dtypes) * len(numels) * M.CASES_PER_SIZE, sorted(got)
        bad = [k for k, v in got.items() if not v[0]]
        assert not bad, (r, bad)
        same = {k: v[1] for k, v in got.items() if not k.startswith("rs")}  # identical bits on every rank
        assert same == {k: v[1] for k, v in res[0].items() if not k.startswith("rs")}, r


def test_world_1_and_error_cases():
    got = launch(M.world1_and_errors, 1, args=("cpu",))[0]
    assert len(got) == 3 + M.N_ERRORS and all(got.values()), got
    for got in launch(M.world1_and_errors, 2, args=("cpu",)):
        assert len(got) == M.N_ERRORS and all(got.values()), got


def test_wrappers_on_cpu_tensors():
    for got in launch(M.bucketer, 2, args=("cpu", "mxfp4_e2m1", "ef")):
        assert got["buckets"] >= 2 and len(got["steps"]) == 3, got
        assert all(step[i][0] for step in got["steps"] for i in range(got["buckets"])), got
    for got in launch(M.zero, 2, args=("cpu", "mxfp4_e2m1", "mxfp6_e2m3", "ef")):
        assert got["buckets"] >= 2 and len(got["steps"]) == 3 and got["state_keys"] == [], got
        assert all(step[i][0] and step[i][1] for step in got["steps"] for i in range(got["buckets"])), got


def test_wrong_arguments_raise():
    x = torch.zeros(64)
    w = torch.zeros(17 * 16, dtype=torch.uint8)
    fns = (lambda **k: ops.mx_quantize_reference(x, 1, wire="mxfp4_e2m1", **k),
           lambda **k: ops.mx_quantize_shards_reference(x, 2, wire="mxfp4_e2m1", **k),
           lambda **k: ops.mx_dequantize_reference(w, 64, wire="mxfp4_e2m1", **k),
           lambda **k: ops.mx_dequantize_shards_reference(w, 64, wire="mxfp4_e2m1", **k),
           lambda **k: ops.mx_fold_reference(w, 1, 64, wire="mxfp4_e2m1", **k),
           lambda **k: ops.mx_quantize(x, wire="mxfp4_e2m1", **k), lambda **k: ops.mx_quantize_shards(x, 2, wire="mxfp4_e2m1", **k),
           lambda **k: ops.mx_dequantize(w, 64, wire="mxfp4_e2m1", **k),
           lambda **k: ops.mx_dequantize_shards(w, 64, wire="mxfp4_e2m1", **k),
           lambda **k: ops.mx_fold(w, 1, 64, wire="mxfp4_e2m1", **k))
    for fn in fns:
        with pytest.raises(ValueError, match="unknown rotation 'haar'.*hadamard"):
            fn(rotation="haar")
        with pytest.raises(ValueError, match=r"rotation_seed must be in \[0, 2\^64\)"):
            fn(rotation="hadamard", rotation_seed=1 << 64)
        with pytest.raises(ValueError, match=r"rotation_seed must be in \[0, 2\^64\)"):
            fn(rotation_seed=-1)
        with pytest.raises(TypeError, match="rotation_seed must be an int"):
            fn(rotation="hadamard", rotation_seed=True)
    for fn in (ops.mx_reduce, ops.mx_reduce_reference):  # the owner stage takes no rotation
        with pytest.raises(TypeError, match="rotation"):
            fn(w, 1, wire="mxfp4_e2m1", rotation="hadamard")
    from pytorch_distributed_collective_communication_amd.parallel import ddp
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    lin = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="rotation needs a compressed wire"):
        ddp.GradBucketer(lin, rotation="hadamard")
    with pytest.raises(ValueError, match="unknown rotation 'haar'"):
        ddp.GradBucketer(lin, wire="mxfp4_e2m1", rotation="haar")
    with pytest.raises(ValueError, match="grad_rotation needs a grad_wire"):
        ShardedOptimizer(lin.parameters(), param_wire="mxfp6_e2m3", grad_rotation="hadamard")
    with pytest.raises(ValueError, match="param_rotation needs a param_wire"):
        ShardedOptimizer(lin.parameters(), grad_wire="mxfp4_e2m1", param_rotation="hadamard")
    with pytest.raises(ValueError, match=r"2\^64"):
        ShardedOptimizer(lin.parameters(), grad_wire="mxfp4_e2m1", grad_rotation="hadamard", rotation_seed=1 << 64)
