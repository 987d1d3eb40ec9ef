"""Stochastic rounding on the block-scaled wires (docs/collectives.md "Stochastic rounding"), everything
that needs no GPU: the `ops.*_reference` twins against the independent numpy reference
tests/_mx_sr_ref.py bit for bit, csrc/kernels/mx_sr.h through the stand-alone program
tests/native/mx_sr_check.cpp (ASan + UBSan) against the same reference, the properties of the contract,
the unbiasedness cap, the collectives over the shm transport against a single-process simulation,
world 1, every error, and the seeds of the two training wrappers.
"""
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from pytorch_distributed_collective_communication_amd import ops
from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _mx_ef_ref as E
from tests import _mx_sr_ref as S
from tests import _workers_mx_sr as M
from tests._workers_mx import rank_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
BUILD = os.path.join(ROOT, "build", "san")
SRC = os.path.join(ROOT, "tests", "native", "mx_sr_check.cpp")
HDR = os.path.join(CSRC, "kernels", "mx_sr.h")

WIRES = tuple(S.WIRES)
NUMELS = (1, 31, 33, 513, 4113)
SHARDS = (1, 33, 512)
WORLDS = (1, 2, 3, 8)
SR = dict(rounding="stochastic")


@functools.lru_cache(maxsize=None)
def _x(n, dtn, seed=0):
    return rank_inputs(n, 2, 700 + n + seed, S.DTYPES[dtn])[1]


def _assert_wire(R, got, ref, nchunks, what):
    assert R.same_wire(got.numpy(), ref, nchunks), what


# ------------------------------------------------------------------ the references, bit for bit
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("dtn", list(S.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_quantize_reference(wire, dtn, world):
    R = S.WIRES[wire]
    differs = 0
    for n in NUMELS:
        x = _x(n, dtn)
        keep = x.clone()
        seed, stream = (1 << 63) + n, 2 * world + 1
        want = S.quantize(R.f32(x), world, wire, seed, stream)
        got = ops.mx_quantize_reference(x, world, wire=wire, seed=seed, stream=stream, **SR)
        assert np.array_equal(got.numpy(), want), (wire, dtn, world, n)
        assert torch.equal(x.view(torch.uint8), keep.view(torch.uint8))
        differs += int((want != R.quantize(R.f32(x), world)).sum())
    assert differs  # (it is not the nearest wire)


@pytest.mark.parametrize("W", WORLDS)
@pytest.mark.parametrize("dtn", list(S.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_quantize_shards_reference(wire, dtn, W):
    R = S.WIRES[wire]
    for m in SHARDS:
        x = _x(W * m, dtn, seed=7)
        want = S.quantize_shards(R.f32(x), W, wire, 99 + m, 4, index_offset=m)
        got = ops.mx_quantize_shards_reference(x, W, wire=wire, seed=99 + m, stream=4, index_offset=m, **SR)
        assert np.array_equal(got.numpy(), want), (wire, dtn, W, m)


@pytest.mark.parametrize("wire", WIRES)
def test_both_layouts_draw_the_same_word_for_the_same_element(wire):
    # 8 shards of 512 elements are the same bytes in both layouts: so are they rounded stochastically
    x = _x(8 * 512, "float32", seed=3)
    a = ops.mx_quantize_reference(x, 8, wire=wire, seed=5, stream=1, **SR)
    b = ops.mx_quantize_shards_reference(x, 8, wire=wire, seed=5, stream=1, **SR)
    assert torch.equal(a, b)
    # and element i of shard r is rounded as element r m + i of the tensor, wherever its block starts
    m = 33
    x = _x(3 * m, "float32", seed=4)
    w = S.quantize_shards(S.WIRES[wire].f32(x), 3, wire, 5, 1)
    for r in range(3):
        alone = S.quantize(S.WIRES[wire].f32(x)[r * m:(r + 1) * m], 1, wire, 5, 1, index_offset=r * m)
        assert np.array_equal(w[r * alone.size:(r + 1) * alone.size], alone)


@pytest.mark.parametrize("op", ["sum", "avg"])
@pytest.mark.parametrize("nsrc", list(range(1, 9)))
@pytest.mark.parametrize("wire", WIRES)
def test_reduce_reference(wire, nsrc, op):
    R = S.WIRES[wire]
    for n in (48 * 32, 4113):
        xs = rank_inputs(n, nsrc, 40 + nsrc)
        xs[nsrc - 1][:1024] = torch.from_numpy(S.R4.edge_tensor()[0][:1024])  # NaN, inf and zero blocks
        w = np.concatenate([R.quantize(R.f32(x), 1) for x in xs])
        want = S.reduce(w, nsrc, op, wire, 31 + n, 2 * nsrc + 1)
        got = ops.mx_reduce_reference(torch.from_numpy(w), nsrc, op, wire=wire, seed=31 + n, stream=2 * nsrc + 1, **SR)
        _assert_wire(R, got, want, 1, (wire, nsrc, op, n))
        assert (R.split(want, 1)[1] == 255).any()  # the NaN blocks are there


@pytest.mark.parametrize("dtn", list(S.DTYPES))
@pytest.mark.parametrize("edges", ["mxfp8_e4m3", "mxfp4_e2m1"])
@pytest.mark.parametrize("wire", WIRES)
def test_edge_tensors(wire, edges, dtn):
    """NaN, inf, zero blocks, both clamps of e and the top of the range: the edge sets of both formats."""
    R = S.WIRES[wire]
    xe, names = S.WIRES[edges].edge_tensor()
    x = torch.from_numpy(xe).to(S.DTYPES[dtn])
    want = S.quantize(R.f32(x), 1, wire, 3, 0)
    got = ops.mx_quantize_reference(x, 1, wire=wire, seed=3, **SR)
    _assert_wire(R, got, want, 1, (wire, edges, dtn))
    # scale bytes, NaN / inf blocks and all-zero blocks are those of the nearest wire
    near = R.quantize(R.f32(x), 1)
    assert np.array_equal(R.split(want, 1)[1], R.split(near, 1)[1])
    q, s = R.split(want, 1)
    xb = R.f32(x).reshape(-1, 32)
    special, zero = ~np.isfinite(xb).all(axis=1), ~xb.any(axis=1)
    assert special.any() and zero.any()
    assert not q[:xb.shape[0]][special | zero].any() and (s[:xb.shape[0]][special] == 255).all()
    # and the reduce of that wire alone gives back its values: every one is on the grid of its block's new
    # scale (a block that dequantizes to an inf or a NaN comes back as a NaN block)
    back = ops.mx_reduce_reference(torch.from_numpy(want), 1, "sum", wire=wire, seed=8, stream=1, **SR).numpy()
    a, b = R.d_blocks(*R.split(back, 1)), R.d_blocks(*R.split(want, 1))
    finite = np.isfinite(b).all(axis=1)
    assert finite.sum() > 50 and np.array_equal(a[finite], b[finite]) and np.isnan(a[~finite]).all()


# ------------------------------------------------------------------ the header, through its host program
def _build() -> str:
    exe = os.path.join(BUILD, "mx_sr_check")
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


def _ask(queries, batch=4096):
    """The host program's answers to `queries`, as ints."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    exe = _build()
    out = []
    for i in range(0, len(queries), batch):
        part = queries[i:i + batch]
        r = subprocess.run([exe] + part, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
        lines = r.stdout.strip().splitlines()
        assert lines[-1] == f"ok {len(part)}", lines[-1]
        out += [int(v) for v in lines[:-1]]
    assert len(out) == len(queries)
    return out


def test_host_program_self_check():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok" and "runtime error" not in r.stderr, r.stdout + r.stderr


@pytest.mark.parametrize("wire", WIRES)
def test_host_program_codes_equal_the_reference(wire):
    """Every grid point, every midpoint, the f32 neighbours of every grid point and subnormal targets down to
    2^-40, each with u in {0, 1, T - 1, T, T + 1, 2^32 - 1}."""
    kind = "e4m3" if wire == "mxfp8_e4m3" else "e2m1"
    vals = S.probe_values(wire)
    assert (np.abs(vals) == np.float32(2.0 ** -40)).any() and (np.abs(vals) == S.GRIDS[wire][-1]).any()
    _, T = S.split(np.abs(vals.astype(np.float64)), wire)
    queries, want = [], []
    for v, bits, t in zip(vals, S.f32_bits(vals), T):
        for u in S.probe_words(t):
            queries.append(f"{kind}:{int(bits):x}:{u:x}")
            want.append(int(S.code_of(np.array([np.float64(v)]), np.array([u], dtype=np.uint64), wire)[0]))
    assert len(queries) > 6 * 4 * (S.GRIDS[wire].size - 1)
    assert _ask(queries) == want


def test_host_program_words_equal_the_reference():
    seeds = (0, 1, 1234, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 0xC0FFEE12345678)
    streams = (0, 1, 15, (1 << 32) - 1)
    xs = (0, 1, 0x9E3779B9, (1 << 32) - 1)
    idx = (0, 1, 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 33) - 1, 7 << 32, (1 << 64) - 1)
    assert _ask([f"mix:{x:x}" for x in xs]) == [int(S.mix(x)) for x in xs]
    assert _ask([f"key:{s:x}:{t:x}" for s in seeds for t in streams]) == [S.key(s, t) for s in seeds for t in streams]
    assert [ops.mx_sr_key(s, t) for s in seeds for t in streams] == [S.key(s, t) for s in seeds for t in streams]
    for k in (0, S.key(1234, 3)):
        assert _ask([f"word:{k:x}:{i:x}" for i in idx]) == [int(v) for v in S.words(k, np.array(idx, dtype=np.uint64))]


# ------------------------------------------------------------------ properties of the contract
@pytest.mark.parametrize("wire", WIRES)
def test_values_on_the_grid_never_move(wire):
    R = S.WIRES[wire]
    g = S.GRIDS[wire].astype(np.float32)
    rng = np.random.default_rng(5)
    # blocks whose amax is the format's largest magnitude (e = 0) hold grid points of both signs
    xb = rng.choice(np.concatenate([g, -g]), size=(64, 32)).astype(np.float32)
    xb[:, 0] = g[-1]
    x = torch.from_numpy(xb.reshape(-1).copy())
    near = R.quantize(xb.reshape(-1), 1)
    for seed in range(4):
        got = ops.mx_quantize_reference(x, 1, wire=wire, seed=seed, **SR).numpy()
        assert np.array_equal(got, S.quantize(xb.reshape(-1), 1, wire, seed))
        # (nearest writes +0 for -0 on the FP8 wire only in its sign bit: compare values)
        assert np.array_equal(R.d_blocks(*R.split(got, 1)), R.d_blocks(*R.split(near, 1)))
        assert np.array_equal(R.d_blocks(*R.split(got, 1)).reshape(-1)[:x.numel()], xb.reshape(-1))


@pytest.mark.parametrize("wire", WIRES)
def test_the_count_of_up_is_exact(wire):
    """For 64 fixed s and u = j 2^20, j = 0 .. 4095, "up" happens exactly ceil(T / 2^20) times."""
    kind = "e4m3" if wire == "mxfp8_e4m3" else "e2m1"
    rng = np.random.default_rng(11)
    top = S.GRIDS[wire][-1]
    s = np.concatenate([rng.uniform(0, top, 40), np.ldexp(rng.uniform(1, 2, 24), -rng.integers(1, 20, 24))])
    s = s.astype(np.float32)
    s = s[s < top]
    assert s.size == 64
    lo, T = S.split(s.astype(np.float64), wire)
    queries = [f"{kind}:{int(b):x}:{j << 20:x}" for b in S.f32_bits(s) for j in range(4096)]
    got = np.array(_ask(queries, batch=8192)).reshape(64, 4096)
    ref = S.code_of(np.repeat(s.astype(np.float64), 4096), np.tile(np.arange(4096, dtype=np.uint64) << 20, 64), wire)
    assert np.array_equal(got, ref.reshape(64, 4096))
    up = (got != lo[:, None]).sum(axis=1)
    assert np.array_equal(up, -(-T.astype(np.int64) // (1 << 20))), (up, T)
    assert (up > 0).any() and (up < 4096).all()


def test_streams_and_seeds_give_other_words():
    idx = np.arange(4096, dtype=np.uint64)
    base = S.words(S.key(1234, 0), idx)
    for k in (S.key(1234, 1), S.key(1235, 0), S.key(1234 + (1 << 32), 0)):
        other = S.words(k, idx)
        assert (other != base).mean() > 0.99
    x = _x(4113, "float32")
    a = ops.mx_quantize_reference(x, 1, seed=1234, stream=0, **SR)
    assert torch.equal(a, ops.mx_quantize_reference(x, 1, seed=1234, stream=0, **SR))  # the same bits again
    assert not torch.equal(a, ops.mx_quantize_reference(x, 1, seed=1234, stream=1, **SR))
    assert not torch.equal(a, ops.mx_quantize_reference(x, 1, seed=1235, stream=0, **SR))
    # the bits of the words look like coin flips
    bits = ((base[:, None] >> np.arange(32, dtype=np.uint64)) & 1).mean(axis=0)
    assert (np.abs(bits - 0.5) < 0.05).all(), bits


@pytest.mark.parametrize("wire", WIRES)
def test_index_offset_across_the_high_word(wire):
    R = S.WIRES[wire]
    x = _x(128, "float32", seed=9)
    off = (1 << 32) - 48
    want = S.quantize(R.f32(x), 1, wire, 77, 5, index_offset=off)
    got = ops.mx_quantize_reference(x, 1, wire=wire, seed=77, stream=5, index_offset=off, **SR)
    assert np.array_equal(got.numpy(), want)
    # the words past the boundary come from the key of the next high word, not from a wrapped index
    k = S.key(77, 5)
    assert not np.array_equal(S.words(k, np.arange(1 << 32, (1 << 32) + 80, dtype=np.uint64)),
                              S.words(k, np.arange(80, dtype=np.uint64)))


# ------------------------------------------------------------------ unbiasedness
CALLS = 256


def _mean_error_ratio(wire, x, quantize):
    """max over elements of |mean_t D(Q_t(x)) - x| / (G 2^e_b sqrt(ln(2 n / 1e-6) / (2 T)))."""
    R = S.WIRES[wire]
    n = x.size
    mean = np.zeros(n, dtype=np.float64)
    e = None
    for t in range(CALLS):
        w = quantize(t).numpy()
        q, s = R.split(w, 1)
        e = s.astype(np.int64) - 127
        mean += R.d_blocks(q, s).reshape(-1)[:n].astype(np.float64)
    mean /= CALLS
    bound = S.STEP[wire] * np.ldexp(1.0, np.repeat(e, 32)[:n]) * math.sqrt(math.log(2 * n / 1e-6) / (2 * CALLS))
    return float((np.abs(mean - x.astype(np.float64)) / bound).max())


@pytest.mark.parametrize("kind", ["normal", "lognormal"])
@pytest.mark.parametrize("wire", WIRES)
def test_the_mean_of_many_calls_is_the_input(wire, kind):
    """Per element, |mean over 256 calls (seed 1234, stream t) of D(Q(x)) - x| stays within
    G 2^e_b sqrt(ln(2 n / 1e-6) / (2 T)), G = 32 (FP8) or 2 (FP4) -- Hoeffding for errors within one grid
    step, all 4096 elements at once with probability 1 - 1e-6. No element is left out. Nearest rounding
    keeps its error at every T and leaves the bound. Measured with these references, as fractions of the
    bound: stochastic 0.40 (FP8 normal), 0.38 (FP8 log-normal), 0.35 (FP4 normal), 0.32 (FP4 log-normal);
    nearest 2.35, 2.37, 2.36, 2.33."""
    x = E.bound_series(kind, n=4096, T=1)[0]
    xt = torch.from_numpy(x)
    sr = _mean_error_ratio(wire, x, lambda t: ops.mx_quantize_reference(xt, 1, wire=wire, seed=1234, stream=t, **SR))
    near = _mean_error_ratio(wire, x, lambda t: ops.mx_quantize_reference(xt, 1, wire=wire))
    print(f"{wire} {kind}: stochastic {sr:.3f}, nearest {near:.3f} (of the bound)")
    assert sr <= 1.0, sr
    assert near > 1.0, near


@pytest.mark.parametrize("wire", WIRES)
def test_averaging_over_ranks_is_reported(wire):
    """Printed, not asserted against a threshold: the RMS error of the mean of 8 quantizations of the same x
    (n = 16384, streams 0 .. 7) next to that of nearest rounding, which gains nothing from the 8. Measured
    with these references: FP8 0.0136 against 0.0270 (one stochastic call: 0.0378), FP4 0.0582 against 0.1145
    (one call: 0.1649), normal x."""
    x = E.bound_series("normal", n=16384, T=1)[0]
    xt = torch.from_numpy(x)
    d = [ops.mx_dequantize_reference(ops.mx_quantize_reference(xt, 1, wire=wire, seed=1234, stream=k, **SR), x.size,
                                     wire=wire).numpy().astype(np.float64) for k in range(8)]
    near = ops.mx_dequantize_reference(ops.mx_quantize_reference(xt, 1, wire=wire), x.size, wire=wire).numpy()
    rms = lambda v: float(np.sqrt(np.mean((v - x.astype(np.float64)) ** 2)))  # noqa: E731
    one, mean8, n8 = rms(d[0]), rms(np.mean(d, axis=0)), rms(near.astype(np.float64))
    print(f"{wire}: rms error of one stochastic call {one:.4f}, of the mean of 8 {mean8:.4f}, nearest {n8:.4f}")
    assert np.isfinite([one, mean8, n8]).all()


# ------------------------------------------------------------------ errors
def test_rounding_errors_in_ops():
    x = torch.zeros(64)
    w = torch.zeros(17 * 16, dtype=torch.uint8)
    calls = [lambda **k: ops.mx_quantize_reference(x, 1, **k), lambda **k: ops.mx_quantize_shards_reference(x, 2, **k),
             lambda **k: ops.mx_reduce_reference(w, 1, wire="mxfp4_e2m1", **k),
             # the GPU entry points check before they look for the extension or a device
             lambda **k: ops.mx_quantize(x, 1, **k), lambda **k: ops.mx_quantize_shards(x, 2, **k),
             lambda **k: ops.mx_reduce(w, 1, wire="mxfp4_e2m1", **k)]
    for i, fn in enumerate(calls):
        with pytest.raises(ValueError, match="unknown rounding 'up'"):
            fn(rounding="up")
        for seed in (-1, 1 << 64):
            with pytest.raises(ValueError, match=r"seed must be in \[0, 2\^64\)"):
                fn(seed=seed, **SR)
        with pytest.raises(ValueError, match=r"stream must be in \[0, 2\^32\)"):
            fn(stream=1 << 32, **SR)
        with pytest.raises(TypeError, match="seed must be an int"):
            fn(seed=1.5, **SR)
        res = torch.zeros(512 if i % 3 == 2 else 64)
        with pytest.raises(ValueError, match="alternatives"):
            fn(residual=res, **SR)
        if i % 3 != 2:
            with pytest.raises(ValueError, match="index_offset"):
                fn(index_offset=(1 << 64) - 63, **SR)
            with pytest.raises(ValueError, match="index_offset"):
                fn(index_offset=-1, **SR)
    with pytest.raises(TypeError):
        ops.mx_quantize_reference(x, 1, "mxfp8_e4m3", None, "stochastic")  # keyword-only


def test_wrappers_refuse_what_they_cannot_do():
    from pytorch_distributed_collective_communication_amd.parallel import ddp
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    lin = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="rounding='stochastic' needs a compressed wire"):
        ddp.GradBucketer(lin, rounding="stochastic")
    with pytest.raises(ValueError, match="alternatives"):
        ddp.GradBucketer(lin, wire="mxfp4_e2m1", rounding="stochastic", error_feedback=True)
    with pytest.raises(ValueError, match="unknown rounding"):
        ddp.GradBucketer(lin, wire="mxfp4_e2m1", rounding="floor")
    with pytest.raises(ValueError, match="seed"):
        ddp.GradBucketer(lin, wire="mxfp4_e2m1", rounding="stochastic", seed=1 << 64)
    with pytest.raises(ValueError, match="grad_rounding='stochastic' needs a grad_wire"):
        ShardedOptimizer(lin.parameters(), grad_rounding="stochastic", param_wire="mxfp8_e4m3")
    with pytest.raises(ValueError, match="alternatives"):
        ShardedOptimizer(lin.parameters(), grad_wire="mxfp4_e2m1", grad_rounding="stochastic", grad_error_feedback=True)
    with pytest.raises(ValueError, match="unknown grad_rounding"):
        ShardedOptimizer(lin.parameters(), grad_wire="mxfp4_e2m1", grad_rounding="floor")
    with pytest.raises(ValueError, match="grad_seed"):
        ShardedOptimizer(lin.parameters(), grad_wire="mxfp4_e2m1", grad_rounding="stochastic", grad_seed=-1)


# ------------------------------------------------------------------ the collectives over shm
def _check_collectives(res, n_cases):
    for r, got in enumerate(res):
        assert len(got) == n_cases, sorted(got)
        bad = [k for k, v in got.items() if not v[0]]
        assert not bad, (r, bad)
        same = {k: v[1] for k, v in got.items() if not k.startswith("rs/")}  # identical bits on every rank
        assert same == {k: v[1] for k, v in res[0].items() if not k.startswith("rs/")}, r


@pytest.mark.parametrize("world", [2, 3, 4])
def test_collectives_on_cpu_tensors(world):
    numels = (33, 513, 4113)
    dtypes = tuple(S.DTYPES) if world == 2 else ("float32", "bfloat16")
    res = launch(M.collective_cases, world, args=("cpu", numels, dtypes))
    _check_collectives(res, len(WIRES) * len(dtypes) * len(numels) * 4)


N_ERRORS = 3 * 4 + 3 + 1


def test_world_1_and_error_cases():
    got = launch(M.world1_and_errors, 1, args=("cpu",))[0]
    assert len(got) == 3 + N_ERRORS and all(got.values()), got
    for got in launch(M.world1_and_errors, 2, args=("cpu",)):
        assert len(got) == N_ERRORS and all(got.values()), got


# ------------------------------------------------------------------ the training wrappers on CPU tensors
def _check_bucketer(res):
    for got in res:
        nb = got["buckets"]
        assert nb >= 2 and got["no_sync"] and got["steps_counted"] == 3, got
        first, again = got["runs"]
        for t, step in enumerate(first):
            for i in range(nb):
                assert step[i][0], (t, i, step[i])
                assert step[i][1] == res[0]["runs"][0][t][i][1]  # the same bits on every rank
        # the same gradients at steps 1 and 2, other seeds: other bits
        assert any(first[0][i][1] != first[1][i][1] for i in range(nb)), first
        assert again == first  # a rebuilt bucketer with the same seed repeats them


def test_grad_bucketer_with_stochastic_rounding_on_cpu_tensors():
    _check_bucketer(launch(M.bucketer, 2, args=("cpu", "mxfp4_e2m1")))


def _check_zero(res):
    for got in res:
        nb = got["buckets"]
        assert nb >= 2, got
        for t, step in enumerate(got["steps"]):
            for i in range(nb):
                assert step[i][0], (t, i, step[i])
            assert step["digest"] == res[0]["steps"][t]["digest"]  # replicas agree
        assert got["sd_step"] == 2 and got["counted"] == 3 and got["loaded_step"] == 2, got
        assert got["restored"] == got["original"], got  # step 3 after a reload, bit for bit
        assert got["old_checkpoint_loads_zero"] and got["no_sync"], got


def test_sharded_optimizer_with_stochastic_rounding_on_cpu_tensors():
    _check_zero(launch(M.zero, 2, args=("cpu",)))
