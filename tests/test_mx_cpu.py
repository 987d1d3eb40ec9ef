"""The block-scaled FP8 wire format `mxfp8_e4m3` without a GPU (docs/collectives.md "Compressed
all-reduce").

* `ops.mx_*_reference` (plain PyTorch) against tests/_mx_ref.py (numpy integer arithmetic): every
  branch of the quantizer, exact bytes and exact values;
* idempotence D(Q(D(w))) == D(w) and the derived error bound against an f64 sum;
* `all_reduce_compressed` on CPU tensors over the shm transport (worlds 2, 3, 4), world 1, the
  error cases;
* the layout header under ASan + UBSan (tests/native/mx_layout_check.cpp, a stand-alone program).

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
from tests import _workers_mx as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
BUILD = os.path.join(ROOT, "build", "san")
SRC = os.path.join(ROOT, "tests", "native", "mx_layout_check.cpp")
HDR = os.path.join(CSRC, "kernels", "mx_layout.h")

NUMELS = (1, 31, 32, 33, 511, 513, 4096 + 17, 65536 + 17, 70001)


def _f32_bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the edge set holds what it claims
def test_edge_blocks_cover_every_branch_of_the_quantizer():
    eb = R.edge_blocks()
    amax = {k: int((_f32_bits(v) & 0x7FFFFFFF).max()) for k, v in eb.items()}
    q = {k: R.q_blocks(v[None]) for k, v in eb.items()}
    scale = {k: int(s[0]) for k, (_, s) in q.items()}
    assert amax["zero"] == 0 and scale["zero"] == 127 and not q["zero"][0].any()
    # +0 and -0 both present, still the all-zero block
    assert set(_f32_bits(eb["pm_zero"]).tolist()) == {0, 0x80000000} and scale["pm_zero"] == 127
    assert not q["pm_zero"][0].any()
    for j in (-100, -20, 0, 7, 100):
        a, b = f"amax_448_2^{j}", f"amax_448_2^{j}_plus_ulp"
        assert amax[a] & 0x7FFFFF == 0x600000 and amax[b] == amax[a] + 1
        assert scale[a] == 127 + j and scale[b] == 128 + j  # the step of e
        assert (q[a][0] & 0x7F).max() == 0x7E and (q[b][0] & 0x7F).max() == 0x76  # 448 exactly; 224 one ulp above
    assert amax["mant_600000"] == 0x3FE00000 and scale["mant_600000"] == 127 - 8
    assert amax["mant_600001"] == 0x3FE00001 and scale["mant_600001"] == 127 - 7
    assert scale["mant_600001_negative"] == 127 - 7
    assert scale["amax_2^-120"] == 10 and scale["amax_2^-126"] == 10 and scale["amax_subnormal"] == 10  # the lower clamp
    assert amax["amax_subnormal"] < 0x00800000
    assert scale["amax_3e38"] == 247  # the upper end: e = 120
    assert np.isfinite(R.d_blocks(*q["amax_3e38"])).all()
    assert np.isnan(eb["one_nan"]).sum() == 1 and scale["one_nan"] == 255
    assert np.isinf(eb["one_inf"]).sum() == 1 and scale["one_inf"] == 255
    assert np.isnan(R.d_blocks(*q["one_nan"])).all() and np.isnan(R.d_blocks(*q["one_inf"])).all()
    # ties, FP8 subnormals and underflow after scaling (e = 0: the block is its own scaled value)
    t, (tq, ts) = eb["ties_and_subnormals"], q["ties_and_subnormals"]
    assert int(ts[0]) == 127
    d = R.d_blocks(tq, ts)[0]
    assert d[1] == 16 and d[2] == 20 and d[3] == 20 and d[4] == 24  # 17, 19, 21, 23: ties to even
    assert d[11] == 0 and d[13] == 2.0 ** -9 and d[14] == 0  # 2^-10 ties to 0; just above / below it
    assert d[15] == 2.0 ** -9 and d[16] == 2.0 ** -8  # the smallest subnormal; 3 2^-10 ties to even
    assert tq[0][20] == 0x80 and tq[0][21] == 0  # -0 keeps its sign next to a non-zero amax
    assert d[27] == 0 and t[27] != 0  # underflow after scaling
    # random data over 80 binades
    rb = R.random_binades(96, 11)
    ex = (_f32_bits(rb) >> 23) & 0xFF
    assert int(ex.max()) - int(ex[ex > 0].min()) >= 80


# ------------------------------------------------------------------ the references against each other
@pytest.mark.parametrize("world", [1, 3, 8])
def test_references_agree_on_the_edge_blocks(world):
    x, _ = R.edge_tensor()
    for dtn, dt in R.DTYPES.items():
        xt = torch.from_numpy(x).to(dt)
        want = R.quantize(R.f32(xt), world)
        got = ops.mx_quantize_reference(xt, world)
        assert got.dtype == torch.uint8 and got.numel() == ops.mx_wire_bytes(x.size, world) == want.size
        assert np.array_equal(got.numpy(), want), dtn  # every byte (both write 0 under a NaN block)
        for odt in R.DTYPES.values():
            d = ops.mx_dequantize_reference(got, x.size, odt, world)
            assert d.dtype == odt and R.same(d, R.dequantize(want, x.size, world, odt)), (dtn, odt)


@pytest.mark.parametrize("numel", NUMELS)
def test_references_agree_on_ragged_sizes(numel):
    for world in (1, 3, 8):
        x = M.rank_inputs(numel, 2, 77 + numel)[1]
        want = R.quantize(R.f32(x), world)
        got = ops.mx_quantize_reference(x, world).numpy()
        assert np.array_equal(got, want), (numel, world)
        # padding blocks (whole chunks at small sizes): scale 127, payload 0
        q, s = R.split(got, world)
        first_pad = -(-numel // 32)
        assert (s[first_pad:] == 127).all() and not q[first_pad:].any()
        if numel % 32:
            assert not q[first_pad - 1, numel % 32:].any()
        assert R.same(ops.mx_dequantize_reference(torch.from_numpy(got), numel, torch.float32, world),
                      R.dequantize(want, numel, world))


@pytest.mark.parametrize("nsrc", [1, 2, 3, 5, 8])
def test_reduce_reference_folds_in_source_order(nsrc):
    xs = M.rank_inputs(48 * 32, nsrc, 5 + nsrc)
    xs[0][:len(R.edge_tensor()[0])][:1024] = torch.from_numpy(R.edge_tensor()[0][:1024])  # NaN / zero blocks too
    wire = np.concatenate([R.quantize(R.f32(x), 1) for x in xs])
    for op in ("sum", "avg"):
        want = R.reduce(wire, nsrc, op)
        got = ops.mx_reduce_reference(torch.from_numpy(wire), nsrc, op).numpy()
        assert np.array_equal(got, want), (nsrc, op)
    if nsrc >= 3:  # the inputs tell fold orders apart
        back = np.concatenate([R.quantize(R.f32(x), 1) for x in reversed(xs)])
        assert not R.same_wire(R.reduce(back, nsrc, "sum"), R.reduce(wire, nsrc, "sum"), 1)


def test_chunk_rule_matches_the_reference():
    for w in range(1, 9):
        for n in NUMELS + (0, 512 * w - 1, 512 * w + 1, 4 << 20, 31776 * 32 * w, 31776 * 32 * w + 1, (1 << 33) + 5):
            assert ops.mx_chunk_blocks(n, w) == R.chunk_blocks(n, w), (n, w)
            assert ops.mx_wire_bytes(n, w) == R.wire_bytes(n, w)
    assert ops.mx_chunk_blocks(4 << 20, 4) == 32768  # a chunk wire past 1 MiB: whole 4-KiB tiles
    assert ops.mx_chunk_blocks(31776 * 32, 1) == 32768 and ops.mx_chunk_blocks(31760 * 32, 1) == 31760


# ------------------------------------------------------------------ properties of the contract
def test_requantizing_a_dequantized_wire_changes_nothing():
    # D(Q(D(w))) == D(w) for every wire the quantizer can write: scale bytes 10..247 (and 255), any
    # non-NaN payload, values finite (scale 247 with |payload| >= 256 would be 2^128)
    rng = np.random.default_rng(5)
    blocks = 4096
    q = rng.integers(0, 256, (blocks, 32)).astype(np.uint8)
    q[(q & 0x7F) == 0x7F] = 0x7E
    q[rng.random((blocks, 32)) < 0.3] = 0  # sparse blocks, small maxima
    q[:64, 1:] &= 0x87  # blocks of FP8 subnormals and zeros only
    s = rng.integers(10, 247, blocks).astype(np.uint8)
    s[:32], s[32:64], s[64:96] = 10, 247, 255
    q[32:64] &= 0xF7  # below 256: finite at the top scale
    for D, Q in ((R.d_blocks, R.q_blocks), (ops._mx_dequantize_blocks, ops._mx_quantize_blocks)):
        conv = (lambda a: a) if D is R.d_blocks else torch.from_numpy
        back = (lambda a: a) if D is R.d_blocks else (lambda a: a.numpy())
        d = back(D(conv(q), conv(s)))
        assert np.isfinite(d[s != 255]).all()
        q2, s2 = Q(conv(d))
        d2 = back(D(q2, s2))
        assert R.same(torch.from_numpy(d2), torch.from_numpy(d))
        assert ((np.abs(d) >= 2.0 ** -126) | (d == 0) | np.isnan(d)).all()  # normal f32 or zero


@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_error_bound_against_the_f64_sum(world):
    # |result - exact| <= (sum_r amax_{r,b} + amax_b(fold)) / 16 * (1 + 2^-10) per element of block
    # b: each quantization errs by at most amax / 16 (3 mantissa bits, scaled amax <= 448; half an
    # ulp of the top binade is 16 of 448 ... 256), the f32 fold by far less (the 2^-10 slack).
    # Derived, not measured; it holds for blocks with every amax_r >= 2^-100.
    rng = np.random.default_rng(world)
    blocks = 2048
    xs = []
    for r in range(world):
        normal = rng.standard_normal((blocks // 2, 32))
        lognormal = np.exp(rng.standard_normal((blocks // 2, 32)) * 3.0) * rng.choice([-1.0, 1.0], (blocks // 2, 32))
        xs.append(np.concatenate([normal, lognormal]).astype(np.float32))
    exact = np.sum([x.astype(np.float64) for x in xs], axis=0)
    amax_in = np.sum([np.abs(x).max(axis=1).astype(np.float64) for x in xs], axis=0)
    ds = [R.d_blocks(*R.q_blocks(x)) for x in xs]
    fold = R.fold_blocks(ds, "sum")
    bound = (amax_in + np.abs(fold).max(axis=1).astype(np.float64)) / 16 * (1 + 2.0 ** -10)
    got = R.all_reduce([torch.from_numpy(x.reshape(-1)) for x in xs], "sum").numpy().reshape(blocks, 32)
    worst = (np.abs(got.astype(np.float64) - exact) / bound[:, None]).max()
    print(f"world {world}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0, worst
    # the torch reference computes the same values
    wire = torch.cat([ops.mx_quantize_reference(torch.from_numpy(x.reshape(-1))) for x in xs])
    y = ops.mx_dequantize_reference(ops.mx_reduce_reference(wire, world, "sum"), blocks * 32)
    assert R.same(y, torch.from_numpy(got))


# ------------------------------------------------------------------ the collective on CPU tensors
@pytest.mark.parametrize("world", [2, 3, 4])
def test_all_reduce_compressed_cpu_tensors(world):
    numels = (1, 33, 512 * world - 1, 512 * world + 1, 70001)
    res = launch(M.all_reduce_cases, world, args=("cpu", numels, tuple(R.DTYPES), ("sum", "avg")))
    for r, got in enumerate(res):
        assert len(got) == 3 * len(numels) * 2, sorted(got)
        bad = [k for k, v in got.items() if not v[0]]
        assert not bad, (r, bad)
        assert {k: v[1] for k, v in got.items()} == {k: v[1] for k, v in res[0].items()}, r  # the same bits


def test_inputs_tell_fold_orders_apart():
    # world 3: folding the ranks in another order gives other values, so the test above pins the order
    xs = M.rank_inputs(512 * 3 + 1, 3, 1000 + (512 * 3 + 1) % 9973)
    want = R.all_reduce(xs, "sum")
    assert not R.same(R.all_reduce(xs[::-1], "sum"), want)
    assert not R.same(R.all_reduce([xs[1], xs[2], xs[0]], "sum"), want)


def test_world_1_leaves_the_tensor_unchanged():
    got = launch(M.world1_and_errors, 1, args=("cpu",))[0]
    assert len(got) == 3 + 6 and all(got.values()), got


def test_error_cases():
    for got in launch(M.world1_and_errors, 2, args=("cpu",)):
        assert len(got) == 6 and all(got.values()), got
    with pytest.raises(ValueError, match="'max'"):
        ops.mx_reduce_reference(torch.zeros(33 * 16, dtype=torch.uint8), 1, "max")
    with pytest.raises(TypeError, match="float64"):
        ops.mx_quantize_reference(torch.zeros(4, dtype=torch.float64))


def test_grad_bucketer_with_a_compressed_wire_on_cpu_tensors():
    res = launch(M.bucketer, 2, args=("cpu",))
    for got in res:
        assert got["buckets"] >= 2 and got["handles"] == ["CompressedWork"], got
        for i in range(got["buckets"]):
            assert got[i][0], (i, got[i])
            assert got[i][1] == res[0][i][1]  # the same bits on both ranks
    from pytorch_distributed_collective_communication_amd.parallel import ddp

    with pytest.raises(ValueError, match="mxfp4"):
        ddp.GradBucketer(torch.nn.Linear(2, 2), wire="mxfp4")


# ------------------------------------------------------------------ the layout header, sanitized
def _build() -> str:
    exe = os.path.join(BUILD, "mx_layout_check")
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


def test_layout_header_under_sanitizers():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    exe = _build()
    cases = [(n, w) for w in (1, 2, 3, 4, 8) for n in NUMELS + (512 * w - 1, 512 * w + 1, 4 << 20)]
    argv = [str(v) for c in cases for v in c]
    for args in ([], argv):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
        lines = r.stdout.strip().splitlines()
        assert lines[-1].split()[0] == "ok" and int(lines[-1].split()[1]) >= len(cases)
        for ln in lines[:-1]:  # "numel world cb wire_bytes": the C++ layout and the Python one agree
            n, w, cb, nbytes = map(int, ln.split())
            assert ops.mx_chunk_blocks(n, w) == cb and ops.mx_wire_bytes(n, w) == nbytes, ln
