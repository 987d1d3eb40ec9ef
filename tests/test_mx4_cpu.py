"""The block-scaled FP4 wire format `mxfp4_e2m1` without a GPU (docs/collectives.md "The
`mxfp4_e2m1` wire format").

* `ops.mx_*_reference(wire="mxfp4_e2m1")` (plain PyTorch) against tests/_mx4_ref.py (numpy integer
  arithmetic on the f32 bits and the table of the eight magnitudes): exact bytes, exact values;
* the Python layout helpers against the layout header (tests/native/mx4_layout_check.cpp, a
  stand-alone program under ASan + UBSan), the 1 MiB alignment switch included;
* the three collectives on CPU tensors over the shm transport (worlds 2, 3, 4, 8), world 1, the
  error cases; `GradBucketer` and `ShardedOptimizer` with the FP4 wire;
* the three derived error bounds against f64 sums.

Every comparison is exact: rtol = atol = 0, NaN where the reference has NaN.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

from pytorch_distributed_collective_communication_amd import ops
from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _mx4_ref as R
from tests import _workers_mx as M8
from tests import _workers_mx4 as M
from tests._workers_mx_shard import shard_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
BUILD = os.path.join(ROOT, "build", "san")
SRC = os.path.join(ROOT, "tests", "native", "mx4_layout_check.cpp")
HDR = os.path.join(CSRC, "kernels", "mx_layout.h")

W4 = R.WIRE
NUMELS = (1, 31, 32, 33, 63, 65, 511, 513, 4113, 65553)
WORLDS = (1, 3, 8)
# 17 cb reaches 1 MiB between cb = 61680 (2^20 - 16 bytes) and cb = 61696
BELOW, ABOVE = 61680 * 32, 61680 * 32 + 1


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the edge set holds what it claims
def test_edge_blocks_cover_every_branch_of_the_quantizer():
    eb = R.edge_blocks()
    amax = {k: int((_bits(v) & 0x7FFFFFFF).max()) for k, v in eb.items()}
    q = {k: R.q_blocks(v[None]) for k, v in eb.items()}
    code = {k: R.unpack_codes(v[0])[0] for k, v in q.items()}
    scale = {k: int(s[0]) for k, (_, s) in q.items()}
    d = {k: R.d_blocks(*v)[0] for k, v in q.items()}
    for z in ("zero", "minus_zero"):  # an all-zero block whatever the signs
        assert amax[z] == 0 and scale[z] == 127 and not q[z][0].any()
    assert (_bits(eb["minus_zero"]) == 0x80000000).all()
    assert np.isnan(eb["one_nan"]).sum() == 1 and scale["one_nan"] == 255 and np.isnan(d["one_nan"]).all()
    assert np.isinf(eb["both_inf"]).sum() == 2 and scale["both_inf"] == 255 and np.isnan(d["both_inf"]).all()
    assert not q["one_nan"][0].any() and not q["both_inf"][0].any()  # the reference writes 0 there
    for j in (-100, -20, 0, 9, 100):  # the m = 1.5 switch: e = k - 2 up to mantissa 0x400000, k - 1 above
        a, up, dn = f"amax_1.5_2^{j}", f"amax_1.5_2^{j}_plus_ulp", f"amax_1.5_2^{j}_minus_ulp"
        assert amax[a] & 0x7FFFFF == 0x400000 and amax[up] == amax[a] + 1 and amax[dn] == amax[a] - 1
        assert scale[a] == 127 + j - 2 and scale[dn] == 127 + j - 2 and scale[up] == 127 + j - 1
        assert (code[a] & 7).max() == 7 and (code[dn] & 7).max() == 7  # scaled amax 6 (or a hair below)
        assert (code[up] & 7).max() == 5                                # scaled amax just above 3
    assert scale["mant_400001_negative"] == 127 - 1 and code["mant_400001_negative"][5] == 8 | 5
    # ties go to the even code, in both signs; e = 0 so the block is its own scaled value
    t, c = eb["ties"], code["ties"]
    assert scale["ties"] == 127 and t[0] == 6 and c[0] == 7
    assert t[1:8].tolist() == list(R.TIES) and c[1:8].tolist() == [0, 2, 2, 4, 4, 6, 6]
    assert t[8:15].tolist() == [-v for v in R.TIES] and c[8:15].tolist() == [8, 10, 10, 12, 12, 14, 14]
    assert c[15:19].tolist() == [0, 1, 2, 3] and c[19:23].tolist() == [8 | 1, 8 | 2, 8 | 3, 8 | 4]  # a hair off the ties
    assert c[23] == 0 and c[24] == 8 and c[25] == 0 and c[26] == 8  # below 0.25: signed zero codes
    assert c[27] == 8 and c[28] == 0                                  # -0 keeps its sign next to a non-zero amax
    assert d["ties"][24] == 0 and np.signbit(d["ties"][24]) and not np.signbit(d["ties"][23])
    for k, sh in (("ties_2^40", 40), ("ties_2^-60", -60)):  # the same codes under another scale
        assert scale[k] == 127 + sh and np.array_equal(code[k][:25], c[:25])
    # the lower clamp: e = -125, every non-zero dequantized value is a normal f32
    for k in ("amax_2^-124", "amax_2^-126", "amax_subnormal", "amax_largest_subnormal"):
        assert scale[k] == 2, k
        nz = d[k][d[k] != 0]
        assert (np.abs(nz) >= 2.0 ** -126).all()
    assert amax["amax_subnormal"] < 0x00800000 and not code["amax_subnormal"].any()  # 0x123 2^-149 2^125 < 0.25
    assert code["amax_2^-126"][5] == 1 and d["amax_2^-126"][5] == 2.0 ** -126        # 0.5 2^-125
    assert scale["amax_2^-120"] == 127 - 120 - 2
    # the top: e = 126; a payload of 4 is 2^128
    assert scale["amax_f32_max"] == 253 and code["amax_f32_max"][5] == 6 and np.isinf(d["amax_f32_max"][5])
    assert scale["amax_1.5_2^127"] == 252 and d["amax_1.5_2^127"][5] == eb["amax_1.5_2^127"][5]
    # the other dtypes' extremes survive their casts
    assert torch.tensor(eb["amax_f16_max"]).to(torch.float16).isfinite().all()
    assert float(torch.tensor(eb["amax_f16_min_subnormal"]).to(torch.float16)[5]) == 2.0 ** -24
    assert torch.tensor(eb["amax_bf16_max"]).to(torch.bfloat16).isfinite().all()
    ex = (_bits(R.random_binades(96, 13)) >> 23) & 0xFF
    assert int(ex.max()) - int(ex[ex > 0].min()) >= 80


# ------------------------------------------------------------------ the references against each other
@pytest.mark.parametrize("world", WORLDS)
def test_references_agree_on_the_edge_blocks(world):
    x, _ = R.edge_tensor()
    for dtn, dt in R.DTYPES.items():
        xt = torch.from_numpy(x).to(dt)
        want = R.quantize(R.f32(xt), world)
        got = ops.mx_quantize_reference(xt, world, wire=W4)
        assert got.dtype == torch.uint8 and got.numel() == ops.mx_wire_bytes(x.size, world, wire=W4) == want.size
        assert np.array_equal(got.numpy(), want), dtn  # every byte (both write 0 under a NaN block)
        for odt in R.DTYPES.values():
            d = ops.mx_dequantize_reference(got, x.size, odt, world, wire=W4)
            assert d.dtype == odt and R.same(d, R.dequantize(want, x.size, world, odt)), (dtn, odt)


@pytest.mark.parametrize("numel", NUMELS)
def test_references_agree_on_ragged_sizes(numel):
    for world in WORLDS:
        x = M8.rank_inputs(numel, 2, 77 + numel)[1]
        want = R.quantize(R.f32(x), world)
        got = ops.mx_quantize_reference(x, world, wire=W4).numpy()
        assert np.array_equal(got, want), (numel, world)
        q, s = R.split(got, world)  # padding blocks (whole chunks at small sizes): scale 127, payload 0
        first_pad = -(-numel // 32)
        assert (s[first_pad:] == 127).all() and not q[first_pad:].any()
        if numel % 32:
            assert not R.unpack_codes(q[first_pad - 1:first_pad])[0, numel % 32:].any()
        assert R.same(ops.mx_dequantize_reference(torch.from_numpy(got), numel, torch.float32, world, wire=W4),
                      R.dequantize(want, numel, world))


@pytest.mark.parametrize("W", WORLDS)
def test_shard_references_agree(W):
    edge = torch.from_numpy(R.edge_tensor()[0])
    for dtn, dt in R.DTYPES.items():
        cases = [(shard_inputs(m, max(W, 2), 50 + m, dt)[1][:W * m], m) for m in NUMELS[:-1]]  # m = 1, m % 32 != 0
        x = shard_inputs(edge.numel(), max(W, 2), 7)[0][:W * edge.numel()].clone()
        x[(W - 1) * edge.numel():] = edge
        cases.append((x.to(dt), edge.numel()))
        for x, m in cases:
            want = R.quantize_shards(R.f32(x), W)
            got = ops.mx_quantize_shards_reference(x, W, wire=W4)
            assert got.numel() == ops.mx_shard_wire_bytes(m, W, wire=W4) == R.shard_wire_bytes(m, W) == want.size
            assert np.array_equal(got.numpy(), want), (dtn, m, W)
            for odt in R.DTYPES.values():
                d = ops.mx_dequantize_shards_reference(got, m, odt, W, wire=W4)
                assert d.dtype == odt and R.same(d, R.dequantize_shards(want, m, W, odt)), (dtn, m, W, odt)
    # blocks are counted from each shard's start: for m % 32 != 0 the bytes differ from the dealt wire
    x = shard_inputs(33, 2, 3)[0]
    assert not np.array_equal(R.quantize_shards(R.f32(x), 2)[:16 * 16], R.quantize(R.f32(x), 2)[:16 * 16])


@pytest.mark.parametrize("nsrc", [1, 2, 3, 5, 8])
def test_reduce_and_fold_references_fold_in_source_order(nsrc):
    for n in (48 * 32, 4113):
        xs = M8.rank_inputs(n, nsrc, 5 + nsrc)
        xs[nsrc - 1][:1024] = torch.from_numpy(R.edge_tensor()[0][:1024])  # NaN / inf / zero blocks too
        wire = np.concatenate([R.quantize(R.f32(x), 1) for x in xs])
        for op in ("sum", "avg"):
            got = ops.mx_reduce_reference(torch.from_numpy(wire), nsrc, op, wire=W4).numpy()
            assert np.array_equal(got, R.reduce(wire, nsrc, op)), (nsrc, n, op)
            for dt in R.DTYPES.values():
                f = ops.mx_fold_reference(torch.from_numpy(wire), nsrc, n, dt, op, wire=W4)
                assert f.dtype == dt and R.same(f, R.fold(wire, nsrc, n, op, dt)), (nsrc, n, op, dt)
        if nsrc >= 3:  # the inputs tell fold orders apart
            back = np.concatenate([R.quantize(R.f32(x), 1) for x in reversed(xs)])
            assert not R.same_wire(R.reduce(back, nsrc, "sum"), R.reduce(wire, nsrc, "sum"), 1)
            assert not R.same(R.fold(back, nsrc, n), R.fold(wire, nsrc, n))


def test_requantizing_a_dequantized_wire_changes_nothing():
    # D(Q(D(w))) == D(w) for every wire the quantizer can write (finite values: below 4 at scale 253)
    rng = np.random.default_rng(5)
    blocks = 2048
    q = rng.integers(0, 256, (blocks, 16)).astype(np.uint8)
    q[rng.random((blocks, 16)) < 0.3] = 0
    s = rng.integers(2, 253, blocks).astype(np.uint8)
    s[:32], s[32:64], s[64:96] = 2, 253, 255
    q[32:64] &= 0xDD  # codes 0..5 and their negatives: at most 3 2^126
    d = R.d_blocks(q, s)
    assert np.isfinite(d[s != 255]).all()
    assert R.same(torch.from_numpy(R.d_blocks(*R.q_blocks(d))), torch.from_numpy(d))
    dt = ops._mx4_dequantize_blocks(torch.from_numpy(q), torch.from_numpy(s))
    assert R.same(dt, torch.from_numpy(d))
    assert R.same(ops._mx4_dequantize_blocks(*ops._mx4_quantize_blocks(dt)), dt)
    assert ((np.abs(d) >= 2.0 ** -126) | (d == 0) | np.isnan(d)).all()  # normal f32 or zero


# ------------------------------------------------------------------ the layout
def test_layout_helpers_match_the_reference():
    for w in range(1, 9):
        for n in NUMELS + (0, 512 * w - 1, 512 * w + 1, BELOW * w, ABOVE * w, (1 << 33) + 5):
            assert ops.mx_chunk_blocks(n, w, wire=W4) == R.chunk_blocks(n, w), (n, w)
            assert ops.mx_wire_bytes(n, w, wire=W4) == R.wire_bytes(n, w) == 17 * R.chunk_blocks(n, w) * w
        for m in NUMELS + (BELOW, ABOVE):
            assert ops.mx_shard_blocks(m, wire=W4) == R.shard_blocks(m) == ops.mx_chunk_blocks(m, 1, wire=W4)
            assert ops.mx_shard_wire_bytes(m, w, wire=W4) == R.shard_wire_bytes(m, w)
    # the 1 MiB switch: 17 cb just below 2^20 stays, just above goes to whole 4-KiB tiles
    assert ops.mx_chunk_blocks(BELOW, 1, wire=W4) == 61680 and 17 * 61680 == (1 << 20) - 16
    assert ops.mx_chunk_blocks(ABOVE, 1, wire=W4) == 65536
    # ... at another place than for FP8, whose values are unchanged
    assert ops.mx_chunk_blocks(BELOW, 1) == 65536 and ops.mx_chunk_blocks(31760 * 32, 1) == 31760
    assert ops.mx_chunk_blocks(31760 * 32, 1, wire=W4) == 31760
    assert ops.mx_wire_bytes(4096, 1) == 33 * 128 and ops.mx_wire_bytes(4096, 1, wire=W4) == 17 * 128


def _build() -> str:
    exe = os.path.join(BUILD, "mx4_layout_check")
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
    cases = [("d", n, w) for w in (1, 2, 3, 8) for n in NUMELS + (512 * w - 1, 512 * w + 1, BELOW * w, ABOVE * w)]
    cases += [("s", m, w) for w in (1, 3, 8) for m in NUMELS] + [("s", BELOW, 2), ("s", ABOVE, 2)]
    argv = [str(v) for c in cases for v in c]
    for args in ([], argv):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
        lines = r.stdout.strip().splitlines()
        assert lines[-1].split()[0] == "ok" and int(lines[-1].split()[1]) >= len(cases)
        for ln in lines[:-1]:  # "d|s n world cb wire_bytes": the C++ layout and the Python one agree
            mode, n, w, cb, nbytes = ln.split()
            n, w, cb, nbytes = int(n), int(w), int(cb), int(nbytes)
            if mode == "d":
                assert ops.mx_chunk_blocks(n, w, wire=W4) == cb and ops.mx_wire_bytes(n, w, wire=W4) == nbytes, ln
            else:
                assert ops.mx_shard_blocks(n, wire=W4) == cb and ops.mx_shard_wire_bytes(n, w, wire=W4) == nbytes, ln


# ------------------------------------------------------------------ the error bounds
@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_error_bounds_against_f64_sums(world):
    # One scaled unit is 2^e < amax / 3 (the scaled amax lies in (3, 6]) and the coarsest grid step, 4 .. 6,
    # is 2 units, so a quantization errs by at most amax_block / 3; the f32 fold adds far less (the 2^-10
    # slack). Derived, not measured; every block here has amax >= 2^-100, so no element is excluded.
    rng = np.random.default_rng(40 + world)
    blocks = 1024
    xs = []
    for r in range(world):
        normal = rng.standard_normal((blocks // 2, 32))
        lognormal = np.exp(rng.standard_normal((blocks // 2, 32)) * 3.0) * rng.choice([-1.0, 1.0], (blocks // 2, 32))
        xs.append(np.concatenate([normal, lognormal]).astype(np.float32))
    amaxes = [np.abs(x).max(axis=1).astype(np.float64) for x in xs]
    assert min(a.min() for a in amaxes) >= 2.0 ** -100
    exact = np.sum([x.astype(np.float64) for x in xs], axis=0)
    ts = [torch.from_numpy(x.reshape(-1)) for x in xs]
    slack = 1 + 2.0 ** -10

    def share(got, bound):
        return float((np.abs(got.numpy().reshape(blocks, 32).astype(np.float64) - exact) / bound[:, None]).max())

    # reduce-scatter: one quantization per contribution, the fold stays f32. Blocks are independent, so
    # the fold of the whole tensor is what the ranks' shards hold together (checked on whole-block shards)
    fold = R.fold_blocks([R.d_blocks(*R.q_blocks(x)) for x in xs], "sum")
    m = blocks // world * 32
    rs = torch.cat([R.reduce_scatter([t[:m * world] for t in ts], k) for k in range(world)])
    assert R.same(rs, torch.from_numpy(fold.reshape(-1)[:m * world]))
    rs_share = share(torch.from_numpy(fold.reshape(-1)), sum(amaxes) / 3 * slack)
    # all-reduce: the fold is quantized once more
    ar_share = share(R.all_reduce(ts), (sum(amaxes) + np.abs(fold).max(axis=1).astype(np.float64)) / 3 * slack)
    # all-gather: every shard quantized once, against the shard itself
    ag_share = 0.0
    for x, a in zip(xs, amaxes):
        g = R.all_gather([torch.from_numpy(x.reshape(-1))]).numpy().reshape(blocks, 32).astype(np.float64)
        ag_share = max(ag_share, float((np.abs(g - x.astype(np.float64)) / (a / 3)[:, None]).max()))
    print(f"world {world}: worst error / bound: reduce-scatter {rs_share:.3f}, all-reduce {ar_share:.3f}, "
          f"all-gather {ag_share:.3f}")
    assert rs_share <= 1.0 and ar_share <= 1.0 and ag_share <= 1.0, (rs_share, ar_share, ag_share)
    # the torch references compute the same values
    wire = torch.cat([ops.mx_quantize_reference(t, wire=W4) for t in ts])
    y = ops.mx_dequantize_reference(ops.mx_reduce_reference(wire, world, "sum", wire=W4), blocks * 32, wire=W4)
    assert R.same(y, R.all_reduce(ts))


# ------------------------------------------------------------------ the collectives on CPU tensors
@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_collectives_on_cpu_tensors(world):
    numels = (1, 33, 513, 4113)
    dtypes = tuple(R.DTYPES) if world <= 4 else ("float32",)
    res = launch(M.collective_cases, world, args=("cpu", numels, dtypes, ("sum", "avg")))
    for r, got in enumerate(res):
        assert len(got) == len(dtypes) * len(numels) * 5, sorted(got)
        bad = [k for k, v in got.items() if not v[0]]
        assert not bad, (r, bad)
        same = {k: v[1] for k, v in got.items() if not k.startswith("rs/")}  # identical bits on every rank
        assert same == {k: v[1] for k, v in res[0].items() if not k.startswith("rs/")}, r


def test_inputs_tell_fold_orders_apart():
    n = 513
    xs = M8.rank_inputs(n, 3, M._seed(n))
    want = R.all_reduce(xs, "sum")
    assert not R.same(R.all_reduce(xs[::-1], "sum"), want)
    ss = shard_inputs(n, 3, M._seed(n) + 17)
    assert not R.same(R.reduce_scatter(ss[::-1], 1), R.reduce_scatter(ss, 1))


def test_world_1_and_error_cases():
    got = launch(M.world1_and_errors, 1, args=("cpu",))[0]
    assert len(got) == 9 + 17 and all(got.values()), got
    for got in launch(M.world1_and_errors, 2, args=("cpu",)):
        assert len(got) == 17 and all(got.values()), got


def test_unknown_wires_raise_in_ops():
    x = torch.zeros(64)
    w = torch.zeros(17 * 16, dtype=torch.uint8)
    for bad in ("mxfp4", "mxfp6", None):
        for fn in (lambda: ops.mx_quantize_reference(x, 1, wire=bad), lambda: ops.mx_reduce_reference(w, 1, wire=bad),
                   lambda: ops.mx_dequantize_reference(w, 64, wire=bad), lambda: ops.mx_fold_reference(w, 1, 64, wire=bad),
                   lambda: ops.mx_quantize_shards_reference(x, 2, wire=bad),
                   lambda: ops.mx_dequantize_shards_reference(w, 64, wire=bad),
                   lambda: ops.mx_chunk_blocks(64, 1, wire=bad), lambda: ops.mx_wire_bytes(64, 1, wire=bad),
                   lambda: ops.mx_shard_blocks(64, wire=bad), lambda: ops.mx_shard_wire_bytes(64, 1, wire=bad),
                   lambda: ops.mx_quantize(x, wire=bad), lambda: ops.mx_fold(w, 1, 64, wire=bad)):
            with pytest.raises(ValueError, match="unknown wire format .*mxfp4_e2m1"):
                fn()
    with pytest.raises(ValueError, match="'max'"):
        ops.mx_reduce_reference(w, 1, "max", wire=W4)
    with pytest.raises(TypeError, match="float64"):
        ops.mx_quantize_reference(torch.zeros(4, dtype=torch.float64), wire=W4)
    with pytest.raises(ValueError, match="272 bytes"):  # an FP8-sized wire is not an FP4 wire
        ops.mx_dequantize_reference(torch.zeros(33 * 16, dtype=torch.uint8), 64, wire=W4)


def test_grad_bucketer_with_the_fp4_wire_on_cpu_tensors():
    res = launch(M.bucketer, 2, args=("cpu",))
    for got in res:
        assert got["buckets"] >= 2 and got["handles"] == ["CompressedWork"], got
        for i in range(got["buckets"]):
            assert got[i][0], (i, got[i])
            assert got[i][1] == res[0][i][1]  # the same bits on both ranks
    from pytorch_distributed_collective_communication_amd.parallel import ddp

    for bad in ("mxfp4", "mxfp6"):
        with pytest.raises(ValueError, match=bad):
            ddp.GradBucketer(torch.nn.Linear(2, 2), wire=bad)


@pytest.mark.parametrize("grad_wire,param_wire", [(W4, W4), (W4, None), (None, W4), (W4, "mxfp8_e4m3")])
def test_sharded_optimizer_with_fp4_wires_on_cpu_tensors(grad_wire, param_wire):
    res = launch(M.zero, 2, args=("cpu", grad_wire, param_wire))
    for got in res:
        assert got["buckets"] >= 2, got
        if grad_wire is not None:
            assert got["handles"] == ["CompressedWork"], got
        for i in range(got["buckets"]):
            assert got[i][0] and got[i][1], (i, got[i])
        assert got["digest"] == res[0]["digest"]
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    with pytest.raises(ValueError, match="mxfp4"):
        ShardedOptimizer(torch.nn.Linear(2, 2).parameters(), grad_wire="mxfp4")
