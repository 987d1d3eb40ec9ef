"""The block-scaled FP6 wire format `mxfp6_e2m3` without a GPU (docs/collectives.md "The `mxfp6_e2m3`
wire format").

* `ops.mx_*_reference(wire="mxfp6_e2m3")` (plain PyTorch) against tests/_mx6_ref.py (a float64 table of the 32
  magnitudes, distances compared, bits packed one by one): exact bytes, exact values -- both layouts, three
  dtypes, reduce and fold with 1..8 sources, error feedback and stochastic rounding;
* the layout helpers and `mx_sr_e2m3` against the headers (tests/native/mx6_check.cpp, a stand-alone program
  under ASan + UBSan), the 1 MiB alignment switch included; the error cases;
* the three derived error bounds against f64 sums, the error-feedback series and the unbiasedness cap;
* the three collectives on CPU tensors over the shm transport (worlds 2, 3, 4, 8), plain, with residuals and
  stochastic; world 1; `GradBucketer` and `ShardedOptimizer` with the FP6 wire.

Every comparison is exact: rtol = atol = 0, NaN where the reference has NaN.
"""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from pytorch_distributed_collective_communication_amd import ops
from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _mx6_ref as R
from tests import _mx_ef_ref as E
from tests import _workers_mx as M8
from tests import _workers_mx6 as M
from tests._workers_mx_shard import shard_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
BUILD = os.path.join(ROOT, "build", "san")
SRC = os.path.join(ROOT, "tests", "native", "mx6_check.cpp")
HDRS = (os.path.join(CSRC, "kernels", "mx_layout.h"), os.path.join(CSRC, "kernels", "mx_sr.h"))

W6 = R.WIRE
SR = dict(rounding="stochastic")
NUMELS = (1, 31, 32, 33, 63, 65, 511, 513, 4113, 65553)
WORLDS = (1, 3, 8)
# 25 cb reaches 1 MiB between cb = 41936 (2^20 - 176 bytes) and cb = 41952
BELOW, ABOVE = 41936 * 32, 41936 * 32 + 1


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the reference itself
def test_the_reference_packs_the_documented_bit_stream():
    rng = np.random.default_rng(1)
    code = rng.integers(0, 64, (64, 32)).astype(np.uint8)
    q = R.pack_codes(code)
    assert q.shape == (64, 24) and np.array_equal(R.unpack_codes(q), code)
    for b in range(4):  # written out: bit n of the stream is bit n % 8 of byte n / 8
        stream = sum(int(c) << (6 * j) for j, c in enumerate(code[b]))
        assert bytes(q[b]) == stream.to_bytes(24, "little")
    assert np.array_equal(ops._mx6_pack(torch.from_numpy(code)).numpy(), q)
    assert np.array_equal(ops._mx6_unpack(torch.from_numpy(q)).numpy(), code)
    assert R.MAGS.tolist() == [0, .125, .25, .375, .5, .625, .75, .875, 1, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
                               2, 2.25, 2.5, 2.75, 3, 3.25, 3.5, 3.75, 4, 4.5, 5, 5.5, 6, 6.5, 7, 7.5]


def test_edge_blocks_cover_every_branch_of_the_quantizer():
    eb = R.edge_blocks()
    amax = {k: int((_bits(v) & 0x7FFFFFFF).max()) for k, v in eb.items()}
    q = {k: R.q_blocks(v[None]) for k, v in eb.items()}
    code = {k: R.unpack_codes(v[0])[0] for k, v in q.items()}
    scale = {k: int(s[0]) for k, (_, s) in q.items()}
    d = {k: R.d_blocks(*v)[0] for k, v in q.items()}
    for z in ("zero", "minus_zero"):
        assert amax[z] == 0 and scale[z] == 127 and not q[z][0].any()
    for z in ("one_nan", "both_inf"):
        assert scale[z] == 255 and np.isnan(d[z]).all() and not q[z][0].any()
    for j in (-100, -20, 0, 9, 100):  # the m = 1.875 switch: e = k - 2 up to mantissa 0x700000, k - 1 above
        a, up, dn = f"amax_1.875_2^{j}", f"amax_1.875_2^{j}_plus_ulp", f"amax_1.875_2^{j}_minus_ulp"
        assert amax[a] & 0x7FFFFF == 0x700000 and amax[up] == amax[a] + 1 and amax[dn] == amax[a] - 1
        assert scale[a] == 127 + j - 2 and scale[dn] == 127 + j - 2 and scale[up] == 127 + j - 1
        assert (code[a] & 31).max() == 31 and (code[dn] & 31).max() == 31  # scaled amax 7.5 (or a hair below)
        assert (code[up] & 31).max() == 23                                  # scaled amax just above 3.75
    assert scale["mant_700001_negative"] == 127 - 1 and code["mant_700001_negative"][5] == 32 | 23
    # ties go to the even code, in both signs; e = 0 so the block is its own scaled value
    t, c = eb["ties"], code["ties"]
    assert scale["ties"] == 127 and t[0] == 7.5 and c[0] == 31
    assert c[1:9].tolist() == [0, 2, 8, 8, 16, 16, 24, 30]
    assert c[9:17].tolist() == [32 | v for v in (0, 2, 8, 8, 16, 16, 24, 30)]
    assert c[17:20].tolist() == [0, 1, 7] and c[20:23].tolist() == [32 | 1, 32 | 2, 32 | 8]  # a hair off the ties
    assert c[23] == 0 and c[24] == 32 and c[25] == 0 and c[26] == 32  # below 0.0625: signed zero codes
    assert c[27] == 32 and c[28] == 0                                   # -0 keeps its sign next to a non-zero amax
    assert d["ties"][24] == 0 and np.signbit(d["ties"][24]) and not np.signbit(d["ties"][23])
    for k, sh in (("ties_2^40", 40), ("ties_2^-60", -60)):
        assert scale[k] == 127 + sh and np.array_equal(code[k][:25], c[:25])
    # the lower clamp: e = -123, every non-zero dequantized value is a normal f32
    for k in ("amax_2^-122", "amax_2^-126", "amax_subnormal", "amax_largest_subnormal"):
        assert scale[k] == 4, k
        nz = d[k][d[k] != 0]
        assert (np.abs(nz) >= 2.0 ** -126).all()
    assert not code["amax_subnormal"].any() and code["amax_2^-126"][5] == 1 and d["amax_2^-126"][5] == 2.0 ** -126
    assert scale["amax_2^-118"] == 127 - 118 - 2
    # the top: e = 126; a payload of 4 or more is inf, from amax 1.9375 2^127 on
    assert scale["amax_f32_max"] == 253 and code["amax_f32_max"][5] == 24 and np.isinf(d["amax_f32_max"][5])
    assert scale["amax_1.9375_2^127"] == 253 and code["amax_1.9375_2^127"][5] == 24 and np.isinf(d["amax_1.9375_2^127"][5])
    assert code["amax_below_1.9375_2^127"][5] == 23 and np.isfinite(d["amax_below_1.9375_2^127"]).all()
    assert scale["amax_1.875_2^127"] == 252 and d["amax_1.875_2^127"][5] == eb["amax_1.875_2^127"][5]
    # and the twin in ops takes every one of these branches the same way
    for k, v in eb.items():
        w = ops.mx_quantize_reference(torch.from_numpy(v), 1, wire=W6).numpy()
        tq, ts = R.split(w, 1)
        assert ts[0] == scale[k] and np.array_equal(R.unpack_codes(tq[:1])[0], code[k]), k
        back = ops.mx_dequantize_reference(torch.from_numpy(w), 32, wire=W6)
        assert R.same(back, torch.from_numpy(d[k])), k


# ------------------------------------------------------------------ the twins against the reference
@pytest.mark.parametrize("world", WORLDS)
def test_references_agree_on_the_edge_blocks(world):
    x, _ = R.edge_tensor()
    for dtn, dt in R.DTYPES.items():
        xt = torch.from_numpy(x).to(dt)
        want = R.quantize(R.f32(xt), world)
        got = ops.mx_quantize_reference(xt, world, wire=W6)
        assert got.dtype == torch.uint8 and got.numel() == ops.mx_wire_bytes(x.size, world, wire=W6) == want.size
        assert np.array_equal(got.numpy(), want), dtn
        for odt in R.DTYPES.values():
            d = ops.mx_dequantize_reference(got, x.size, odt, world, wire=W6)
            assert d.dtype == odt and R.same(d, R.dequantize(want, x.size, world, odt)), (dtn, odt)
        for seed in (0, 3):
            want = R.quantize(R.f32(xt), world, (seed, 2, 5))
            got = ops.mx_quantize_reference(xt, world, wire=W6, seed=seed, stream=2, index_offset=5, **SR)
            assert np.array_equal(got.numpy(), want), (dtn, seed)


@pytest.mark.parametrize("numel", NUMELS)
def test_references_agree_on_ragged_sizes(numel):
    for world in WORLDS:
        x = M8.rank_inputs(numel, 2, 77 + numel)[1]
        want = R.quantize(R.f32(x), world)
        got = ops.mx_quantize_reference(x, world, wire=W6).numpy()
        assert np.array_equal(got, want), (numel, world)
        q, s = R.split(got, world)
        first_pad = -(-numel // 32)
        assert (s[first_pad:] == 127).all() and not q[first_pad:].any()
        if numel % 32:
            assert not R.unpack_codes(q[first_pad - 1:first_pad])[0, numel % 32:].any()
        assert R.same(ops.mx_dequantize_reference(torch.from_numpy(got), numel, torch.float32, world, wire=W6),
                      R.dequantize(want, numel, world))
        # error feedback
        r = E.random_residual(numel, 5 + numel)
        want_w, want_r = R.quantize_ef(R.f32(x), r, world)
        res = torch.from_numpy(r.copy())
        got = ops.mx_quantize_reference(x, world, wire=W6, residual=res)
        assert np.array_equal(got.numpy(), want_w) and R.same_residual(res, want_r), (numel, world)


def test_rounding_probe_through_the_twins():
    v = R.rounding_probe()
    assert v.size > 120000 and (np.abs(v) == np.float32(7.5)).any() and (np.abs(v) == np.float32(0.0625)).any()
    for e in (0, -123, 60):
        x = R.probe_blocks(v, e).reshape(-1)
        assert np.array_equal(ops.mx_quantize_reference(torch.from_numpy(x), 1, wire=W6).numpy(), R.quantize(x, 1)), e
        got = ops.mx_quantize_reference(torch.from_numpy(x), 1, wire=W6, seed=e + 200, **SR)
        assert np.array_equal(got.numpy(), R.quantize(x, 1, (e + 200, 0, 0))), e


@pytest.mark.parametrize("W", WORLDS)
def test_shard_references_agree(W):
    edge = torch.from_numpy(R.edge_tensor()[0])
    for dtn, dt in R.DTYPES.items():
        cases = [(shard_inputs(m, max(W, 2), 50 + m, dt)[1][:W * m], m) for m in NUMELS[:-1]]
        x = shard_inputs(edge.numel(), max(W, 2), 7)[0][:W * edge.numel()].clone()
        x[(W - 1) * edge.numel():] = edge
        cases.append((x.to(dt), edge.numel()))
        for x, m in cases:
            want = R.quantize_shards(R.f32(x), W)
            got = ops.mx_quantize_shards_reference(x, W, wire=W6)
            assert got.numel() == ops.mx_shard_wire_bytes(m, W, wire=W6) == R.shard_wire_bytes(m, W) == want.size
            assert np.array_equal(got.numpy(), want), (dtn, m, W)
            for odt in R.DTYPES.values():
                d = ops.mx_dequantize_shards_reference(got, m, odt, W, wire=W6)
                assert d.dtype == odt and R.same(d, R.dequantize_shards(want, m, W, odt)), (dtn, m, W, odt)
            r = E.random_residual(W * m, 9 + m)
            want_w, want_r = R.quantize_shards_ef(R.f32(x), r, W)
            res = torch.from_numpy(r.copy())
            got = ops.mx_quantize_shards_reference(x, W, wire=W6, residual=res)
            assert np.array_equal(got.numpy(), want_w) and R.same_residual(res, want_r), (dtn, m, W)
            got = ops.mx_quantize_shards_reference(x, W, wire=W6, seed=m, stream=1, index_offset=(1 << 32) - 40, **SR)
            assert np.array_equal(got.numpy(), R.quantize_shards(R.f32(x), W, (m, 1, (1 << 32) - 40))), (dtn, m, W)
    x = shard_inputs(33, 2, 3)[0]
    assert not np.array_equal(R.quantize_shards(R.f32(x), 2)[:24 * 16], R.quantize(R.f32(x), 2)[:24 * 16])


@pytest.mark.parametrize("nsrc", range(1, 9))
def test_reduce_and_fold_references_fold_in_source_order(nsrc):
    for n in (48 * 32, 4113):
        xs = M8.rank_inputs(n, nsrc, 5 + nsrc)
        xs[nsrc - 1][:1024] = torch.from_numpy(R.edge_tensor()[0][:1024])  # NaN / inf / zero blocks too
        wire = np.concatenate([R.quantize(R.f32(x), 1) for x in xs])
        cb = R.chunk_blocks(n, 1)
        for op in ("sum", "avg"):
            got = ops.mx_reduce_reference(torch.from_numpy(wire), nsrc, op, wire=W6).numpy()
            assert np.array_equal(got, R.reduce(wire, nsrc, op)), (nsrc, n, op)
            for dt in R.DTYPES.values():
                f = ops.mx_fold_reference(torch.from_numpy(wire), nsrc, n, dt, op, wire=W6)
                assert f.dtype == dt and R.same(f, R.fold(wire, nsrc, n, op, dt)), (nsrc, n, op, dt)
            r2 = E.random_residual(32 * cb, nsrc)
            want_w, want_r = R.reduce_ef(wire, nsrc, op, r2)
            res = torch.from_numpy(r2.copy())
            got = ops.mx_reduce_reference(torch.from_numpy(wire), nsrc, op, wire=W6, residual=res)
            assert R.same_wire(got.numpy(), want_w, 1) and R.same_residual(res, want_r), (nsrc, n, op)
            got = ops.mx_reduce_reference(torch.from_numpy(wire), nsrc, op, wire=W6, seed=nsrc, stream=7, **SR)
            assert np.array_equal(got.numpy(), R.reduce(wire, nsrc, op, (nsrc, 7))), (nsrc, n, op)
        if nsrc >= 3:
            back = np.concatenate([R.quantize(R.f32(x), 1) for x in reversed(xs)])
            assert not R.same_wire(R.reduce(back, nsrc, "sum"), R.reduce(wire, nsrc, "sum"), 1)


def test_requantizing_a_dequantized_wire_changes_nothing():
    # D(Q(D(w))) == D(w) for every wire the quantizer can write (finite values: below 4 at scale 253)
    rng = np.random.default_rng(5)
    blocks = 2048
    code = rng.integers(0, 64, (blocks, 32)).astype(np.uint8)
    code[rng.random((blocks, 32)) < 0.3] = 0
    s = rng.integers(4, 253, blocks).astype(np.uint8)
    s[:32], s[32:64], s[64:96] = 4, 253, 255
    code[32:64] = (code[32:64] & 32) | np.minimum(code[32:64] & 31, 23)  # at most 3.75 2^126
    q = R.pack_codes(code)
    d = R.d_blocks(q, s)
    assert np.isfinite(d[s != 255]).all()
    assert R.same(torch.from_numpy(R.d_blocks(*R.q_blocks(d))), torch.from_numpy(d))
    dt = ops._mx6_dequantize_blocks(torch.from_numpy(q), torch.from_numpy(s))
    assert R.same(dt, torch.from_numpy(d))
    assert R.same(ops._mx6_dequantize_blocks(*ops._mx6_quantize_blocks(dt)), dt)
    assert ((np.abs(d) >= 2.0 ** -126) | (d == 0) | np.isnan(d)).all()  # normal f32 or zero


# ------------------------------------------------------------------ the layout and the headers
def test_layout_helpers_match_the_reference():
    for w in range(1, 9):
        for n in NUMELS + (0, 512 * w - 1, 512 * w + 1, BELOW * w, ABOVE * w, (1 << 33) + 5):
            assert ops.mx_chunk_blocks(n, w, wire=W6) == R.chunk_blocks(n, w), (n, w)
            assert ops.mx_wire_bytes(n, w, wire=W6) == R.wire_bytes(n, w) == 25 * R.chunk_blocks(n, w) * w
            assert ops.mx_owner_residual_numel(n, w, wire=W6) == 32 * R.chunk_blocks(n, w)
        for m in NUMELS + (BELOW, ABOVE):
            assert ops.mx_shard_blocks(m, wire=W6) == R.shard_blocks(m) == ops.mx_chunk_blocks(m, 1, wire=W6)
            assert ops.mx_shard_wire_bytes(m, w, wire=W6) == R.shard_wire_bytes(m, w)
    assert ops.mx_chunk_blocks(BELOW, 1, wire=W6) == 41936 and 25 * 41936 == (1 << 20) - 176
    assert ops.mx_chunk_blocks(ABOVE, 1, wire=W6) == 45056 and 25 * 41952 >= 1 << 20
    # ... at another place than for the other wires, whose values are unchanged
    assert ops.mx_chunk_blocks(BELOW, 1) == 45056 and ops.mx_chunk_blocks(BELOW, 1, wire="mxfp4_e2m1") == 41936
    assert ops.mx_wire_bytes(4096, 1) == 33 * 128 and ops.mx_wire_bytes(4096, 1, wire=W6) == 25 * 128
    assert ops.MX_WIRES == ("mxfp8_e4m3", "mxfp4_e2m1", "mxfp6_e2m3")


def _build() -> str:
    exe = os.path.join(BUILD, "mx6_check")
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


def _ask(queries, batch=4096):
    """The host program's answers to `queries`: one list of ints per query."""
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
        out += [[int(v) for v in ln.split()] for ln in lines[:-1]]
    assert len(out) == len(queries)
    return out


def test_host_program_self_check():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok" and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_layout_header_under_sanitizers():
    dealt = [(n, w) for w in (1, 2, 3, 8) for n in NUMELS + (512 * w - 1, 512 * w + 1, BELOW * w, ABOVE * w)]
    got = _ask([f"d:{n:x}:{w:x}" for n, w in dealt])
    assert got == [[R.chunk_blocks(n, w), R.wire_bytes(n, w)] for n, w in dealt]
    assert got == [[ops.mx_chunk_blocks(n, w, wire=W6), ops.mx_wire_bytes(n, w, wire=W6)] for n, w in dealt]
    shards = [(m, w) for w in (1, 3, 8) for m in NUMELS] + [(BELOW, 2), (ABOVE, 2)]
    got = _ask([f"s:{m:x}:{w:x}" for m, w in shards])
    assert got == [[R.shard_blocks(m), R.shard_wire_bytes(m, w)] for m, w in shards]
    cbs = (16, 48, 4096, 41936, 41952, 45056)  # below and at the 1 MiB rule
    assert _ask([f"c:{cb:x}" for cb in cbs]) == [[25 * cb, 24 * (cb - 1), 24 * cb, 25 * cb - 1] for cb in cbs]
    where = [(m, i) for m in (1, 5, 33, 96, 513) for i in (0, 1, m - 1, m, 2 * m + m // 2, 3 * m - 1)]
    where += [(4113, i) for i in range(4113, 4113 + 70)]  # every bit position of two blocks of the second shard
    assert _ask([f"p:{m:x}:{i:x}" for m, i in where]) == [[R.shard_payload_byte(m, i), R.shard_scale_byte(m, i)]
                                                          for m, i in where]
    # and the bytes are where the reference's wire has the element: flipping the element flips that byte
    m = 33
    x = np.full(3 * m, 7.5, dtype=np.float32)
    base = R.quantize_shards(x, 3)
    for i in (0, 5, 31, 32, 40, 70, 98):
        y = x.copy()
        y[i] = 7.0  # code 31 -> 30 under the same scale: the element's lowest bit
        diff = np.nonzero(R.quantize_shards(y, 3) != base)[0]
        assert diff.tolist() == [R.shard_payload_byte(m, i)], (i, diff)


def test_host_program_codes_equal_the_reference():
    """mx_sr_e2m3 on every grid point, every midpoint, their f32 neighbours and small values down to f32
    subnormals, each with u in {0, 1, T - 1, T, T + 1, 2^32 - 1}; both signs."""
    v = R.rounding_probe()
    v = np.concatenate([v[:900], v[v.size // 2:v.size // 2 + 900]])  # the grid, the midpoints, neighbours, small values
    assert (v < 0).any() and (np.abs(v) == np.float32(7.5)).any() and (np.abs(v) < np.float32(2.0 ** -126)).any()
    a = np.abs(v.astype(np.float64))
    lo = np.searchsorted(R.MAGS, a, side="right") - 1
    hi = np.minimum(lo + 1, 31)
    T = np.floor((a - R.MAGS[lo]) / np.where(hi > lo, R.MAGS[hi] - R.MAGS[lo], 1.0) * 4294967296.0).astype(np.uint64)
    queries, vals, words = [], [], []
    for x, bits, t in zip(v, _bits(v), T):
        for u in sorted({0, 1, max(int(t) - 1, 0), min(int(t), 0xFFFFFFFF), min(int(t) + 1, 0xFFFFFFFF), 0xFFFFFFFF}):
            queries.append(f"e2m3:{int(bits):x}:{u:x}")
            vals.append(x)
            words.append(u)
    pad = -len(vals) % 31
    xb = R.probe_blocks(np.array(vals + [0.0] * pad, dtype=np.float32))
    ub = np.concatenate([np.array(words + [0] * pad, dtype=np.uint64).reshape(-1, 31),
                         np.zeros((xb.shape[0], 1), dtype=np.uint64)], axis=1)
    want = R.codes_sr(xb, ub)[0][:, :31].reshape(-1)[:len(vals)]
    assert [g[0] for g in _ask(queries)] == want.tolist()


# ------------------------------------------------------------------ errors
def test_unknown_wires_raise_in_ops():
    x = torch.zeros(64)
    w = torch.zeros(25 * 16, dtype=torch.uint8)
    for bad in ("mxfp6", "mxfp4", "mxfp6_e3m2", None):
        for fn in (lambda: ops.mx_quantize_reference(x, 1, wire=bad), lambda: ops.mx_reduce_reference(w, 1, wire=bad),
                   lambda: ops.mx_dequantize_reference(w, 64, wire=bad), lambda: ops.mx_fold_reference(w, 1, 64, wire=bad),
                   lambda: ops.mx_quantize_shards_reference(x, 2, wire=bad),
                   lambda: ops.mx_dequantize_shards_reference(w, 64, wire=bad),
                   lambda: ops.mx_chunk_blocks(64, 1, wire=bad), lambda: ops.mx_wire_bytes(64, 1, wire=bad),
                   lambda: ops.mx_shard_blocks(64, wire=bad), lambda: ops.mx_shard_wire_bytes(64, 1, wire=bad),
                   lambda: ops.mx_owner_residual_numel(64, 1, wire=bad),
                   lambda: ops.mx_quantize(x, wire=bad), lambda: ops.mx_fold(w, 1, 64, wire=bad)):
            with pytest.raises(ValueError, match="unknown wire format .*mxfp8_e4m3, mxfp4_e2m1, mxfp6_e2m3"):
                fn()
    with pytest.raises(ValueError, match="'max'"):
        ops.mx_reduce_reference(w, 1, "max", wire=W6)
    with pytest.raises(TypeError, match="float64"):
        ops.mx_quantize_reference(torch.zeros(4, dtype=torch.float64), wire=W6)
    for other in (33, 17):  # an FP8- or FP4-sized wire is not an FP6 wire
        with pytest.raises(ValueError, match="400 bytes"):
            ops.mx_dequantize_reference(torch.zeros(other * 16, dtype=torch.uint8), 64, wire=W6)
        with pytest.raises(ValueError, match="400 bytes"):
            ops.mx_fold_reference(torch.zeros(other * 16, dtype=torch.uint8), 1, 64, wire=W6)
        with pytest.raises(ValueError, match="800 bytes"):
            ops.mx_dequantize_shards_reference(torch.zeros(other * 32, dtype=torch.uint8), 33, torch.float32, 2, wire=W6)
    with pytest.raises(ValueError, match="not a wire"):
        ops.mx_reduce_reference(torch.zeros(17 * 16, dtype=torch.uint8), 1, wire=W6)
    with pytest.raises(ValueError, match="alternatives"):
        ops.mx_quantize_reference(x, 1, wire=W6, residual=torch.zeros(64), **SR)
    from pytorch_distributed_collective_communication_amd.parallel import ddp
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    lin = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="'mxfp6'.*mxfp6_e2m3"):
        ddp.GradBucketer(lin, wire="mxfp6")
    with pytest.raises(ValueError, match="'mxfp6'.*mxfp6_e2m3"):
        ShardedOptimizer(lin.parameters(), param_wire="mxfp6")


# ------------------------------------------------------------------ the derived bounds
@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_error_bounds_against_f64_sums(world):
    """One scaled unit is 2^e < amax / 3.75 (the scaled amax lies in (3.75, 7.5]). In the top binade, 4 .. 7.5,
    the grid step is half a unit and nearest rounding errs by at most a quarter unit; a value can sit there only
    if the scaled amax is at least 4, so that error is at most amax / 16. Below the top binade the step is at
    most a quarter unit, the error an eighth, which is below amax / 30. The f32 fold adds far less (the 2^-10
    slack). Derived, not measured; every block has amax >= 2^-100 and no element is excluded.
    Worst fractions of the bound seen here (reduce-scatter, all-reduce, all-gather), normal and log-normal
    halves together: world 2: 0.784, 0.697, 0.940; 3: 0.778, 0.593, 0.939; 4: 0.754, 0.609, 0.940;
    8: 0.575, 0.503, 0.939."""
    rng = np.random.default_rng(60 + world)
    blocks = 1024
    xs = []
    for r in range(world):
        normal = rng.standard_normal((blocks // 2, 32))
        lognormal = np.exp(rng.standard_normal((blocks // 2, 32)) * 2.0) * rng.choice([-1.0, 1.0], (blocks // 2, 32))
        xs.append(np.concatenate([normal, lognormal]).astype(np.float32))
    amaxes = [np.abs(x).max(axis=1).astype(np.float64) for x in xs]
    assert min(a.min() for a in amaxes) >= 2.0 ** -100
    exact = np.sum([x.astype(np.float64) for x in xs], axis=0)
    ts = [torch.from_numpy(x.reshape(-1)) for x in xs]
    slack = 1 + 2.0 ** -10

    def share(got, bound):
        return float((np.abs(got.numpy().reshape(blocks, 32).astype(np.float64) - exact) / bound[:, None]).max())

    fold = R.fold_blocks([R.d_blocks(*R.q_blocks(x)) for x in xs], "sum")
    m = blocks // world * 32
    rs = torch.cat([R.reduce_scatter([t[:m * world] for t in ts], k) for k in range(world)])
    assert R.same(rs, torch.from_numpy(fold.reshape(-1)[:m * world]))
    rs_share = share(torch.from_numpy(fold.reshape(-1)), sum(amaxes) / 16 * slack)
    ar_share = share(R.all_reduce(ts), (sum(amaxes) + np.abs(fold).max(axis=1).astype(np.float64)) / 16 * slack)
    ag_share = 0.0
    for x, a in zip(xs, amaxes):
        g = R.all_gather([torch.from_numpy(x.reshape(-1))]).numpy().reshape(blocks, 32).astype(np.float64)
        ag_share = max(ag_share, float((np.abs(g - x.astype(np.float64)) / (a / 16)[:, None]).max()))
        sc = a / np.ldexp(1.0, R.scale_exponent((_bits(x) & 0x7FFFFFFF).max(axis=1)))
        assert (sc > 3.75).all() and (sc <= 7.5).all()  # the scaled amax
    print(f"world {world}: worst error / bound: reduce-scatter {rs_share:.3f}, all-reduce {ar_share:.3f}, "
          f"all-gather {ag_share:.3f}")
    assert rs_share <= 1.0 and ar_share <= 1.0 and ag_share <= 1.0, (rs_share, ar_share, ag_share)
    wire = torch.cat([ops.mx_quantize_reference(t, wire=W6) for t in ts])
    y = ops.mx_dequantize_reference(ops.mx_reduce_reference(wire, world, "sum", wire=W6), blocks * 32, wire=W6)
    assert R.same(y, R.all_reduce(ts))


@pytest.mark.parametrize("kind", ["normal", "lognormal"])
def test_error_feedback_series_stays_within_the_derived_bound(kind):
    """The protocol of the other wires (tests/_mx_ef_ref.py bound_series: 64 calls, 16384 elements): per element
    (a) |r_t| after every call, (b) |sum sent - sum x| at the end with feedback, each <= A_b / 15 (1 + 2^-10), A_b
    the largest block amax of x seen so far; (c) without feedback the sum leaves the bound. No element is left
    out. Measured here as fractions of the bound: normal 0.900, 0.859, 30.3; log-normal 0.929, 0.882, 53.0."""
    xs = E.bound_series(kind)
    T, n = xs.shape
    assert (T, n) == (64, 16384)
    res = torch.zeros(n)

    def step(x, use):
        xt = torch.from_numpy(x)
        if use:
            w = ops.mx_quantize_reference(xt, 1, wire=W6, residual=res)
            ref_w, ref_r = R.quantize_ef(x, step.r, 1)
            assert np.array_equal(w.numpy(), ref_w) and R.same_residual(res, ref_r)
            step.r = ref_r
            return R.dequantize(ref_w, n, 1).numpy(), res.numpy().copy()
        return R.dequantize(R.quantize(x, 1), n, 1).numpy(), None

    step.r = np.zeros(n, dtype=np.float32)
    A = np.zeros(n // 32, dtype=np.float64)
    sums = np.zeros((3, n), dtype=np.float64)
    worst_r, bound = 0.0, None
    for t in range(T):
        x = xs[t]
        A = np.maximum(A, np.abs(x.astype(np.float64)).reshape(-1, 32).max(axis=1))
        assert (A >= 2.0 ** -100).all()
        bound = np.repeat(A / R.BOUND_DIV * (1 + 2.0 ** -10), 32)
        sent, r = step(x, True)
        plain, _ = step(x, False)
        worst_r = max(worst_r, float((np.abs(r.astype(np.float64)) / bound).max()))
        sums += np.stack([x, sent, plain]).astype(np.float64)
    with_ef = float((np.abs(sums[1] - sums[0]) / bound).max())
    without = float((np.abs(sums[2] - sums[0]) / bound).max())
    print(f"{kind}: worst |r| {worst_r:.3f}, |sum sent - sum x| with feedback {with_ef:.3f}, without {without:.3f} (of the bound)")
    assert worst_r <= 1.0 and with_ef <= 1.0, (worst_r, with_ef)
    assert without > 1.0, without


@pytest.mark.parametrize("kind", ["normal", "lognormal"])
def test_the_mean_of_many_stochastic_calls_is_the_input(kind):
    """The protocol of the other wires: per element, |mean over 256 calls (seed 1234, stream t) of D(Q(x)) - x|
    stays within G 2^e_b sqrt(ln(2 n / 1e-6) / (2 T)) with G = 0.5 scaled units, the largest grid step --
    Hoeffding, all 4096 elements at once with probability 1 - 1e-6. No element is left out; nearest rounding
    leaves the bound. One call errs by less than one step, < amax / 8. Measured as fractions of the bound:
    stochastic 0.402 (normal), 0.378 (log-normal); nearest 2.358, 2.366; the worst single call 0.983 and 0.944
    of amax / 8."""
    x = E.bound_series(kind, n=4096, T=1)[0]
    xt = torch.from_numpy(x)
    calls = 256

    def ratio(quantize):
        mean = np.zeros(x.size, dtype=np.float64)
        worst_one = 0.0
        for t in range(calls):
            q, s = R.split(quantize(t).numpy(), 1)
            d = R.d_blocks(q, s).reshape(-1)[:x.size].astype(np.float64)
            amax = np.repeat(np.abs(x.astype(np.float64)).reshape(-1, 32).max(axis=1), 32)
            worst_one = max(worst_one, float((np.abs(d - x) / (amax / 8)).max()))
            mean += d
        e = s.astype(np.int64) - 127
        bound = R.STEP * np.ldexp(1.0, np.repeat(e, 32)[:x.size]) * math.sqrt(math.log(2 * x.size / 1e-6) / (2 * calls))
        return float((np.abs(mean / calls - x.astype(np.float64)) / bound).max()), worst_one

    sr, one = ratio(lambda t: ops.mx_quantize_reference(xt, 1, wire=W6, seed=1234, stream=t, **SR))
    near, _ = ratio(lambda t: ops.mx_quantize_reference(xt, 1, wire=W6))
    print(f"{kind}: stochastic {sr:.3f}, nearest {near:.3f} (of the bound); one call {one:.3f} of amax / 8")
    assert sr <= 1.0 and one < 1.0, (sr, one)
    assert near > 1.0, near
    got = ops.mx_quantize_reference(xt, 1, wire=W6, seed=1234, stream=3, **SR).numpy()
    assert np.array_equal(got, R.quantize(x, 1, (1234, 3, 0)))


# ------------------------------------------------------------------ the collectives on CPU tensors
@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_collectives_on_cpu_tensors(world):
    numels = (1, 33, 513) if world > 4 else (1, 33, 513, 4113)
    dtypes = tuple(R.DTYPES) if world == 2 else (("float32", "bfloat16") if world <= 4 else ("float32",))
    res = launch(M.collective_cases, world, args=("cpu", numels, dtypes))
    for r, got in enumerate(res):
        assert len(got) == len(dtypes) * len(numels) * M.CASES_PER_SIZE, sorted(got)
        bad = [k for k, v in got.items() if not v[0]]
        assert not bad, (r, bad)
        same = {k: v[1] for k, v in got.items() if not k.startswith("rs")}  # identical bits on every rank
        assert same == {k: v[1] for k, v in res[0].items() if not k.startswith("rs")}, r


def test_world_1_and_error_cases():
    got = launch(M.world1_and_errors, 1, args=("cpu",))[0]
    assert len(got) == 9 + M.N_ERRORS and all(got.values()), got
    for got in launch(M.world1_and_errors, 2, args=("cpu",)):
        assert len(got) == M.N_ERRORS and all(got.values()), got


@pytest.mark.parametrize("mode", ["plain", "ef", "sr"])
def test_grad_bucketer_with_the_fp6_wire_on_cpu_tensors(mode):
    res = launch(M.bucketer, 2, args=("cpu", mode))
    for got in res:
        assert got["buckets"] >= 2 and got["handles"] == ["CompressedWork"] and len(got["steps"]) == 3, got
        for t, step in enumerate(got["steps"]):
            for i in range(got["buckets"]):
                assert step[i][0], (t, i, step[i])
                assert step[i][1] == res[0]["steps"][t][i][1]  # the same bits on both ranks


@pytest.mark.parametrize("grad_wire,param_wire,mode", [(W6, W6, "plain"), ("mxfp4_e2m1", W6, "plain"), (W6, W6, "ef"),
                                                       (W6, W6, "sr")])
def test_sharded_optimizer_with_fp6_wires_on_cpu_tensors(grad_wire, param_wire, mode):
    res = launch(M.zero, 2, args=("cpu", grad_wire, param_wire, mode))
    for got in res:
        assert got["buckets"] >= 2 and got["handles"] == ["CompressedWork"] and len(got["steps"]) == 3, got
        for t, step in enumerate(got["steps"]):
            for i in range(got["buckets"]):
                assert step[i][0] and step[i][1], (t, i, step[i])
            assert step["digest"] == res[0]["steps"][t]["digest"]  # replicas agree
        assert got["restored"] == got["original"], got  # step 3 after a state_dict round trip, residuals included
        assert got["residual_nonzero"] in (None, True)
