"""Exact values for every reduce dtype without a GPU.

* the reference itself (tests/_exact.py `fold`, `same`) against hand-computed values, and against plain
  python integer arithmetic on the edge sets: it leaves no case out and masks nothing;
* the input builders: conditions on the inputs (ties of both parities, overflows, subnormal results,
  wraparound in SUM and PROD for every width), so the GPU tests that use them can tell a truncating
  narrowing, a signed uint8 or a half-width int64 compare from the real thing;
* the host reduction on integer edge values as a stand-alone program under ASan + UBSan
  (tests/native/cpu_reduce_check.cpp): the wraparound is computed without signed overflow;
* CPU tensors through the shm transport at worlds 2, 3 and 4 (csrc/host/cpu_reduce.h): every dtype, int16
  included, against the same reference with the same assertions as the GPU launches.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _exact as E
from tests import _workers_exact as X
from tests import _workers_fp8 as F

I8, U8, I16, I32, I64 = torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64


def _t(vals, dt):
    return torch.tensor(vals, dtype=dt)


# ------------------------------------------------------------------------------------------ the reference
def test_fold_integers_by_hand():
    f = lambda a, b, op, dt: E.fold([_t(a, dt), _t(b, dt)], op, dt).tolist()  # noqa: E731
    assert f([127, -128, -1], [1, -1, -1], "SUM", I8) == [-128, 127, -2]
    assert f([200, 255], [100, 1], "SUM", U8) == [44, 0]
    assert f([16, -128, 127], [16, -1, 127], "PRODUCT", I8) == [0, -128, 1]
    assert f([16, 255], [16, 255], "PRODUCT", U8) == [0, 1]
    # AVG: the WRAPPED sum, truncated toward zero
    assert f([127, -128, -3, 3, -1], [1, -1, 0, 0, 0], "AVG", I8) == [-64, 63, -1, 1, 0]
    assert f([200, 255], [100, 2], "AVG", U8) == [22, 0]
    assert f([2 ** 31 - 1], [1], "AVG", I32) == [-(2 ** 30)]
    assert f([2 ** 63 - 1, -7], [1, 0], "AVG", I64) == [-(2 ** 62), -3]
    # MIN / MAX in the dtype's own signedness
    assert f([200, 0], [100, 255], "MAX", U8) == [200, 255] and f([200, 0], [100, 255], "MIN", U8) == [100, 0]
    assert f([-56, 0], [100, -1], "MAX", I8) == [100, 0] and f([-56, 0], [100, -1], "MIN", I8) == [-56, -1]
    # int64 pairs that differ only in one dword
    a, b = 0x12345678_80000000, 0x12345678_7FFFFFFF
    assert f([a, -a], [b, -b], "MAX", I64) == [a, -b] and f([a, -a], [b, -b], "MIN", I64) == [b, -a]
    assert f([0x1_0000_0005], [5], "MAX", I64) == [0x1_0000_0005]
    assert f([2 ** 63 - 1], [2 ** 63 - 1], "SUM", I64) == [-2] and f([2 ** 63 - 1], [2], "PRODUCT", I64) == [-2]
    assert f([-2 ** 63], [-1], "PRODUCT", I64) == [-2 ** 63] and f([-2 ** 31], [-1], "PRODUCT", I32) == [-2 ** 31]
    assert f([0b1100], [0b1010], "BAND", I16) == [0b1000] and f([0b1100], [0b1010], "BOR", I16) == [0b1110]
    assert f([0b1100, -1], [0b1010, 1], "BXOR", I16) == [0b0110, -2]
    three = [_t([100], I8), _t([100], I8), _t([100], I8)]
    assert E.fold(three, "SUM", I8).tolist() == [44] and E.fold(three, "AVG", I8).tolist() == [14]


@pytest.mark.parametrize("dtn", ["int8", "uint8", "int16", "int32", "int64"])
def test_fold_integers_against_python_ints(dtn):
    # python's unbounded integers, wrapped by hand, over every pair of the edge set and three sources
    dt = E.DTYPES[dtn]
    bits = 8 * np.dtype(dtn).itemsize
    signed = dtn != "uint8"
    if bits == 8:
        a, b = E.byte_pairs(dtn)
        a, b = a[::37], b[::37]
    else:
        a, b = E.int_pairs(dtn)
        a, b = a[:len(E.int_edges(dtn)) ** 2], b[:len(E.int_edges(dtn)) ** 2]
    c = torch.roll(a, 7)

    def wrap(v):
        v &= (1 << bits) - 1
        return v - (1 << bits) if signed and v >> (bits - 1) else v

    def trunc_div(v, w):
        return -(-v // w) if v < 0 else v // w

    py = {"SUM": lambda x, y, z: wrap(x + y + z), "PRODUCT": lambda x, y, z: wrap(x * y * z),
          "AVG": lambda x, y, z: trunc_div(wrap(x + y + z), 3), "MIN": min, "MAX": max,
          "BAND": lambda x, y, z: x & y & z, "BOR": lambda x, y, z: x | y | z, "BXOR": lambda x, y, z: x ^ y ^ z}
    la, lb, lc = a.tolist(), b.tolist(), c.tolist()
    for op in E.INT_OPS:
        want = [py[op](x, y, z) for x, y, z in zip(la, lb, lc)]
        assert E.fold([a, b, c], op, dt).tolist() == want, (dtn, op)


def test_fold_bool_and_floats_by_hand():
    a, b = _t([0, 0, 1, 1], torch.bool), _t([0, 1, 0, 1], torch.bool)
    for op in ("SUM", "MAX", "BOR"):
        assert E.fold([a, b], op, torch.bool).tolist() == [False, True, True, True]
    for op in ("PRODUCT", "MIN", "BAND"):
        assert E.fold([a, b], op, torch.bool).tolist() == [False, False, False, True]
    assert E.fold([a, b], "BXOR", torch.bool).tolist() == [False, True, True, False]
    assert E.fold([a, b, b], "SUM", torch.bool).view(torch.uint8).tolist() == [0, 1, 1, 1]
    with pytest.raises(ValueError):
        E.fold([a, b], "AVG", torch.bool)
    with pytest.raises(ValueError):
        E.fold([_t([1.0], torch.float32)] * 2, "BXOR", torch.float32)
    nan, inf = float("nan"), float("inf")
    bf = torch.bfloat16
    # ties to even, one rounding: 1 + 2^-8 is a tie (-> 1), 1 + 2^-8 + 2^-8 is exact in fp32 (-> 1 + 2^-7)
    assert E.fold([_t([1.0], bf), _t([2.0 ** -8], bf)], "SUM", bf).float().tolist() == [1.0]
    assert E.fold([_t([1.0], bf), _t([2.0 ** -8], bf), _t([2.0 ** -8], bf)], "SUM", bf).float().tolist() == [1.0 + 2.0 ** -7]
    assert E.fold([_t([1.0 + 2.0 ** -7], bf), _t([2.0 ** -8], bf)], "SUM", bf).float().tolist() == [1.0 + 2.0 ** -6]
    big = torch.finfo(torch.float16).max
    assert E.fold([_t([big], torch.float16)] * 2, "SUM", torch.float16).tolist() == [inf]
    assert E.fold([_t([big], torch.float16)] * 2, "AVG", torch.float16).tolist() == [big]  # fp32 holds the sum
    # MIN / MAX: a NaN in either position wins
    for op in ("MIN", "MAX"):
        for dt in (torch.float16, bf, torch.float32, torch.float64):
            r = E.fold([_t([nan, 1.0, 2.0], dt), _t([1.0, nan, 1.0], dt)], op, dt)
            assert r.isnan().tolist() == [True, True, False] and r[2].item() == (1.0 if op == "MIN" else 2.0)
    # fp32 / f64 in their own precision, in list order
    x = [_t([1.0], torch.float32), _t([2.0 ** -24], torch.float32), _t([2.0 ** -24], torch.float32)]
    assert E.fold(x, "SUM", torch.float32).tolist() == [1.0] and E.fold(x[::-1], "SUM", torch.float32).tolist() == [1.0 + 2.0 ** -23]
    x64 = [t.double() for t in x]
    assert E.fold(x64, "SUM", torch.float64).tolist() == [1.0 + 2.0 ** -23]
    assert E.fold([_t([inf], torch.float32), _t([-inf], torch.float32)], "SUM", torch.float32).isnan().all()


def test_same_masks_nothing():
    f32 = torch.float32
    nan = float("nan")
    assert E.same(_t([0.0, nan, 1.0], f32), _t([-0.0, nan, 1.0], f32))
    assert not E.same(_t([1.0, nan], f32), _t([nan, nan], f32)) and not E.same(_t([nan, 1.0], f32), _t([nan, nan], f32))
    assert not E.same(_t([1.0], f32), _t([1.0 + 2.0 ** -23], f32))
    assert not E.same(_t([1.0], torch.float64), _t([1.0 + 2.0 ** -52], torch.float64))  # not compared in fp32
    assert not E.same(_t([float("inf")], f32), _t([-float("inf")], f32))
    assert not E.same(_t([1.0], f32), _t([1.0], torch.float64)) and not E.same(_t([1.0], f32), _t([1.0, 1.0], f32))
    assert E.same(_t([-2 ** 63, 5], I64), _t([-2 ** 63, 5], I64)) and not E.same(_t([2 ** 62], I64), _t([2 ** 62 + 1], I64))
    assert not E.same(_t([1], I8), _t([1], U8))
    two = _t([2], U8).view(torch.bool)  # a "true" whose byte is 2
    assert E.same(_t([True], torch.bool), _t([True], torch.bool)) and not E.same(two, _t([True], torch.bool))
    # the FP8 tests' reference is this one
    assert F.fold is E.fold and F.same is E.same


# ------------------------------------------------------------------------------------------ the builders
@pytest.mark.parametrize("dtn", ["bfloat16", "float16"])
def test_narrow_pairs_meet_ties_overflows_and_subnormals(dtn):
    dt = E.DTYPES[dtn]
    a, b = E.narrow_pairs(dtn)
    assert a.numel() == b.numel() == len(E.NARROW_PARTNERS) * 65536
    for k in range(len(E.NARROW_PARTNERS)):  # every encoding in every row
        assert torch.equal(a[k * 65536:(k + 1) * 65536].view(torch.int16).int() & 0xFFFF, torch.arange(65536, dtype=torch.int32))
    fi = torch.finfo(dt)
    s = a.float() + b.float()               # what the kernel has before it rounds
    drop = 23 - (7 if dtn == "bfloat16" else 10)  # fp32 mantissa bits the narrowing drops
    bits = s.view(torch.int32)
    normal = s.isfinite() & (s.abs() >= fi.smallest_normal) & (s.abs() < fi.max)
    tie = normal & ((bits & ((1 << drop) - 1)) == (1 << (drop - 1)))
    odd = ((bits >> drop) & 1) == 1
    assert int((tie & ~odd).sum()) >= 1000 and int((tie & odd).sum()) >= 1000
    # a truncating narrowing gets every odd tie and every tie's upper half wrong; count what RNE does with them
    r = s.to(dt)
    up = r.float().abs() > s.abs()
    assert int((tie & odd & up).sum()) == int((tie & odd).sum()) and int((tie & ~odd & up).sum()) == 0
    below = normal & ((bits & ((1 << drop) - 1)) == (1 << (drop - 2)))       # a quarter ulp: down
    above = normal & ((bits & ((1 << drop) - 1)) == (3 << (drop - 2)))       # three quarters: up
    assert int(below.sum()) >= 1000 and int((below & up).sum()) == 0
    assert int(above.sum()) >= 1000 and int((above & up).sum()) == int(above.sum())
    assert int((r.isinf() & s.isfinite()).sum()) >= 100                        # overflow to inf, no saturation
    sub = (r.float() != 0) & (r.float().abs() < fi.smallest_normal)
    assert int(sub.sum()) >= 100
    assert int((sub & (a.float().abs() >= fi.smallest_normal)).sum()) >= 1  # ... also from normal inputs
    assert int(s.isnan().sum()) >= 65536
    p = a.float() * b.float()
    assert int((p.to(dt).isinf() & a.float().isfinite() & b.float().isfinite()).sum()) >= 100  # PROD overflows too


@pytest.mark.parametrize("dtn", ["int8", "uint8", "int16", "int32", "int64"])
def test_integer_sets_wrap_and_cross_the_sign(dtn):
    dt = E.DTYPES[dtn]
    bits = 8 * np.dtype(dtn).itemsize
    a, b = E.byte_pairs(dtn) if bits == 8 else E.int_pairs(dtn)
    if bits == 8:
        assert len({(x, y) for x, y in zip(a.tolist(), b.tolist())}) == 65536
    else:
        es = bits // 8
        m = len(E.int_edges(dtn)) ** 2
        assert a.numel() >= m + 4099 and (a.numel() - 4099) * es >= 2 * 4096 and ((a.numel() - 4099) * es) % 4096 != 0
        need = {0, 1, -1, 2, -2, -(1 << (bits - 1)), -(1 << (bits - 1)) + 1, (1 << (bits - 1)) - 1, (1 << (bits - 1)) - 2}
        if bits == 64:
            need |= {0xFFFFFFFF, 0x1_0000_0000, -0x1_0000_0000, 0x7FFFFFFF_00000000, 0x80000000}
        assert need <= set(E.int_edges(dtn))
        assert {(x, y) for x in E.int_edges(dtn) for y in E.int_edges(dtn)} <= set(zip(a[:m].tolist(), b[:m].tolist()))
        rnd = a[-4099:].to(torch.int64)
        assert int((rnd < 0).sum()) > 1000 and int((rnd.abs() > (1 << (bits - 3))).sum()) > 1000  # full range
    la, lb = a.tolist(), b.tolist()
    lo, hi = (0, 255) if dtn == "uint8" else (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    wraps_sum = sum(1 for x, y in zip(la, lb) if not lo <= x + y <= hi)
    wraps_prod = sum(1 for x, y in zip(la, lb) if not lo <= x * y <= hi)
    assert wraps_sum >= 100 and wraps_prod >= 100, (wraps_sum, wraps_prod)
    neg_avg = sum(1 for x, y in zip(la, lb) if lo <= x + y <= hi and (x + y) < 0 and (x + y) % 2) if dtn != "uint8" else 1
    assert neg_avg >= 1  # truncation differs from flooring
    if dtn == "uint8":   # a signed compare orders these pairs the other way round
        assert sum(1 for x, y in zip(la, lb) if (x >= 128) != (y >= 128)) == 2 * 128 * 128
    if dtn == "int64":   # pairs that differ only in the low dword, bit 31 set in exactly one of them
        lowdiff = [(x, y) for x, y in zip(la, lb) if x != y and x >> 32 == y >> 32 and ((x ^ y) >> 31) & 1]
        highdiff = [(x, y) for x, y in zip(la, lb) if x != y and (x & 0xFFFFFFFF) == (y & 0xFFFFFFFF)]
        assert len(lowdiff) >= 8 and len(highdiff) >= 8


@pytest.mark.parametrize("dtn", ["float32", "float64"])
def test_wide_pairs_hold_the_edge_block(dtn):
    dt = E.DTYPES[dtn]
    a, b = E.wide_pairs(dtn)
    fi = torch.finfo(dt)
    es = a.element_size()
    assert (a.numel() - 4099) * es >= 2 * 4096 and ((a.numel() - 4099) * es) % 4096 != 0
    sub = lambda t: (t != 0) & (t.abs() < fi.smallest_normal)  # noqa: E731
    s, p = a + b, a * b
    assert int((s.isinf() & a.isfinite() & b.isfinite()).sum()) >= 2     # max + max
    assert int((p.isinf() & a.isfinite() & b.isfinite()).sum()) >= 2
    assert int((a.isinf() & b.isinf() & s.isnan()).sum()) >= 2           # inf + -inf
    assert int((a.isnan() & ~b.isnan()).sum()) >= 2 and int((~a.isnan() & b.isnan()).sum()) >= 2
    assert int((sub(a) | sub(b)).sum()) >= 10 and int(sub(s).sum()) >= 2 and int(sub(p).sum()) >= 1
    zero = lambda t: t == 0  # noqa: E731
    assert int((zero(a) & zero(b) & (torch.signbit(a) != torch.signbit(b))).sum()) >= 2   # +0 with -0
    xs = E.mixed_magnitudes(4099, dt, 8, 55)
    fwd, rev = E.fold(xs, "SUM", dt), E.fold(xs[::-1], "SUM", dt)
    assert int((fwd != rev).sum()) >= 100  # another order of the additions rounds differently
    assert int((fwd != _tree(xs, dt)).sum()) >= 100


def _tree(xs, dt):
    """The sum of xs as a pairwise tree (halves split recursively, the smaller one first: x0 + (x1 + x2) for
    three) in the accumulator precision of `fold`, cast to dt once."""
    def go(ys):
        return ys[0] if len(ys) == 1 else go(ys[:len(ys) // 2]) + go(ys[len(ys) // 2:])

    return go([x.to(dt if dt in E.WIDE.values() else torch.float32) for x in xs]).to(dt)


@pytest.mark.parametrize("nsrc", [3, 5, 8])
@pytest.mark.parametrize("dtn", ["bfloat16", "float16"])
def test_narrow_mixed_magnitudes_depend_on_the_order(dtn, nsrc):
    # the inputs of test_k1_narrow_wide_folds (same seed): after the cast to dt, the reversed fold and the
    # pairwise tree differ from the fold in list order, so a K1 that associates differently cannot pass
    dt = E.DTYPES[dtn]
    for n in (1023, 65536 + 17):
        xs = E.mixed_magnitudes(n, dt, nsrc, 4321 + n % 991)
        assert len(xs) == nsrc and all(x.dtype == dt and bool(x.isfinite().all()) for x in xs)
        fwd = E.fold(xs, "SUM", dt)
        assert bool(fwd.isfinite().all())
        rev, tree = E.fold(xs[::-1], "SUM", dt), _tree(xs, dt)
        assert int((fwd != rev).sum()) >= max(100, n // 2), int((fwd != rev).sum())
        assert int((fwd != tree).sum()) >= max(100, n // 2), int((fwd != tree).sum())
        # ... and rounding every partial sum to dt (an accumulator of the narrow type) differs as well
        acc = xs[0]
        for x in xs[1:]:
            acc = (acc.float() + x.float()).to(dt)
        assert int((fwd != acc).sum()) >= 100


def test_collective_inputs_and_the_pattern():
    for dtn, dt in E.DTYPES.items():
        if dtn.startswith("float8"):
            continue
        xs = E.collective_inputs(4099, dt, 3, 3)
        again = E.collective_inputs(4099, dt, 3, 3)
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(xs, again))
        if dt.is_floating_point:
            assert xs[0][0].isnan() and xs[2][-1].isnan() and xs[2][2].isinf() and xs[0][-3].isinf()
            assert all(x[1] == torch.finfo(dt).max and x[-2] == torch.finfo(dt).max for x in xs)
            assert E.fold(xs, "SUM", dt)[1].isinf()
        elif dt != torch.bool:
            bits = 8 * xs[0].element_size()
            assert int(xs[0].to(torch.int64).abs().max()) > (1 << (bits - 2))
    p = E.pattern(3 * 4096 + 77)
    for shift in (1, 16, 64, 256, 1024, 4096, 8192):
        assert int((p[shift:] != p[:-shift]).sum()) > 0.9 * (p.numel() - shift)


def test_guarded_slices_notice_a_stray_byte():
    x = E.random_bits(1001, torch.int16, 1)
    g = X.Guarded(x, torch.device("cpu"), 3)
    assert g.t.dtype == torch.int16 and torch.equal(g.t, x) and g.intact()
    g.arena[X.GUARD + g.nbytes] ^= 1   # the first byte after the payload
    assert not g.intact()
    g.arena[X.GUARD + g.nbytes] ^= 1
    g.arena[X.GUARD - 1] ^= 0x80
    assert not g.intact()


# ------------------------------------------------------------------------------------------ the host fold, sanitized
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
BUILD = os.path.join(ROOT, "build", "san")
SRC = os.path.join(ROOT, "tests", "native", "cpu_reduce_check.cpp")
HDR = os.path.join(CSRC, "host", "cpu_reduce.h")


def _build_cpu_reduce_check() -> str:
    exe = os.path.join(BUILD, "cpu_reduce_check")
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(p) for p in (SRC, HDR)):
        return exe
    os.makedirs(BUILD, exist_ok=True)
    tdir = os.path.dirname(torch.__file__)
    inc, lib = os.path.join(tdir, "include"), os.path.join(tdir, "lib")
    tmp = f"{exe}.{os.getpid()}.tmp"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}", f"-I{CSRC}", "-isystem", inc,
           "-isystem", os.path.join(inc, "torch", "csrc", "api", "include"), SRC, f"-L{lib}", "-lc10",
           f"-Wl,-rpath,{lib}", "-o", tmp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-6000:]
    os.replace(tmp, exe)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_fold_wraps_without_signed_overflow():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([_build_cpu_reduce_check()], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 10000, r.stdout[-2000:]


# ------------------------------------------------------------------------------------------ the shm transport
_CPU_DTYPES = ("float32", "float64", "bfloat16", "float16", "int8", "uint8", "int16", "int32", "int64", "bool")
_CPU_PLAN = tuple((dtn, n) for dtn in _CPU_DTYPES for n in (1, 1000, 4099))


@pytest.mark.parametrize("world", [2, 3, 4])
def test_cpu_tensors_through_the_shm_transport(world):
    res = launch(X.cpu_reductions, world, args=("cpu", _CPU_PLAN))
    # per size: 4 float dtypes x 7, 5 integer dtypes x 11, bool x 9; then AVG on bool and the check afterwards
    assert X.case_count(_CPU_PLAN) == 3 * (4 * 7 + 5 * 11 + 9) == 276
    for r, got in enumerate(res):
        bad = {k: v for k, v in got.items() if not v[0]}
        assert not bad, (r, bad)
        assert len(got) == 276 + 2, sorted(got)
