"""Exact values for every reduce dtype on the GPU: K1 on one GPU, guard bands around K1 / K2 outputs, every
IPC protocol and the host engine with the ranks sharing GPU 0.

The reference is always `tests/_exact.py` `fold` (CPU, shares no code with the kernels) and every comparison
is `same(got, fold(...))`: no tolerance anywhere. See docs/collectives.md for the contract per dtype.
"""
import functools

import pytest
import torch

from tests import _exact as E
from tests import _workers_exact as X
from tests.test_backend_gpu import _NUMERICS_ENV, _gpu_launch
from tests.test_fp8_gpu import _PROTOCOL_SIZES, _PROTOCOL_WORLDS

pytestmark = pytest.mark.gpu

K1_IMPLS = ["lds", "regs", "lds_ntl", "stream", "stream_ntl"]
RAGGED = (1, 3, 1023, 4099, 65536 + 17)


def _ops():
    from pytorch_distributed_collective_communication_amd import ops

    return ops


def _dev():
    return torch.device("cuda", 0)


def _check(got, ref, srcs, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    if not E.same(got, ref):
        count, first = E.mismatch(got, ref, srcs)
        pytest.fail(f"{what}: {count} of {ref.numel()} differ; (i, inputs, got, want): {first}")


def _k1_all_ops(srcs, refs, impl, what, **kw):
    ops = _ops()
    gs = [s.to(_dev()) for s in srcs]
    for op, ref in refs.items():
        got = ops.reduce_nway(gs, op=E.K1_OP[op], impl=impl, **kw)
        _check(got, ref, srcs, f"{what} {op} {impl}")


@functools.lru_cache(maxsize=None)
def _pair_case(kind, dtn):
    """(srcs, {op: reference}) of a two-source builder, computed once for all impls."""
    a, b = {"bytes": E.byte_pairs, "ints": E.int_pairs, "narrow": E.narrow_pairs, "wide": E.wide_pairs}[kind](dtn)
    dt = E.DTYPES[dtn]
    return (a, b), {op: E.fold([a, b], op, dt) for op in E.ops_for(dt)}


# ------------------------------------------------------------------------------------------ K1, integers
@pytest.mark.parametrize("impl", K1_IMPLS)
@pytest.mark.parametrize("dtn", ["int8", "uint8"])
def test_k1_every_pair_of_bytes(dtn, impl):
    # all 65 536 pairs: wraparound of SUM / PROD, AVG of a wrapped sum, MIN / MAX across the sign bit
    srcs, refs = _pair_case("bytes", dtn)
    assert len(refs) == 8
    _k1_all_ops(srcs, refs, impl, dtn)


@pytest.mark.parametrize("impl", K1_IMPLS)
@pytest.mark.parametrize("dtn", ["int32", "int64"])
def test_k1_integer_edges(dtn, impl):
    # every pair of edge values (MIN, MAX, dword boundaries) over two tiles and a ragged tail, then random bits
    srcs, refs = _pair_case("ints", dtn)
    assert len(refs) == 8
    _k1_all_ops(srcs, refs, impl, dtn)


@functools.lru_cache(maxsize=None)
def _random_case(dtn, nsrc, n):
    dt = E.DTYPES[dtn]
    srcs = tuple(E.random_bits(n, dt, 1000 * nsrc + 7 * k + n % 991) for k in range(nsrc))
    return srcs, {op: E.fold(list(srcs), op, dt) for op in E.ops_for(dt)}


@pytest.mark.parametrize("impl", ["lds_ntl", "stream"])
@pytest.mark.parametrize("dtn", ["int8", "uint8", "int32", "int64"])
def test_k1_integers_every_source_count(dtn, impl):
    for nsrc in range(1, 9):
        for n in RAGGED:
            srcs, refs = _random_case(dtn, nsrc, n)
            assert len(refs) == 8
            _k1_all_ops(srcs, refs, impl, f"{dtn} nsrc={nsrc} n={n}")


@pytest.mark.parametrize("impl", ["lds_ntl", "stream"])
def test_k1_bool(impl):
    ops = _ops()
    for nsrc in range(1, 9):
        for n in RAGGED:
            srcs, refs = _random_case("bool", nsrc, n)
            assert len(refs) == 7
            gs = [s.to(_dev()) for s in srcs]
            for op, ref in refs.items():
                got = ops.reduce_nway(gs, op=E.K1_OP[op], impl=impl)
                assert got.dtype == torch.bool
                raw = got.view(torch.uint8).cpu()
                assert int(raw.max()) <= 1, (op, nsrc, n, "a result byte is neither 0 nor 1")
                _check(got, ref, srcs, f"bool {op} nsrc={nsrc} n={n} {impl}")
    x = torch.ones(64, dtype=torch.bool, device=_dev())
    with pytest.raises(RuntimeError, match="unsupported for"):
        ops.reduce_nway([x, x], op="avg", impl=impl)


# ------------------------------------------------------------------------------------------ K1, floats
@pytest.mark.parametrize("impl", K1_IMPLS)
@pytest.mark.parametrize("dtn", ["bfloat16", "float16"])
def test_k1_every_narrow_encoding(dtn, impl):
    # every encoding against ±0, subnormal, 1, max, inf, NaN and partners that put the fp32 sum on, below and
    # above a rounding tie (tests/test_exact_cpu.py counts the ties, overflows and subnormal results)
    srcs, refs = _pair_case("narrow", dtn)
    assert len(refs) == 5
    _k1_all_ops(srcs, refs, impl, dtn)


@functools.lru_cache(maxsize=None)
def _mixed_case(dtn, nsrc, n):
    dt = E.DTYPES[dtn]
    xs = E.mixed_magnitudes(n, dt, nsrc, 4321 + n % 991)
    xp = [E.random_values(n, dt, 77 + 17 * k + n % 991, 0.5, 1.5) for k in range(nsrc)]
    return {op: ((xp if op == "PRODUCT" else xs), E.fold(xp if op == "PRODUCT" else xs, op, dt))
            for op in E.FLOAT_OPS}


@pytest.mark.parametrize("nsrc", [3, 5, 8])
@pytest.mark.parametrize("dtn", ["bfloat16", "float16"])
def test_k1_narrow_wide_folds(dtn, nsrc):
    # sources of mixed magnitude with cancellation: the fp32 fold in source order, rounded once. Another
    # association (reversed, a pairwise tree) or a narrow accumulator differs in most elements of these inputs
    # (tests/test_exact_cpu.py test_narrow_mixed_magnitudes_depend_on_the_order counts them)
    ops = _ops()
    for n in RAGGED:
        for op, (srcs, ref) in _mixed_case(dtn, nsrc, n).items():
            gs = [s.to(_dev()) for s in srcs]
            for impl in ("lds", "regs", "stream_ntl"):
                _check(ops.reduce_nway(gs, op=E.K1_OP[op], impl=impl), ref, srcs, f"{dtn} {op} {impl} nsrc={nsrc} n={n}")


@functools.lru_cache(maxsize=None)
def _wide_case(dtn, nsrc):
    dt = E.DTYPES[dtn]
    a, b = E.wide_pairs(dtn)
    # further sources: the same edge block and random tail, rotated, so every position still meets an edge
    srcs = [a, b] + [torch.roll(a if k % 2 else b, 5 * k + 1) for k in range(2, nsrc)]
    return srcs, {op: E.fold(srcs, op, dt) for op in E.FLOAT_OPS}


@pytest.mark.parametrize("impl", K1_IMPLS)
@pytest.mark.parametrize("nsrc", [2, 3, 8])
@pytest.mark.parametrize("dtn", ["float32", "float64"])
def test_k1_float32_float64(dtn, nsrc, impl):
    # own-precision fold in source order: ±0, subnormals, overflow to inf, inf - inf, NaN in either position
    srcs, refs = _wide_case(dtn, nsrc)
    _k1_all_ops(srcs, refs, impl, f"{dtn} nsrc={nsrc}")
    if nsrc == 8:  # and a fold whose result depends on the association
        for n in (1023, 4099):
            xs = E.mixed_magnitudes(n, E.DTYPES[dtn], 8, 55 + n)
            _k1_all_ops(xs, {op: E.fold(xs, op, E.DTYPES[dtn]) for op in ("SUM", "AVG")}, impl, f"{dtn} mixed n={n}")


# ------------------------------------------------------------------------------------------ K1, call forms
@pytest.mark.parametrize("dtn", ["int8", "uint8", "int32", "int64", "bool", "bfloat16", "float16", "float32",
                                 "float64"])
def test_k1_in_place(dtn):
    ops = _ops()
    dt = E.DTYPES[dtn]
    n = 4099
    if dt.is_floating_point:
        srcs = E.mixed_magnitudes(n, dt, 3, 91)
    else:
        srcs = [E.random_bits(n, dt, 91 + k) for k in range(3)]
    for op in ("SUM", "MAX"):
        gs = [s.to(_dev()) for s in srcs]
        got = ops.reduce_nway(gs, out=gs[0], op=E.K1_OP[op])
        assert got.data_ptr() == gs[0].data_ptr()
        _check(got, E.fold(srcs, op, dt), srcs, f"{dtn} {op} in place")
        for k in (1, 2):
            assert torch.equal(gs[k].cpu().view(torch.uint8), srcs[k].view(torch.uint8)), "a source changed"


@pytest.mark.parametrize("max_blocks", [1, 7])
@pytest.mark.parametrize("dtn", ["uint8", "bfloat16", "int32", "float64"])  # element widths 1, 2, 4, 8
def test_k1_max_blocks(dtn, max_blocks):
    dt = E.DTYPES[dtn]
    n = 65536 + 17
    if dt.is_floating_point:
        srcs = E.mixed_magnitudes(n, dt, 3, 13)
    else:
        srcs = [E.random_bits(n, dt, 13 + k) for k in range(3)]
    refs = {op: E.fold(srcs, op, dt) for op in ("SUM", "AVG", "MIN")}
    for impl in K1_IMPLS:
        _k1_all_ops(srcs, refs, impl, f"{dtn} max_blocks={max_blocks}", max_blocks=max_blocks)


# ------------------------------------------------------------------------------------------ guard bands
FRONT, BACK = 4096, 8192


def _arena(nbytes, salt):
    """A GPU byte arena holding the pattern, the CPU pattern, and the payload's byte range: FRONT bytes of
    guard, the payload (16-B aligned), BACK bytes of guard after its last valid byte."""
    total = FRONT + nbytes + BACK
    pat = E.pattern(total, salt)
    arena = pat.to(_dev())
    assert arena.data_ptr() % 16 == 0
    return arena, pat, FRONT, FRONT + nbytes


def _guard_sizes(esize):
    ns = set()
    for nbytes in (1, 15, 17, 4095, 4097, 16 * 4096 - 4, 16 * 4096, 16 * 4096 + 4):
        ns.add(max(1, nbytes // esize))       # the largest n at or below the byte size ...
        ns.add((nbytes + esize - 1) // esize)  # ... and the smallest at or above it
    return sorted(ns)


@pytest.mark.parametrize("impl", K1_IMPLS)
@pytest.mark.parametrize("dtn", ["uint8", "bfloat16", "float32", "int64"])  # element widths 1, 2, 4, 8
def test_k1_writes_nothing_outside_the_output(dtn, impl):
    ops = _ops()
    dt = E.DTYPES[dtn]
    esize = torch.empty(0, dtype=dt).element_size()
    for n in _guard_sizes(esize):
        if dt.is_floating_point:
            srcs = [E.random_values(n, dt, 5 + k + n) for k in range(2)]
        else:
            srcs = [E.random_bits(n, dt, 5 + k + n) for k in range(2)]
        ref = E.fold(srcs, "SUM", dt)
        arena, pat, lo, hi = _arena(n * esize, n)
        out = arena[lo:hi].view(dt)
        got = ops.reduce_nway([s.to(_dev()) for s in srcs], out=out, op="sum", impl=impl)
        assert got.data_ptr() == arena.data_ptr() + lo
        after = arena.cpu()
        what = f"{dtn} {impl} n={n} ({n * esize} bytes)"
        assert torch.equal(after[:lo], pat[:lo]), f"{what}: bytes in front of the output changed"
        changed = (after[hi:] != pat[hi:]).nonzero().flatten()
        assert changed.numel() == 0, f"{what}: bytes after the output changed, first at +{int(changed[0])}"
        _check(after[lo:hi].view(dt), ref, srcs, what)


def _k2_layout(ndesc):
    """(src offset, dst offset, bytes) per member, in bytes: lengths through every path (empty, below a
    vector, ragged tiles, whole tiles), offsets 16-B aligned, 4-B aligned and odd mixed on both sides, at
    least 32 bytes of gap between destinations."""
    lens = [1, 16, 0, 4096, 17, 5000, 0, 8192 + 5, 3, 4095, 100, 4097, 12288, 15, 64, 1000]
    dst_mis = [0, 0, 4, 0, 1, 0, 0, 0, 0, 8, 0, 3, 0, 0, 12, 0, 7]
    src_mis = [0, 0, 0, 0, 1, 4, 0, 0, 0, 0, 0, 5, 0, 0, 0, 2, 0, 0, 8]
    out, s, d = [], 0, FRONT
    for i in range(ndesc):
        ln = lens[i % len(lens)]
        so = (s + 15) // 16 * 16 + src_mis[i % len(src_mis)]
        do = (d + 32 + 15) // 16 * 16 + dst_mis[i % len(dst_mis)]
        out.append((so, do, ln))
        s, d = so + ln, do + ln
    return out, s, d


@pytest.mark.parametrize("ndesc", [63, 64, 65, 129])  # around the per-launch descriptor limit and the host split
def test_k2_multi_copy_writes_exactly_its_destinations(ndesc):
    ops = _ops()
    layout, src_end, dst_end = _k2_layout(ndesc)
    assert any(ln == 0 for _, _, ln in layout[1:-1])
    assert {do % 16 == 0 for _, do, _ in layout} == {True, False} and any(do % 2 for _, do, _ in layout)
    src_cpu = E.random_bits(src_end + BACK, torch.uint8, 3 + ndesc)
    src = src_cpu.to(_dev())
    pat = E.pattern(dst_end + BACK, ndesc)
    want = pat.clone()
    for so, do, ln in layout:
        want[do:do + ln] = src_cpu[so:so + ln]
    for depth in (4, 8):
        for ntl in (True, False):
            for max_blocks in (1, 7):
                arena = pat.to(_dev())
                ops.multi_copy([src[so:so + ln] for so, _, ln in layout], [arena[do:do + ln] for _, do, ln in layout],
                               max_blocks=max_blocks, depth=depth, ntl=ntl)
                after = arena.cpu()
                bad = (after != want).nonzero().flatten()
                assert bad.numel() == 0, (ndesc, depth, ntl, max_blocks, f"{bad.numel()} bytes differ, first at "
                                          f"{int(bad[0])}", [m for m in layout if m[1] - 64 <= int(bad[0]) <= m[1] + m[2] + 64])
    assert torch.equal(src.cpu(), src_cpu)


# ------------------------------------------------------------------------ every IPC protocol, ranks sharing GPU 0
# sizes in BYTES per protocol (n = bytes // element size) and the worlds: the table of tests/test_fp8_gpu.py
_LAUNCHES = {"ints": ("int8", "uint8", "int32", "int64", "bool"),
             "floats": ("float32", "float64", "bfloat16", "float16")}
# where a mode has more than one bulk size (zc, dyn), the largest runs for this dtype only, to keep a launch
# at a few seconds; a mode's only size, and the three small LL sizes, run for every dtype of the launch
_LARGEST_FOR = {"ints": "int32", "floats": "float32"}


def _plan(mode, which):
    """((dtype name, n), ...) of one launch."""
    sizes = _PROTOCOL_SIZES[mode]
    plan = []
    for dtn in _LAUNCHES[which]:
        es = torch.empty(0, dtype=E.DTYPES[dtn]).element_size()
        for b in sizes:
            if len(sizes) > 1 and b == max(sizes) and mode != "ll" and dtn != _LARGEST_FOR[which]:
                continue
            plan.append((dtn, max(1, b // es)))
    # at least one payload of the mode that is no multiple of 16 bytes
    assert any((n * torch.empty(0, dtype=E.DTYPES[d]).element_size()) % 16 for d, n in plan), plan
    return tuple(plan)


def _assert_results(res, plan, mode, want):
    for r in res:
        bad = {k: v for k, v in r.items() if not v[0]}
        assert not bad, bad
        assert len(r) == X.case_count(plan), (len(r), X.case_count(plan), sorted(r))
        engines = {v[1] for k, v in r.items() if k.startswith("all_reduce/")}
        if mode in ("twoshot", "staged_algo"):
            assert engines == {"ipc_2shot"}, engines
        else:
            assert all(e.startswith(want) for e in engines), engines


@pytest.mark.parametrize("which", list(_LAUNCHES))
@pytest.mark.parametrize("mode,world", [(m, w) for m in _PROTOCOL_SIZES for w in _PROTOCOL_WORLDS[m]])
def test_every_ipc_protocol(mode, world, which):
    env, want = _NUMERICS_ENV[mode]
    plan = _plan(mode, which)
    res = _gpu_launch(X.reductions, world, args=("cuda", plan), env=env, timeout_s=120)
    _assert_results(res, plan, mode, want)


def test_oneshot_world4():
    # the W = 4 instantiation of the staged kernels: integers and bf16, small sizes; float32 too, whose sum of
    # four ranks depends on the order of the additions
    env, want = _NUMERICS_ENV["oneshot"]
    plan = tuple((dtn, n) for dtn in ("int8", "uint8", "int32", "int64", "bfloat16", "float32")
                 for n in (1, 4099, 20011))
    assert X.case_count(plan) == 3 * (4 * 11 + 7 + 7) == 174
    res = _gpu_launch(X.reductions, 4, args=("cuda", plan), env=env, timeout_s=120)
    _assert_results(res, plan, "oneshot", want)


def test_host_engine_every_dtype():
    # int16 has no kernel: the label must say the host engine ran, for it and (forced) for everything else
    dts = tuple(E.WIDE) + ("bfloat16", "float16") + tuple(E.INTS) + ("bool",)
    res = _gpu_launch(X.host_engine, 2, args=("cuda", dts, 4099), env={"PDCC_ALGO": "host"}, timeout_s=120)
    for r in res:
        bad = {k: v for k, v in r.items() if not v[0]}
        assert not bad, bad
        assert len(r) == 2 * len(dts) == 20 and {v[1] for v in r.values()} == {"host"}, r
