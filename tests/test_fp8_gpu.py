"""FP8 (float8_e4m3fn / float8_e5m2) reductions on the GPU: K1, every IPC protocol, the host engine
and the default engine selection.

One contract everywhere (docs/collectives.md): sources widened to fp32, folded in rank order in fp32,
rounded to FP8 once, the way torch's CPU cast rounds (nearest even, subnormals kept, no saturation).
The reference is always that CPU fold (tests/_workers_fp8.py `fold`), never a GPU cast or another
engine, and results must equal it as values: rtol = atol = 0, NaN where the reference is NaN.
"""
import functools

import pytest
import torch

from tests import _workers_fp8 as F
from tests.test_backend_gpu import _NUMERICS_ENV, _gpu_launch

pytestmark = pytest.mark.gpu

K1_OPS = {"sum": "SUM", "avg": "AVG", "prod": "PRODUCT", "min": "MIN", "max": "MAX"}
K1_IMPLS = ["lds", "regs", "lds_ntl", "stream", "stream_ntl"]


def _ops():
    from pytorch_distributed_collective_communication_amd import ops

    return ops


def _mismatch(got, ref, srcs):
    """The first few elements where `got` differs from `ref`, with their inputs (for the message)."""
    g, r = got.cpu().float(), ref.float()
    bad = ~((g == r) | (g.isnan() & r.isnan()))
    idx = bad.nonzero().flatten()[:8].tolist()
    return [(i, [float(s[i].float()) for s in srcs], float(g[i]), float(r[i])) for i in idx], int(bad.sum())


# ------------------------------------------------------------------ K1, every pair of encodings
@functools.lru_cache(maxsize=None)
def _pairs(dtn):
    """a[i] = byte(i >> 8), b[i] = byte(i & 255) for i < 65536 (16 tiles), and the reference per op."""
    dt = F.FP8[dtn]
    i = torch.arange(65536, dtype=torch.int32)
    a = (i >> 8).to(torch.uint8).view(dt)
    b = (i & 255).to(torch.uint8).view(dt)
    return a, b, {op: F.fold([a, b], K1_OPS[op], dt) for op in K1_OPS}


@pytest.mark.parametrize("impl", K1_IMPLS)
@pytest.mark.parametrize("dtn", list(F.FP8))
def test_k1_every_pair_of_encodings(dtn, impl):
    # every widening, every overflow / tie / subnormal / NaN case of the narrowing, and ±0
    ops = _ops()
    dev = torch.device("cuda", 0)
    a, b, refs = _pairs(dtn)
    ga, gb = a.to(dev), b.to(dev)
    for op, ref in refs.items():
        got = ops.reduce_nway([ga, gb], op=op, impl=impl)
        assert got.dtype == ref.dtype
        if not F.same(got, ref):
            first, count = _mismatch(got, ref, [a, b])
            pytest.fail(f"{dtn} {op} {impl}: {count} of 65536 pairs differ; (i, inputs, got, want): {first}")


# ------------------------------------------------------------------ K1, ragged sizes and wide folds
@pytest.mark.parametrize("nsrc", [3, 5, 8])
@pytest.mark.parametrize("dtn", list(F.FP8))
def test_k1_ragged_sizes_and_wide_folds(dtn, nsrc):
    ops = _ops()
    dev = torch.device("cuda", 0)
    dt = F.FP8[dtn]
    for n in (1, 3, 1023, 4099, 65536 + 17):
        def rand(k, lo, hi):
            g = torch.Generator().manual_seed(4321 + 17 * k + n % 991)
            return (lo + (hi - lo) * torch.rand(n, generator=g)).to(dt)

        xs = [rand(k, -2.0, 2.0) for k in range(nsrc)]
        xp = [rand(k, 0.5, 1.5) for k in range(nsrc)]
        for op in K1_OPS:
            srcs = xp if op == "prod" else xs
            ref = F.fold(srcs, K1_OPS[op], dt)
            gs = [s.to(dev) for s in srcs]
            for impl in ("lds", "regs", "stream_ntl"):
                got = ops.reduce_nway(gs, op=op, impl=impl)
                if not F.same(got, ref):
                    first, count = _mismatch(got, ref, srcs)
                    pytest.fail(f"{dtn} {op} {impl} nsrc={nsrc} n={n}: {count} differ; {first}")
        # in place: out = srcs[0]
        gs = [s.to(dev) for s in xs]
        got = ops.reduce_nway(gs, out=gs[0], op="sum")
        assert got.data_ptr() == gs[0].data_ptr()
        assert F.same(got, F.fold(xs, "SUM", dt)), (dtn, nsrc, n, "in place")


def test_k1_rejects_bitwise_ops_and_fnuz():
    ops = _ops()
    dev = torch.device("cuda", 0)
    x = torch.ones(64, device=dev).to(torch.float8_e4m3fn)
    with pytest.raises(RuntimeError, match="unsupported for"):
        ops.reduce_nway([x, x], op="bxor")
    z = torch.ones(64, device=dev).to(torch.float8_e4m3fnuz)  # the gfx942 format stays out
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        ops.reduce_nway([z, z], op="sum")


# ------------------------------------------------------------------ every IPC protocol, ranks sharing GPU 0
# sizes in bytes (= elements), chosen so a 1-byte dtype meets each protocol's thresholds
_PROTOCOL_SIZES = {
    "ll": (1, 777, 65521),
    "oneshot": (160037,),
    "twoshot": (1200007,),
    "zc": (2800003, 8000011),
    "push": (2800003,),
    "staged_algo": (2800003,),
    "dyn": (2800003, 9000011),
}
_PROTOCOL_WORLDS = {"ll": (2, 3), "oneshot": (2,), "twoshot": (2, 3), "zc": (2, 3), "push": (2,),
                    "staged_algo": (2,), "dyn": (2,)}


@pytest.mark.parametrize("mode,world", [(m, w) for m in _PROTOCOL_SIZES for w in _PROTOCOL_WORLDS[m]])
def test_every_ipc_protocol(mode, world):
    env, want = _NUMERICS_ENV[mode]
    sizes = _PROTOCOL_SIZES[mode]
    res = _gpu_launch(F.reductions, world, args=("cuda", sizes, True), env=env, timeout_s=120)
    for r in res:
        bad = {k: v for k, v in r.items() if not v[0]}
        assert not bad, bad
        assert len(r) == 2 * len(sizes) * 7, sorted(r)
        # a size that slipped into another protocol must fail, not pass on the wrong path
        engines = {v[1] for k, v in r.items() if k.startswith("all_reduce/")}
        if mode in ("twoshot", "staged_algo"):
            assert engines == {"ipc_2shot"}, engines
        else:
            assert all(e.startswith(want) for e in engines), engines


# ------------------------------------------------------------------ host engine, default selection
def test_host_engine():
    res = _gpu_launch(F.host_engine, 2, env={"PDCC_ALGO": "host"})
    for r in res:
        bad = {k: v for k, v in r.items() if not v[0]}
        assert not bad, bad
        assert len(r) == 4 and {v[1] for v in r.values()} == {"host"}, r


def test_default_selection_never_offers_rccl():
    # RCCL has no FP8 reduction here (a ring rounds at every hop): the static choice is IPC at
    # every size, and the autotuner's rows for these dtypes hold no RCCL engine
    res = _gpu_launch(F.default_selection, 2, timeout_s=120)
    for r in res:
        bad = {k: v for k, v in r["cases"].items() if not v[0]}
        assert not bad, bad
        assert len(r["cases"]) == 8
        assert all(v[1].startswith("ipc") for v in r["cases"].values()), r["cases"]
        rows = [e for e in r["table"] if e["dtype"].startswith("Float8")]
        assert all(e["dtype"] in ("Float8_e4m3fn", "Float8_e5m2") for e in rows), rows
        assert not [e for e in rows if e["algo"].startswith("rccl")], rows
    assert res[0]["table"] == res[1]["table"]
