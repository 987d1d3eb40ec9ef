"""Error feedback on the block-scaled wires (docs/collectives.md "Error feedback"), everything that
needs no GPU: the `ops.*_reference` twins against the independent numpy reference tests/_mx_ef_ref.py
bit for bit (wire and residual), the edge blocks, the derived bound and the telescoping sum, the
collectives over the shm transport against a single-process simulation, world 1 and every error.
"""
import functools

import numpy as np
import pytest
import torch

from pytorch_distributed_collective_communication_amd import ops
from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _mx_ef_ref as E
from tests import _workers_mx_ef as M
from tests._workers_mx import rank_inputs

WIRES = tuple(E.WIRES)
NUMELS = (1, 31, 32, 33, 513, 4113)
SHARDS = (1, 33, 64, 513)
WORLDS = (1, 3, 8)


@functools.lru_cache(maxsize=None)
def _x(n, dtn, seed=0):
    return rank_inputs(n, 2, 500 + n + seed, E.DTYPES[dtn])[1]


def _assert_wire(R, got, ref, nchunks, what):
    assert R.same_wire(got.numpy(), ref, nchunks), what


# ------------------------------------------------------------------ the references, bit for bit
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("dtn", list(E.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_quantize_reference(wire, dtn, world):
    R = E.WIRES[wire]
    for n in NUMELS:
        x = _x(n, dtn)
        r0 = E.random_residual(n, 900 + n)
        want_w, want_r = E.quantize(R.f32(x), r0, world, wire)
        keep = x.clone()
        res = torch.from_numpy(r0.copy())
        got = ops.mx_quantize_reference(x, world, wire=wire, residual=res)
        _assert_wire(R, got, want_w, world, (wire, dtn, world, n))
        assert E.same_residual(res, want_r), (wire, dtn, world, n)
        assert torch.equal(x.view(torch.uint8), keep.view(torch.uint8))  # x is not modified
        assert not np.array_equal(want_r, r0)  # (the residual did change)


@pytest.mark.parametrize("W", WORLDS)
@pytest.mark.parametrize("dtn", list(E.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_quantize_shards_reference(wire, dtn, W):
    R = E.WIRES[wire]
    for m in SHARDS:
        x = _x(W * m, dtn, seed=7)
        r0 = E.random_residual(W * m, 901 + m)
        want_w, want_r = E.quantize_shards(R.f32(x), r0, W, wire)
        res = torch.from_numpy(r0.copy())
        got = ops.mx_quantize_shards_reference(x, W, wire=wire, residual=res)
        _assert_wire(R, got, want_w, W, (wire, dtn, W, m))
        assert E.same_residual(res, want_r), (wire, dtn, W, m)


@pytest.mark.parametrize("op", ["sum", "avg"])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 8])
@pytest.mark.parametrize("wire", WIRES)
def test_reduce_reference(wire, nsrc, op):
    R = E.WIRES[wire]
    for n in (48 * 32, 4113):
        xs = rank_inputs(n, nsrc, 40 + nsrc)
        xs[nsrc - 1][:1024] = torch.from_numpy(E.R4.edge_tensor()[0][:1024])  # NaN, inf and zero blocks
        w = np.concatenate([R.quantize(R.f32(x), 1) for x in xs])
        r0 = E.random_residual(E.owner_numel(n, 1, wire), 77)
        want_w, want_r = E.reduce(w, nsrc, op, r0, wire)
        res = torch.from_numpy(r0.copy())
        got = ops.mx_reduce_reference(torch.from_numpy(w), nsrc, op, wire=wire, residual=res)
        _assert_wire(R, got, want_w, 1, (wire, nsrc, op, n))
        assert E.same_residual(res, want_r), (wire, nsrc, op, n)
        assert (R.split(want_w, 1)[1] == 255).any()  # the NaN blocks are there


def test_owner_residual_numel():
    for wire in WIRES:
        for n, W in ((1, 1), (33, 3), (4113, 8), (1 << 22, 2)):
            assert ops.mx_owner_residual_numel(n, W, wire=wire) == 32 * ops.mx_chunk_blocks(n, W, wire=wire) \
                == E.owner_numel(n, W, wire)


# ------------------------------------------------------------------ the edge blocks
@pytest.mark.parametrize("dtn", list(E.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_edge_tensor_leaves_a_finite_residual(wire, dtn):
    R = E.WIRES[wire]
    xe, names = E.R4.edge_tensor()
    x = torch.from_numpy(xe).to(E.DTYPES[dtn])
    n = x.numel()
    special = ~np.isfinite(R.f32(x).reshape(-1, 32)).all(axis=1)
    assert special[names.index("one_nan")] and special[names.index("both_inf")]
    r0 = np.zeros(n, dtype=np.float32)
    # a finite block whose residual held NaN: reset there, and only there
    pre = next(i for i in range(len(names), n // 32 - 2) if not special[i:i + 3].any())
    r0[pre * 32:(pre + 1) * 32] = np.nan
    r0[(pre + 1) * 32:(pre + 3) * 32] = E.random_residual(64, 5, scale=1e-3)
    want_w, want_r = E.quantize(R.f32(x), r0, 1, wire)
    res = torch.from_numpy(r0.copy())
    got = ops.mx_quantize_reference(x, 1, wire=wire, residual=res)
    _assert_wire(R, got, want_w, 1, (wire, dtn))
    assert E.same_residual(res, want_r)
    r = res.numpy().reshape(-1, 32)
    assert np.isfinite(r).all()
    assert not r[special].any() and not np.signbit(r[special]).any()  # +0 on the NaN / inf blocks
    assert not r[pre].any()
    assert R.split(want_w, 1)[1][pre] == 255  # that block was sent as NaN
    assert r[pre + 1].any() and r[pre + 2].any()  # its neighbours carried on


# ------------------------------------------------------------------ bound and telescoping
def _reference_step(wire):
    state = {}

    def step(x, use_residual):
        n = x.size
        if use_residual:
            res = state.setdefault("r", torch.zeros(n))
            w = ops.mx_quantize_reference(torch.from_numpy(x), 1, wire=wire, residual=res)
            return ops.mx_dequantize_reference(w, n, wire=wire).numpy(), res.numpy().copy()
        w = ops.mx_quantize_reference(torch.from_numpy(x), 1, wire=wire)
        return ops.mx_dequantize_reference(w, n, wire=wire).numpy(), None

    return step


@pytest.mark.parametrize("kind", ["normal", "lognormal"])
@pytest.mark.parametrize("wire", WIRES)
def test_bound_and_telescoping(wire, kind):
    """(a) |r_t| stays within A_b / 15 (FP8) or A_b / 2 (FP4), times 1 + 2^-10, after every one of 64
    calls; (b) so does |sum sent - sum x|, element by element; (c) without feedback that sum leaves the
    bound (19-53x with these references), so (b) does not pass vacuously."""
    a, b, c = E.check_bound(E.bound_series(kind), _reference_step(wire), wire)
    print(f"{wire} {kind}: residual {a:.3f}, sum with feedback {b:.3f}, sum without {c:.1f} (of the bound)")
    assert a <= 1.0, a
    assert b <= 1.0, b
    assert c > 1.0, c


# ------------------------------------------------------------------ the collectives over shm
@pytest.mark.parametrize("world", [2, 3, 4])
def test_collectives_on_cpu_tensors(world):
    numels = (33, 513, 4113)
    dtypes = tuple(E.DTYPES) if world == 2 else ("float32", "bfloat16")
    res = launch(M.collective_cases, world, args=("cpu", numels, dtypes))
    for r, got in enumerate(res):
        assert len(got) == len(WIRES) * len(dtypes) * len(numels) * 3, sorted(got)
        bad = [k for k, v in got.items() if not v[0]]
        assert not bad, (r, bad)
        same = {k: v[1] for k, v in got.items() if not k.startswith("rs/")}  # identical bits on every rank
        assert same == {k: v[1] for k, v in res[0].items() if not k.startswith("rs/")}, r


def test_world_1_and_error_cases():
    got = launch(M.world1_and_errors, 1, args=("cpu",))[0]
    assert len(got) == 2 + 15 and all(got.values()), got
    for got in launch(M.world1_and_errors, 2, args=("cpu",)):
        assert len(got) == 15 and all(got.values()), got


def test_residual_errors_in_ops():
    x = torch.zeros(64)
    w = torch.zeros(17 * 16, dtype=torch.uint8)
    for wire in WIRES:
        for fn in (lambda r: ops.mx_quantize_reference(x, 1, wire=wire, residual=r),
                   lambda r: ops.mx_quantize_shards_reference(x, 2, wire=wire, residual=r)):
            with pytest.raises(TypeError, match="float32.*bfloat16"):
                fn(torch.zeros(64, dtype=torch.bfloat16))
            with pytest.raises(ValueError, match="63 elements, 64 expected"):
                fn(torch.zeros(63))
            with pytest.raises(ValueError, match="contiguous"):
                fn(torch.zeros(64, 2)[:, 0])
            with pytest.raises(ValueError, match="16-byte aligned"):
                fn(torch.zeros(65)[1:])
    with pytest.raises(TypeError, match="float32.*float64"):
        ops.mx_reduce_reference(w, 1, wire="mxfp4_e2m1", residual=torch.zeros(512, dtype=torch.float64))
    with pytest.raises(ValueError, match="64 elements, 512 expected"):
        ops.mx_reduce_reference(w, 1, wire="mxfp4_e2m1", residual=torch.zeros(64))
    # the GPU entry points check the residual before they look for the extension or a device
    for fn in (lambda r: ops.mx_quantize(x, 1, wire="mxfp4_e2m1", residual=r),
               lambda r: ops.mx_quantize_shards(x, 2, wire="mxfp4_e2m1", residual=r)):
        with pytest.raises(TypeError, match="float32.*float16"):
            fn(torch.zeros(64, dtype=torch.float16))
        with pytest.raises(ValueError, match="65 elements, 64 expected"):
            fn(torch.zeros(65))
    with pytest.raises(ValueError, match="64 elements, 512 expected"):
        ops.mx_reduce(w, 1, wire="mxfp4_e2m1", residual=torch.zeros(64))


def test_wrappers_refuse_error_feedback_without_a_wire():
    from pytorch_distributed_collective_communication_amd.parallel import ddp
    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    with pytest.raises(ValueError, match="error_feedback=True needs a compressed wire"):
        ddp.GradBucketer(torch.nn.Linear(2, 2), error_feedback=True)
    with pytest.raises(ValueError, match="grad_error_feedback=True needs a grad_wire"):
        ShardedOptimizer(torch.nn.Linear(2, 2).parameters(), grad_error_feedback=True, param_wire="mxfp8_e4m3")


# ------------------------------------------------------------------ the training wrappers on CPU tensors
@pytest.mark.parametrize("inf_step", [None, 1])
def test_grad_bucketer_with_error_feedback_on_cpu_tensors(inf_step):
    res = launch(M.bucketer, 2, args=("cpu", "mxfp4_e2m1", inf_step))
    _check_bucketer(res, inf_step)


def _check_bucketer(res, inf_step):
    for got in res:
        nb = got["buckets"]
        assert nb >= 2 and got["residuals"] == nb and got["no_sync"] and got["reset"], got
        for t, step in enumerate(got["steps"]):
            for i in range(nb):
                ok, dig, has_nan, finite = step[i]
                assert ok and finite, (t, i, step[i])
                assert dig == res[0]["steps"][t][i][1]  # the same bits on every rank
            # an overflowed gradient sends NaN in its block at that step and at no other
            assert any(step[i][2] for i in range(nb)) == (t == inf_step), (t, step)


def test_sharded_optimizer_with_error_feedback_on_cpu_tensors():
    _check_zero(launch(M.zero, 2, args=("cpu",)))


def _check_zero(res):
    for got in res:
        nb = got["buckets"]
        assert nb >= 2 and got["residual_numel"] == got["padded"], got
        for t, step in enumerate(got["steps"]):
            for i in range(nb):
                assert step[i][0] and step[i][1], (t, i, step[i])
            assert any(step[i][2] for i in range(nb)), t  # (the residuals are in use)
            assert step["digest"] == res[0]["steps"][t]["digest"]  # replicas agree
        assert got["sd_key"] == [["cpu", "torch.float32", got["padded"]]], got["sd_key"]
        assert got["restored"] == got["original"], got  # step 3 after a reload, bit for bit
        assert got["old_checkpoint_loads_zeros"], got
