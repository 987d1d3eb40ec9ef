"""Error feedback on the block-scaled wires on the GPU (docs/collectives.md "Error feedback"): the
fused residual kernels (dealt and shard layout, reduce), the collectives, the bucketer and the sharded
optimizer.

The reference is always tests/_mx_ef_ref.py (numpy on the CPU): wires must equal it byte for byte
(the payload under a NaN block is unspecified), results and residuals as values -- rtol = atol = 0,
+0 and -0 not told apart, and every residual finite.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _mx_ef_ref as E
from tests import _workers_mx_ef as M
from tests._workers_mx import rank_inputs
from tests.test_backend_gpu import _gpu_launch

pytestmark = pytest.mark.gpu

WIRES = tuple(E.WIRES)
NUMELS = (1, 31, 33, 513, 4113, 65553)
# 64 and 4096 start every shard 16-byte aligned in every dtype (the vector path); 1, 33 and 4113 in
# none (the element path)
SHARDS = (1, 33, 64, 4096, 4113)
WORLDS = (1, 3, 8)


def _ops():
    from pytorch_distributed_collective_communication_amd import ops

    return ops


def _dev():
    return torch.device("cuda", 0)


def _edge():
    return torch.from_numpy(E.R4.edge_tensor()[0])


@functools.lru_cache(maxsize=None)
def _dealt_cases(wire, dtn, world):
    """[(name, x, incoming residual, reference wire, reference residual)]"""
    R, dt = E.WIRES[wire], E.DTYPES[dtn]
    xs = [("edge", _edge().to(dt))] + [(f"n{n}", rank_inputs(n, 2, 600 + n, dt)[1]) for n in NUMELS]
    out = []
    for name, x in xs:
        r0 = E.random_residual(x.numel(), 910 + x.numel())
        out.append((name, x, r0) + E.quantize(R.f32(x), r0, world, wire))
    return out


@functools.lru_cache(maxsize=None)
def _shard_cases(wire, dtn, W):
    """[(name, x of W shards, m, incoming residual, reference wire, reference residual)]: every shard size,
    then the edge tensor as the last shard."""
    R, dt = E.WIRES[wire], E.DTYPES[dtn]
    xs = [(f"m{m}", rank_inputs(W * m, 2, 620 + m, dt)[0], m) for m in SHARDS]
    edge = _edge()
    m = edge.numel()
    x = rank_inputs(W * m, 2, 7)[0]
    x[(W - 1) * m:] = edge
    xs.append(("edge", x.to(dt), m))
    out = []
    for name, x, m in xs:
        r0 = E.random_residual(x.numel(), 930 + m)
        out.append((name, x, m, r0) + E.quantize_shards(R.f32(x), r0, W, wire))
    return out


def _assert_wire(R, got, ref, nchunks, what):
    got = got.cpu().numpy()
    if not R.same_wire(got, ref, nchunks):
        gq, gs = R.split(got, nchunks)
        rq, rs = R.split(ref, nchunks)
        bad = np.nonzero((gs != rs) | ((gq != rq).any(axis=1) & (rs != 255)))[0]
        pytest.fail(f"{what}: {len(bad)} blocks differ, first {bad[:3].tolist()}: scales {gs[bad[:3]].tolist()} "
                    f"want {rs[bad[:3]].tolist()}")


def _assert_residual(got, ref, what):
    g = got.cpu().numpy().reshape(-1)
    assert np.isfinite(g).all(), what
    bad = np.nonzero(g != ref)[0]
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), g[bad[:4]].tolist(), ref[bad[:4]].tolist())


# ------------------------------------------------------------------ quantize, dealt and shard layout
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("dtn", list(E.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_quantize(wire, dtn, world):
    ops, R = _ops(), E.WIRES[wire]
    for name, x, r0, want_w, want_r in _dealt_cases(wire, dtn, world):
        g = x.to(_dev())
        res = torch.from_numpy(r0).to(_dev())
        got = ops.mx_quantize(g, world, wire=wire, residual=res)
        what = f"{wire} {dtn} {name} world={world}"
        assert got.numel() == ops.mx_wire_bytes(x.numel(), world, wire=wire) == want_w.size
        _assert_wire(R, got, want_w, world, what)
        _assert_residual(res, want_r, what)
        assert torch.equal(g.cpu().view(torch.uint8), x.view(torch.uint8)), what  # x is not modified
        if name == "edge":  # +0 on the NaN / inf blocks
            with np.errstate(all="ignore"):
                special = ~np.isfinite(R.f32(x).reshape(-1, 32) + r0.reshape(-1, 32)).all(axis=1)
            r = res.cpu().numpy().reshape(-1, 32)
            assert special.sum() >= 2 and not r[special].any() and not np.signbit(r[special]).any(), what


@pytest.mark.parametrize("W", WORLDS)
@pytest.mark.parametrize("dtn", list(E.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_quantize_shards(wire, dtn, W):
    ops, R = _ops(), E.WIRES[wire]
    # the sizes cover both paths: 16-byte vectors exactly when m * element size is a multiple of 16
    vec = [m for m in SHARDS if m * E.DTYPES[dtn].itemsize % 16 == 0]
    assert vec and len(vec) < len(SHARDS) and 1 in SHARDS, vec
    for name, x, m, r0, want_w, want_r in _shard_cases(wire, dtn, W):
        g = x.to(_dev())
        res = torch.from_numpy(r0).to(_dev())
        got = ops.mx_quantize_shards(g, W, wire=wire, residual=res)
        what = f"{wire} {dtn} {name} W={W}"
        assert got.numel() == ops.mx_shard_wire_bytes(m, W, wire=wire) == want_w.size
        _assert_wire(R, got, want_w, W, what)
        _assert_residual(res, want_r, what)
        assert torch.equal(g.cpu().view(torch.uint8), x.view(torch.uint8)), what


# ------------------------------------------------------------------ reduce with the owner residual
@functools.lru_cache(maxsize=None)
def _sources(wire, nsrc, n):
    R = E.WIRES[wire]
    xs = rank_inputs(n, nsrc, 40 + nsrc)
    xs[nsrc - 1][:1024] = _edge()[:1024]  # NaN, inf and zero blocks on the last source
    return np.concatenate([R.quantize(R.f32(x), 1) for x in xs])


@pytest.mark.parametrize("nsrc", [1, 2, 3, 8])
@pytest.mark.parametrize("wire", WIRES)
def test_reduce(wire, nsrc):
    ops, R = _ops(), E.WIRES[wire]
    for n in (48 * 32, 65553):  # one workgroup, and several with a ragged end
        w = _sources(wire, nsrc, n)
        g = torch.from_numpy(w).to(_dev())
        r0 = E.random_residual(E.owner_numel(n, 1, wire), 88)
        assert r0.size == ops.mx_owner_residual_numel(n, 1, wire=wire)
        for op in ("sum", "avg"):
            want_w, want_r = E.reduce(w, nsrc, op, r0, wire)
            res = torch.from_numpy(r0).to(_dev())
            got = ops.mx_reduce(g, nsrc, op, wire=wire, residual=res)
            what = f"{wire} nsrc={nsrc} n={n} {op}"
            _assert_wire(R, got, want_w, 1, what)
            _assert_residual(res, want_r, what)
            assert (R.split(want_w, 1)[1] == 255).any()  # the NaN blocks are there
            assert torch.equal(g.cpu(), torch.from_numpy(w)), what


# ------------------------------------------------------------------ the residual is carried
@pytest.mark.parametrize("wire", WIRES)
def test_two_calls_carry_the_residual(wire):
    ops, R = _ops(), E.WIRES[wire]
    for dtn, dt in E.DTYPES.items():
        n = 4113
        x1, x2 = rank_inputs(n, 2, 71, dt)
        res = torch.zeros(n, device=_dev())
        r = np.zeros(n, dtype=np.float32)
        for x in (x1, x2):
            want_w, r = E.quantize(R.f32(x), r, 3, wire)
            got = ops.mx_quantize(x.to(_dev()), 3, wire=wire, residual=res)
            _assert_wire(R, got, want_w, 3, (wire, dtn))
            _assert_residual(res, r, (wire, dtn))
        assert r.any()
        # ... and the owner's
        w = _sources(wire, 3, 48 * 32)
        own = torch.zeros(E.owner_numel(48 * 32, 1, wire), device=_dev())
        r2 = np.zeros(own.numel(), dtype=np.float32)
        for op in ("avg", "sum"):
            want_w, r2 = E.reduce(w, 3, op, r2, wire)
            got = ops.mx_reduce(torch.from_numpy(w).to(_dev()), 3, op, wire=wire, residual=own)
            _assert_wire(R, got, want_w, 1, (wire, op))
            _assert_residual(own, r2, (wire, op))


# ------------------------------------------------------------------ guard bands
PAT = -7.5


def _arena(n, off):
    a = torch.full((n + 8192,), PAT, dtype=torch.float32, device=_dev())
    return a, a[off:off + n]


def _bands_intact(arena, off, n):
    a = arena.cpu()
    return bool((a[:off] == PAT).all() and (a[off + n:] == PAT).all())


@pytest.mark.parametrize("wire", WIRES)
def test_guard_bands_stay_intact(wire):
    # the residual is a slice of a patterned f32 arena at a 16-byte aligned offset, the wire a slice of a
    # patterned byte arena: not one element outside either changes
    ops, R = _ops(), E.WIRES[wire]
    for dtn, dt in E.DTYPES.items():
        for n, world in ((33, 3), (513, 1), (4113, 1), (65553, 8)):
            x = rank_inputs(n, 2, 9 + n, dt)[0]
            r0 = E.random_residual(n, n)
            want_w, want_r = E.quantize(R.f32(x), r0, world, wire)
            nb = want_w.size
            for off in (4, 1028):  # elements: 16 and 4112 bytes
                arena, res = _arena(n, off)
                res.copy_(torch.from_numpy(r0))
                warena = torch.full((nb + 8192,), 0xA5, dtype=torch.uint8, device=_dev())
                g = x.to(_dev())
                ops.mx_quantize(g, world, out=warena[256:256 + nb], wire=wire, residual=res)
                what = (wire, dtn, n, world, off)
                assert _bands_intact(arena, off, n), what
                _assert_residual(res, want_r, what)
                wa = warena.cpu().numpy()
                assert (wa[:256] == 0xA5).all() and (wa[256 + nb:] == 0xA5).all(), what
                assert R.same_wire(wa[256:256 + nb], want_w, world), what
                assert torch.equal(g.cpu().view(torch.uint8), x.view(torch.uint8)), what
        # shards: what lies past a ragged shard end belongs to the next shard (or to the band)
        for m, W in ((1, 3), (33, 3), (64, 8), (4113, 1), (4113, 3)):
            x = rank_inputs(W * m, 2, 19 + m, dt)[0]
            r0 = E.random_residual(W * m, m)
            want_w, want_r = E.quantize_shards(R.f32(x), r0, W, wire)
            arena, res = _arena(W * m, 1028)
            res.copy_(torch.from_numpy(r0))
            got = ops.mx_quantize_shards(x.to(_dev()), W, wire=wire, residual=res)
            assert _bands_intact(arena, 1028, W * m), (wire, dtn, m, W)
            _assert_residual(res, want_r, (wire, dtn, m, W))
            _assert_wire(R, got, want_w, W, (wire, dtn, m, W))
    # reduce: the owner residual in an arena
    n = 48 * 32
    w = _sources(wire, 2, n)
    r0 = E.random_residual(E.owner_numel(n, 1, wire), 3)
    want_w, want_r = E.reduce(w, 2, "sum", r0, wire)
    arena, res = _arena(r0.size, 1028)
    res.copy_(torch.from_numpy(r0))
    warena = torch.full((want_w.size + 8192,), 0x5A, dtype=torch.uint8, device=_dev())
    ops.mx_reduce(torch.from_numpy(w).to(_dev()), 2, "sum", out=warena[256:256 + want_w.size], wire=wire, residual=res)
    assert _bands_intact(arena, 1028, r0.size)
    _assert_residual(res, want_r, wire)
    wa = warena.cpu().numpy()
    assert (wa[:256] == 0x5A).all() and (wa[256 + want_w.size:] == 0x5A).all()
    assert R.same_wire(wa[256:256 + want_w.size], want_w, 1)


# ------------------------------------------------------------------ bound and telescoping, on the kernels
@pytest.mark.parametrize("kind", ["normal", "lognormal"])
@pytest.mark.parametrize("wire", WIRES)
def test_bound_and_telescoping(wire, kind):
    """(a) |r_t| stays within A_b / 15 (FP8) or A_b / 2 (FP4), times 1 + 2^-10, after every one of 64
    calls of the kernel; (b) so does |sum sent - sum x|, element by element; (c) without feedback that
    sum leaves the bound, so (b) does not pass vacuously."""
    ops = _ops()
    state = {}

    def step(x, use_residual):
        n = x.size
        g = torch.from_numpy(x).to(_dev())
        res = state.setdefault("r", torch.zeros(n, device=_dev())) if use_residual else None
        w = ops.mx_quantize(g, 1, wire=wire, residual=res)
        sent = ops.mx_dequantize(w, n, wire=wire).cpu().numpy()
        return sent, (res.cpu().numpy() if use_residual else None)

    a, b, c = E.check_bound(E.bound_series(kind), step, wire)
    print(f"{wire} {kind}: residual {a:.3f}, sum with feedback {b:.3f}, sum without {c:.1f} (of the bound)")
    assert a <= 1.0, a
    assert b <= 1.0, b
    assert c > 1.0, c


# ------------------------------------------------------------------ errors
def test_wrong_residuals_raise():
    ops, dev = _ops(), _dev()
    x = torch.zeros(64, device=dev)
    w = torch.zeros(17 * 16, dtype=torch.uint8, device=dev)
    W4 = "mxfp4_e2m1"
    for fn, n in ((lambda r: ops.mx_quantize(x, 1, wire=W4, residual=r), 64),
                  (lambda r: ops.mx_quantize_shards(x, 2, wire=W4, residual=r), 64),
                  (lambda r: ops.mx_reduce(w, 1, wire=W4, residual=r), 512)):
        with pytest.raises(TypeError, match="float32.*bfloat16"):
            fn(torch.zeros(n, dtype=torch.bfloat16, device=dev))
        with pytest.raises(ValueError, match=f"{n + 4} elements, {n} expected"):
            fn(torch.zeros(n + 4, device=dev))
        with pytest.raises(ValueError, match="contiguous"):
            fn(torch.zeros(n, 2, device=dev)[:, 0])
        with pytest.raises(ValueError, match="16-byte aligned"):
            fn(torch.zeros(n + 1, device=dev)[1:])
        with pytest.raises(ValueError, match="is on cpu"):
            fn(torch.zeros(n))
    assert not x.any() and not w.any()


def test_world_1_and_errors_on_the_gpu():
    got = _gpu_launch(M.world1_and_errors, 1)[0]
    assert len(got) == 2 + 15 and all(got.values()), got
    for got in _gpu_launch(M.world1_and_errors, 2):
        assert len(got) == 15 and all(got.values()), got


# ------------------------------------------------------------------ the collectives, ranks sharing GPU 0
@pytest.mark.parametrize("async_op", [False, True])
@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_collectives(world, async_op):
    # 33: whole padding chunks; 65553: several workgroups and a ragged end
    numels = (33, 65553)
    dtypes = ("float32", "bfloat16") if world <= 4 else ("float32",)
    res = _gpu_launch(M.collective_cases, world, args=("cuda", numels, dtypes, WIRES, async_op), timeout_s=180)
    for r, got in enumerate(res):
        assert len(got) == len(WIRES) * len(dtypes) * len(numels) * 3, sorted(got)
        bad = [k for k, v in got.items() if not v[0]]
        assert not bad, (r, bad)
        same = {k: v[1] for k, v in got.items() if not k.startswith("rs/")}  # the same bits on every rank
        assert same == {k: v[1] for k, v in res[0].items() if not k.startswith("rs/")}, r


# ------------------------------------------------------------------ the training wrappers
def test_grad_bucketer_with_error_feedback():
    from tests.test_mx_ef_cpu import _check_bucketer

    _check_bucketer(_gpu_launch(M.bucketer, 2, args=("cuda", "mxfp4_e2m1", None), timeout_s=120), None)


def test_a_non_finite_step_does_not_poison_the_next():
    # an inf in one gradient at the second step: NaN in that block at that step, finite results equal to
    # the reference at the third
    from tests.test_mx_ef_cpu import _check_bucketer

    _check_bucketer(_gpu_launch(M.bucketer, 2, args=("cuda", "mxfp4_e2m1", 1), timeout_s=120), 1)


def test_sharded_optimizer_with_error_feedback_and_its_state_dict():
    # grad_wire mxfp4_e2m1 with feedback, param_wire mxfp8_e4m3; a state_dict() taken after step 2 and
    # loaded into a fresh optimizer reproduces step 3 bit for bit, the residuals included
    from tests.test_mx_ef_cpu import _check_zero

    _check_zero(_gpu_launch(M.zero, 2, args=("cuda", "mxfp4_e2m1", "mxfp8_e4m3"), timeout_s=120))
