"""The block-scaled FP8 wire format `mxfp8_e4m3` on the GPU: the three kernels, the collective,
the bucketer (docs/collectives.md "Compressed all-reduce").

The reference is always tests/_mx_ref.py (numpy integer arithmetic on the CPU), never a GPU cast:
wires must equal it byte for byte (the payload under a NaN block is unspecified), values exactly --
rtol = atol = 0, NaN where the reference has NaN.
"""
import functools

import numpy as np
import pytest
import torch

from tests import _mx_ref as R
from tests import _workers_mx as M
from tests.test_backend_gpu import _gpu_launch

pytestmark = pytest.mark.gpu

NUMELS = (1, 31, 32, 33, 511, 513, 4096 + 17, 65536 + 17)
WORLDS = (1, 3, 8)  # 3 and 8: whole padding chunks at the small sizes


def _ops():
    from pytorch_distributed_collective_communication_amd import ops

    return ops


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _inputs(dtn):
    """[(name, CPU tensor of dtype dtn)]: the edge blocks, then every ragged size."""
    dt = R.DTYPES[dtn]
    out = [("edge", torch.from_numpy(R.edge_tensor()[0]).to(dt))]
    out += [(f"n{n}", M.rank_inputs(n, 2, 300 + n, dt)[1]) for n in NUMELS]
    return out


@functools.lru_cache(maxsize=None)
def _ref_wire(dtn, name, world):
    x = dict(_inputs(dtn))[name]
    return R.quantize(R.f32(x), world)


def _wire_diff(got, ref, nchunks):
    gq, gs = R.split(got, nchunks)
    rq, rs = R.split(ref, nchunks)
    bad = np.nonzero((gs != rs) | ((gq != rq).any(axis=1) & (rs != 255)))[0]
    return [(int(b), int(gs[b]), int(rs[b]), gq[b].tolist(), rq[b].tolist()) for b in bad[:3]], len(bad)


# ------------------------------------------------------------------ the three kernels
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("dtn", list(R.DTYPES))
def test_quantize(dtn, world):
    ops = _ops()
    for name, x in _inputs(dtn):
        ref = _ref_wire(dtn, name, world)
        got = ops.mx_quantize(x.to(_dev()), world)
        assert got.dtype == torch.uint8 and got.numel() == ops.mx_wire_bytes(x.numel(), world) == ref.size
        got = got.cpu().numpy()
        if not R.same_wire(got, ref, world):
            first, count = _wire_diff(got, ref, world)
            pytest.fail(f"{dtn} {name} world={world}: {count} blocks differ; (block, s, want s, q, want q): {first}")


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("dtn", list(R.DTYPES))
def test_dequantize(dtn, world):
    # (dtn: the dtype the wire was quantized from; every output dtype is checked)
    ops = _ops()
    for name, x in _inputs(dtn):
        ref = _ref_wire(dtn, name, world)
        w = torch.from_numpy(ref).to(_dev())
        for odt in R.DTYPES.values():
            got = ops.mx_dequantize(w, x.numel(), odt, world)
            assert got.dtype == odt and got.numel() == x.numel()
            assert R.same(got, R.dequantize(ref, x.numel(), world, odt)), (dtn, name, world, odt)


@pytest.mark.parametrize("nsrc", [1, 2, 3, 5, 8])
def test_reduce_folds_in_source_order(nsrc):
    ops = _ops()
    for n in (48 * 32, 65536 + 17):  # one workgroup, and several with a ragged end
        xs = M.rank_inputs(n, nsrc, 40 + nsrc)
        edge = torch.from_numpy(R.edge_tensor()[0][:1024])
        xs[nsrc - 1][:1024] = edge  # NaN, inf, zero and clamped blocks on the last source
        wire = np.concatenate([R.quantize(R.f32(x), 1) for x in xs])
        g = torch.from_numpy(wire).to(_dev())
        for op in ("sum", "avg"):
            ref = R.reduce(wire, nsrc, op)
            got = ops.mx_reduce(g, nsrc, op).cpu().numpy()
            if not R.same_wire(got, ref, 1):
                first, count = _wire_diff(got, ref, 1)
                pytest.fail(f"nsrc={nsrc} n={n} {op}: {count} blocks differ; {first}")
        if nsrc >= 3:
            # the inputs tell orders apart: a reversed fold and (from 5 sources on; at 3 a pairwise
            # tree is the sequential fold) a tree fold give other wires
            ref = R.reduce(wire, nsrc, "sum")
            back = np.concatenate([R.quantize(R.f32(x), 1) for x in reversed(xs)])
            assert not R.same_wire(R.reduce(back, nsrc, "sum"), ref, 1)
        if nsrc >= 5:
            q, s = R.split(wire, nsrc)
            d = R.d_blocks(q, s).reshape(nsrc, -1, 32)
            level = [d[r] for r in range(nsrc)]
            while len(level) > 1:
                level = [R.fold_blocks(level[i:i + 2], "sum") for i in range(0, len(level), 2)]
            assert not R.same_wire(R.join(*R.q_blocks(level[0]), 1), ref, 1)


def test_guard_bands_stay_intact():
    # the wire and the dequantized tensor are slices of patterned arenas; aligned slices are written in
    # place, the others through a copy: either way not one byte outside them changes
    ops = _ops()
    dev = _dev()
    for n, world in ((33, 1), (513, 3), (4096 + 17, 1), (65536 + 17, 8)):
        x = M.rank_inputs(n, 2, 9 + n)[0]
        ref = R.quantize(R.f32(x), world)
        nb = ref.size
        for off in (256, 4099):
            arena = torch.full((nb + 8192,), 0xA5, dtype=torch.uint8, device=dev)
            w = ops.mx_quantize(x.to(dev), world, out=arena[off:off + nb])
            assert w.data_ptr() == arena.data_ptr() + off
            a = arena.cpu().numpy()
            assert (a[:off] == 0xA5).all() and (a[off + nb:] == 0xA5).all(), (n, world, off)
            assert np.array_equal(a[off:off + nb], ref), (n, world, off)
            # reduce (one source: requantize) into an arena slice
            if world == 1:
                arena2 = torch.full((nb + 8192,), 0x5A, dtype=torch.uint8, device=dev)
                ops.mx_reduce(arena[off:off + nb], 1, "sum", out=arena2[off:off + nb])
                a2 = arena2.cpu().numpy()
                assert (a2[:off] == 0x5A).all() and (a2[off + nb:] == 0x5A).all(), (n, off)
                assert R.same_wire(a2[off:off + nb], R.reduce(ref, 1, "sum"), 1)
        wire = torch.from_numpy(ref).to(dev)
        for dt in R.DTYPES.values():
            want = R.dequantize(ref, n, world, dt)
            for off in (64, 1027):  # elements: 16-byte aligned, and not
                pat = torch.full((n + 4096,), -7.5, dtype=dt)
                arena = pat.to(dev)
                ops.mx_dequantize(wire, n, dt, world, out=arena[off:off + n])
                a = arena.cpu()
                assert torch.equal(a[:off], pat[:off]) and torch.equal(a[off + n:], pat[off + n:]), (n, world, dt, off)
                assert R.same(a[off:off + n], want), (n, world, dt, off)


def test_source_at_a_4_byte_offset():
    # a view that is contiguous but not 16-byte aligned goes through a copy, for every dtype
    ops = _ops()
    dev = _dev()
    for dtn, dt in R.DTYPES.items():
        for n in (33, 4096 + 17):
            x = M.rank_inputs(n, 2, 21 + n, dt)[0]
            step = 4 // x.element_size()
            base = torch.zeros(n + 8, dtype=dt, device=dev)
            base[step:step + n] = x.to(dev)
            view = base[step:step + n]
            assert view.data_ptr() % 16 == 4
            got = ops.mx_quantize(view, 3).cpu().numpy()
            assert R.same_wire(got, R.quantize(R.f32(x), 3), 3), (dtn, n)
    # and a strided one
    x = M.rank_inputs(2 * 513, 2, 5)[0]
    got = ops.mx_quantize(x.to(dev)[::2], 1).cpu().numpy()
    assert R.same_wire(got, R.quantize(R.f32(x[::2]), 1), 1)


def test_wrong_arguments_raise():
    ops = _ops()
    dev = _dev()
    with pytest.raises(TypeError, match="float64"):
        ops.mx_quantize(torch.zeros(8, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="'max'"):
        ops.mx_reduce(torch.zeros(33 * 16, dtype=torch.uint8, device=dev), 1, "max")
    with pytest.raises(RuntimeError, match="chunk wires"):
        ops.mx_reduce(torch.zeros(33 * 16 + 1, dtype=torch.uint8, device=dev), 1)
    with pytest.raises(RuntimeError, match="bytes"):
        ops.mx_dequantize(torch.zeros(33 * 16, dtype=torch.uint8, device=dev), 513)


# ------------------------------------------------------------------ the collective, ranks sharing GPU 0
def _check(res, cases):
    for r, got in enumerate(res):
        assert len(got) == cases, sorted(got)
        bad = [k for k, v in got.items() if not v[0]]
        assert not bad, (r, bad)
        assert {k: v[1] for k, v in got.items()} == {k: v[1] for k, v in res[0].items()}, r  # the same bits


@pytest.mark.parametrize("algo", ["default", "ipc"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_all_reduce_compressed(world, algo):
    env = {} if algo == "default" else {"PDCC_ALGO": "ipc"}
    big = world << 20  # the chunk wire reaches 1 MiB: 32768 blocks per chunk
    numels = (1, 33, 512 * world + 1, big)
    res = _gpu_launch(M.all_reduce_cases, world, args=("cuda", numels, ("float32",), ("sum", "avg")), env=env,
                      timeout_s=120)
    _check(res, len(numels) * 2)
    if algo == "ipc":
        assert all(v[2].startswith("ipc") for v in res[0].values()), res[0]
    res = _gpu_launch(M.all_reduce_cases, world, args=("cuda", numels[:3], ("bfloat16", "float16"), ("sum", "avg")),
                      env=env, timeout_s=120)
    _check(res, 3 * 2 * 2)


def test_all_reduce_compressed_world_8():
    res = _gpu_launch(M.all_reduce_cases, 8, args=("cuda", (33,), ("float32",), ("sum",)), timeout_s=120)
    _check(res, 1)


def test_async_op_orders_the_current_stream():
    res = _gpu_launch(M.all_reduce_cases, 2, args=("cuda", (33, 65536 + 17), ("float32", "bfloat16"), ("sum", "avg"),
                                                   True), timeout_s=120)
    _check(res, 2 * 2 * 2)


def test_world_1_and_errors_on_the_gpu():
    got = _gpu_launch(M.world1_and_errors, 1)[0]
    assert len(got) == 3 + 6 and all(got.values()), got


def test_grad_bucketer_with_a_compressed_wire():
    res = _gpu_launch(M.bucketer, 2, timeout_s=120)
    for got in res:
        assert got["buckets"] >= 2 and got["handles"] == ["CompressedWork"], got
        for i in range(got["buckets"]):
            assert got[i][0], (i, got[i])
            assert got[i][1] == res[0][i][1]
