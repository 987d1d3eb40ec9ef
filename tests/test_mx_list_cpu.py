"""The tensor-list layout without a GPU (docs/collectives.md "Tensor-list layout"): the layout helper, the
plain-PyTorch references of ops.mx_quantize_list / mx_dequantize_list against the numpy references applied to the
padded concatenation (tests/_workers_mx_list.pad_cat), all_reduce_compressed of a list of CPU tensors, the argument
errors, and what the layout is for: a scale byte never serves two tensors."""
import pytest
import torch

from pytorch_distributed_collective_communication_amd import ops
from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _mx_rot_ref as R
from tests import _workers_mx_list as ML
from tests._workers_mx import rank_inputs

WIRES = tuple(R.WIRES)


def test_list_numel_is_whole_blocks_per_tensor():
    for numels in list(ML.LISTS.values()) + [(), (0,), (64, 1)]:
        assert ops.mx_list_numel(numels) == 32 * sum(-(-n // 32) for n in numels)


@pytest.mark.parametrize("dtn", list(R.DTYPES))
@pytest.mark.parametrize("wire", WIRES)
def test_references_of_the_list_calls(wire, dtn):
    dt = R.DTYPES[dtn]
    for name in ("ragged", "empty", "many"):
        xs = [rank_inputs(n, 2, 80 + i, dt)[0] for i, n in enumerate(ML.LISTS[name])]
        flat = ML.pad_cat(xs)
        real = ML.pad_cat([torch.ones_like(x) for x in xs])
        for world, rot in ((1, None), (3, 0xFACE0FF1234567)):
            kw = {} if rot is None else dict(rotation="hadamard", rotation_seed=rot)
            ref = ML.ref_quantize(R.f32(flat), world, wire, rot=rot)
            assert R.same_wire(ops.mx_quantize_list_reference(xs, world, wire=wire, **kw).numpy(), ref, world, wire)
            want = ML.ref_quantize(R.f32(flat), world, wire, sr=(3, 4), rot=rot)
            got = ops.mx_quantize_list_reference(xs, world, wire=wire, rounding="stochastic", seed=3, stream=4, **kw)
            assert R.same_wire(got.numpy(), want, world, wire)
            res = torch.full((flat.numel(),), 0.01)
            want, sim = ML.ref_quantize(R.f32(flat), world, wire, res=res.numpy().copy(), rot=rot)
            assert R.same_wire(ops.mx_quantize_list_reference(xs, world, wire=wire, residual=res, **kw).numpy(), want, world, wire)
            assert R.same_residual(res, sim * real.float().numpy())
            outs = [torch.full_like(x, -7.5) for x in xs]
            ops.mx_dequantize_list_reference(torch.from_numpy(ref), outs, world, wire=wire, **kw)
            d = R.dequantize(ref, flat.numel(), world, wire, rot, dt) if rot else R.WIRES[wire].dequantize(ref, flat.numel(), world, dt)
            assert R.same(ML.pad_cat(outs), d * real)


@pytest.mark.parametrize("world", [2, 3])
def test_all_reduce_compressed_of_a_cpu_list(world):
    res = launch(ML.collective, world, args=("cpu", False, ("ragged",)))
    for got in res:
        assert len(got) == len(WIRES) * 2 and all(v[0] for v in got.values()), got
        assert {k: v[1] for k, v in got.items()} == {k: v[1] for k, v in res[0].items()}


def test_a_scale_byte_never_serves_two_tensors():
    """A weight of 16 elements at 2^10 and a bias of 32 at 1 on the FP4 wire. Packed, the bias's first 16 elements
    share the weight's block and scale and flush to zero; in the list layout they start a block of their own."""
    big, small = torch.full((16,), 1024.0), torch.ones(32)
    kw = dict(wire="mxfp4_e2m1")
    packed = ops.mx_dequantize_reference(ops.mx_quantize_reference(torch.cat([big, small]), **kw), 48, **kw)
    assert not packed[16:32].any() and bool(packed[:16].all())
    outs = [torch.zeros(16), torch.zeros(32)]
    ops.mx_dequantize_list_reference(ops.mx_quantize_list_reference([big, small], **kw), outs, **kw)
    assert bool(outs[1][:16].all()) and torch.equal(outs[0], big)


def test_argument_errors():
    f, one = torch.ones(40), torch.ones(1)
    for fn in (ops.mx_quantize_list, ops.mx_quantize_list_reference):  # (raised before anything native is called)
        for kind, needle, args, kw in ((TypeError, "one dtype", [f, f.half()], {}), (TypeError, "list or tuple", f, {}),
                                       (ValueError, "contiguous", [f, torch.ones(8, 8).t()], {}),
                                       (ValueError, "empty list", [], {}), (ValueError, "unknown wire", [f], dict(wire="mxfp5")),
                                       # (the residual of (40, 1) has 2 + 1 blocks)
                                       (ValueError, "64 elements, 96 expected", [f, one], dict(residual=torch.zeros(64))),
                                       (ValueError, "alternatives", [f], dict(residual=torch.zeros(64), rounding="stochastic"))):
            with pytest.raises(kind, match=needle):
                fn(args, **kw)


def test_world_1_an_empty_list_and_the_bucketer_s_keyword():
    assert all(launch(_world1, 1)[0].values())


def _world1(rank, size):
    from pytorch_distributed_collective_communication_amd import distributed as pd
    from pytorch_distributed_collective_communication_amd.parallel import ddp

    xs = [torch.randn(33), torch.randn(5)]
    keep = [x.clone() for x in xs]
    out = {"world 1": pd.all_reduce_compressed(xs, wire="mxfp4_e2m1") is None and all(map(torch.equal, xs, keep)),
           "empty": pd.all_reduce_compressed([], async_op=True).is_completed()}
    for name, kind, call in (("dtype", TypeError, lambda: pd.all_reduce_compressed([xs[0], xs[1].half()])),
                             ("residual", ValueError, lambda: pd.all_reduce_compressed(xs, residual=torch.zeros(38))),
                             ("wire", ValueError, lambda: ddp.GradBucketer(torch.nn.Linear(2, 2), in_place=True))):
        try:
            call()
            out[name] = False
        except kind:
            out[name] = True
    b = ddp.GradBucketer(torch.nn.Linear(2, 2), wire="mxfp8_e4m3", in_place=True, error_feedback=True)
    out["no flat"] = b.buckets[0].flat is None and b.buckets[0].residual.numel() == ops.mx_list_numel([2, 4])
    return out
