"""The exact-value contract of the coalesced collectives, where no GPU is needed: the rank function of
tests/test_coalesced_gpu.py on CPU tensors over the shm transport at W = 1, 2, 3 (and the W = 8 plan), the calls
that must raise, the conditions on the inputs that make the comparison sensitive, and the comparison run on
doctored results. docs/collectives.md "Coalesced collectives: what a call guarantees" states the contract.
"""
import pytest
import torch

from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _exact as E
from tests import _workers_coalesced as C


def assert_launch(res, plan, world, extra):
    assert len(res) == world
    for r, got in enumerate(res):
        bad = {k: v for k, v in got.items() if not v[0]}
        assert not bad, (r, bad)
        assert len(got) == len(plan) + extra, (len(got), len(plan), extra)
        assert all(C.case_key(c) in got for c in plan)


# ------------------------------------------------------------------------------------------ the plans
def test_every_dtype_and_op_runs_on_the_ragged_list():
    assert sum(len(E.ops_for(dt)) for dt in E.DTYPES.values()) == 77 and len(E.DTYPES) == 12
    for mode, world in (("zc", 2), ("ll", 3), ("host", 2), ("cpu", 3)):
        plan = C.plan_for(mode, world)
        assert len(plan) == C.case_count(mode, world)
        for coll in ("all_reduce", "reduce_scatter"):
            ran = {(dtn, op) for c, lst, dtn, op, e, how in plan if c == coll and lst == "ragged" and how == "std"}
            assert ran == {(dtn, op) for dtn, dt in E.DTYPES.items() for op in E.ops_for(dt)}
        for coll in C.COLLS:  # every entry point, and every list, of every collective
            assert {e for c, lst, dtn, op, e, how in plan if c == coll} == set(C.ENTRIES)
            lists = {lst for c, lst, dtn, op, e, how in plan if c == coll}
            want = {"ragged", "empty", "all_empty", "exact16", "views", "one"}
            assert lists - {"mixed"} == want | {f"many{k}" for k in C.many_counts(coll, world)}, (coll, lists)
            assert ("mixed" in lists) == (coll == "all_gather")
    assert {c for c, *_ in C.plan_for("push", 2)} == {"all_reduce"}
    assert {c for c, *_ in C.plan_for("sdma", 2)} == {"all_gather"}


def test_the_lists_are_what_they_are_named_for():
    sizes = {lst: [n * C._esize(dt) for n, _, dt in C.members_of(lst, "uint8")] for lst in C.LISTS}
    assert sizes["ragged"] == [1, 15, 16, 17, 4095, 4096, 4097, 12292]
    assert {b % 16 == 0 for b in sizes["ragged"]} == {True, False}
    e = sizes["empty"]
    assert e[0] == 0 and e[-1] == 0 and 0 in e[1:-1] and any(e) and not any(sizes["all_empty"])
    assert len(sizes["one"]) == 1
    for dtn in E.DTYPES:  # whole 16-byte slots at every element width: the unpadded (at::empty) path
        assert all(n * C._esize(dt) % 16 == 0 for n, _, dt in C.members_of("exact16", dtn))
    assert [k for _, k, _ in C.members_of("views", "float32")] == ["off", "t", "2d", "flat"]
    widths = {C._esize(dt) for _, _, dt in C.members_of("mixed", "uint8")}
    dts = {dt for _, _, dt in C.members_of("mixed", "uint8")}
    assert widths == {1, 2, 4, 8} and {torch.bool, torch.float8_e4m3fn, torch.float8_e5m2} <= dts
    # the descriptor counts cross the K2 per-launch limit and twice that limit, at every world tested
    assert C.many_counts("all_reduce", 2) == C.many_counts("all_reduce", 8) == (63, 64, 65, 129)
    assert C.many_counts("all_gather", 2) == (31, 32, 33, 65)
    for world in (2, 3, 4, 8):
        descs = [k * world for k in C.many_counts("reduce_scatter", world)]
        assert min(descs) < 64 < descs[-2] < 128 < descs[-1], (world, descs)
    # every list but the empty one fills a buffer past the lowered zero-copy threshold and far below 1 MiB,
    # and equal lengths occur in the lists the swap test needs them in
    for lst in C.LISTS:
        if lst != "all_empty":
            assert C.ZC_MIN <= C.packed_bytes(lst, "uint8") <= 64 << 10, lst
    assert len(set(sizes["many65"])) < len(sizes["many65"])


@pytest.mark.parametrize("world", [2, 3])
def test_members_of_equal_length_never_share_an_expected_result(world):
    # a condition on the inputs, not a measurement: a seed that breaks it is to be changed, not the check
    for case in C.plan_for("cpu", world):
        coll, lst, dtn, op, entry, how = case
        if entry != C.ENTRIES[0] and case[:4] == C.plan_for("cpu", world)[0][:4]:
            continue
        want = C.expected(coll, lst, dtn, how, op, world, world - 1)
        seen = {}
        for i, w in enumerate(want):
            if w.numel() == 0:
                continue
            key = (w.dtype, tuple(w.shape), bytes(C._bytes(w).tolist()))
            assert key not in seen, (C.case_key(case), seen[key], i)
            seen[key] = i


@pytest.mark.parametrize("coll", C.COLLS)
def test_a_swap_of_ranks_changes_the_expected_result(coll):
    world = 3
    for lst in ("ragged", "many65" if coll == "all_reduce" else "many43", "views"):
        dtn, how = ("uint8", "std") if coll == "all_gather" else ("float32", "mixed")
        if lst == "views":
            dtn = "float32"
        want = C.expected(coll, lst, dtn, how, "SUM", world, 0)
        xs = C.inputs(coll, lst, dtn, how, world)
        for i, ((n, kind, dt), w) in enumerate(zip(C.members_of(lst, dtn), want)):
            flat = [x.reshape(-1) for x in xs[i]][::-1]  # the ranks in reversed order
            if coll == "all_reduce":
                other = E.fold(flat, "SUM", dt)
            elif coll == "all_gather":
                other = torch.cat(flat)
            else:
                other = E.fold([x[:n] for x in flat], "SUM", dt)
            if n * C._esize(dt) >= 256:  # (a few elements may round alike in either order)
                assert not torch.equal(C._bytes(other), C._bytes(w)), (coll, lst, i)


# ------------------------------------------------------------------------------------------ sensitivity
def _delivered(case, world, rank):
    """The arenas of `case` on CPU holding what an exact engine delivers."""
    coll, lst, dtn, op, entry, how = case
    ain, aout = C.build(case, rank, world, torch.device("cpu"))
    for v, w in zip((aout or ain).ts, C.expected(coll, lst, dtn, how, op, world, rank)):
        v.copy_(w.reshape(v.shape))
    return ain, aout


_SENSITIVITY = {"all_reduce": ("all_reduce", "many65", "float32", "SUM", "api", "mixed"),
                "all_gather": ("all_gather", "many43", "uint8", "SUM", "api", "std"),
                "reduce_scatter": ("reduce_scatter", "many43", "float32", "SUM", "api", "mixed")}


@pytest.mark.parametrize("coll", C.COLLS)
def test_the_comparison_rejects_what_a_wrong_pack_or_unpack_delivers(coll):
    case, world, rank = _SENSITIVITY[coll], 3, 1
    _, lst, dtn, op, entry, how = case
    ms = C.members_of(lst, dtn)

    def ok(doctor):
        ain, aout = _delivered(case, world, rank)
        doctor(aout or ain)
        return C.verdict(case, rank, world, ain, aout, "", [])

    assert ok(lambda a: None)[0]  # what an exact engine delivers passes
    equal = [i for i, m in enumerate(ms) if m == ms[2] and i != 2]
    assert equal, "the list needs two members of equal length"

    def swap(a):
        tmp = a.ts[2].clone()
        a.ts[2].copy_(a.ts[equal[0]])
        a.ts[equal[0]].copy_(tmp)

    def shift(a):  # one member delivered one element late
        a.ts[0].copy_(torch.roll(a.ts[0].clone(), 1))

    def reversed_ranks(a):
        xs = C.inputs(coll, lst, dtn, how, world)
        for v, x, (n, kind, dt) in zip(a.ts, xs, ms):
            flat = [t.reshape(-1) for t in x][::-1]
            if coll == "all_reduce":
                v.copy_(E.fold(flat, op, dt).reshape(v.shape))
            elif coll == "all_gather":
                v.copy_(torch.cat(flat))
            else:
                v.copy_(E.fold([t[rank * n:(rank + 1) * n] for t in flat], op, dt))

    def one_byte_past(a):  # the first byte after a member of four bytes
        lo, dt, shape, kind = a.specs[1]
        end = lo + C._esize(dt) * (shape[0] if len(shape) == 1 else shape[0] * shape[1])
        assert a.guard[end] and not a.guard[end - 1]
        a.arena[end] ^= 0xFF

    def guard_byte(a):
        a.arena[a.arena.numel() - 1] ^= 1

    for doctor in (swap, shift, reversed_ranks):
        v = ok(doctor)
        assert not v[0] and "member" in v[2] and "guard" not in v[2], (doctor.__name__, v)
    for doctor in (one_byte_past, guard_byte):
        v = ok(doctor)
        assert not v[0] and v[2] == "guard bytes changed", (doctor.__name__, v)
    if coll != "all_reduce":  # an input of the gather or the reduce-scatter that changed
        ain, aout = _delivered(case, world, rank)
        ain.arena[ain.specs[0][0]] ^= 1
        v = C.verdict(case, rank, world, ain, aout, "", [])
        assert not v[0] and v[2] == "input 0 changed", v


# ------------------------------------------------------------------------------------------ the shm transport
@pytest.mark.parametrize("world", [1, 2, 3])
def test_cpu_tensors_through_the_shm_transport(world):
    mode = "w1" if world == 1 else "cpu"
    plan = C.plan_for(mode, world)
    assert len(plan) == C.case_count(mode, world) == {1: 33, 2: 217, 3: 214}[world]
    res = launch(C.coalesced, world, args=("cpu", plan, C.b2b_for(mode, world)))
    assert_launch(res, plan, world, 1 + 2 * C.ERRORS["cpu"])
    if world == 1:
        # a world of one returns its inputs, whatever the op. The packed gather and reduce-scatter say so ("local",
        # coalesced.cpp); every plain collective of CPU tensors records "shm" at every world size (tests/test_units.py
        # pins "allreduce/shm" at W = 1), and with it the one-member shortcut and the all-reduce, which hands its
        # packed buffer to the plain all_reduce
        for got in res:
            for c in plan:
                want = "local" if c[0] != "all_reduce" and c[1] != "one" else "shm"
                assert got[C.case_key(c)][1] == want, (C.case_key(c), got[C.case_key(c)])


def test_the_world8_plan_on_the_shm_transport():
    # the W = 8 GPU launch, here first: 8 descriptors per member, the many lists around 64 and 128 of them
    plan = C.plan_for("w8", 8)
    assert len(plan) == C.case_count("w8", 8) == 4 * 2 + 3 + 4 + 3 + 4 * 2 + 3
    res = launch(C.coalesced, 8, args=("cpu", plan, (), False))
    assert_launch(res, plan, 8, 0)
