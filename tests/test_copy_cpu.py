"""The exact-byte contract of the copy collectives, where no GPU is needed: the plan of tests/test_copy_gpu.py
over the shm transport (this proves the harness and the reference), the sensitivity of the comparison to what a
subtly wrong engine would deliver, and the condition on the inputs that gives it that sensitivity.
"""
import pytest
import torch

from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _copy_ref as R
from tests import _workers_copy as C

T = R.T
MODES = {"ll": (2, 3, 4), "ll_views": (2, 3, 4), "staged": (2, 3, 4), "staged_cut": (2, 3), "zc": (2, 3), "dyn": (2, 3), "sdma": (2, 3),
         "host": (2, 3), "w8": (8,)}


# ------------------------------------------------------------------------------------------ the reference
def test_routing_rules_by_hand():
    W = 3
    for coll in R.COLLS:
        ins = R.inputs(coll, 5, W, 1)
        assert len(ins) == W and all(len(x) == R.chunks_of(coll, W) for x in ins)
        again = R.inputs(coll, 5, W, 1)
        assert all(torch.equal(a, b) for x, y in zip(ins, again) for a, b in zip(x, y))
    b = R.inputs("broadcast", 5, W, 2)
    assert [R.expected("broadcast", b, r, 1)[0] is b[1][0] for r in range(W)] == [True] * W
    g = R.inputs("gather", 5, W, 3)
    assert R.expected("gather", g, 0, 2) == [] and R.expected("gather", g, 1, 2) == []
    assert all(a is c[0] for a, c in zip(R.expected("gather", g, 2, 2), g))
    assert all(a is c[0] for a, c in zip(R.expected("all_gather", g, 1, 0), g))
    s = R.inputs("scatter", 5, W, 4)
    assert [R.expected("scatter", s, r, 2)[0] is s[2][r] for r in range(W)] == [True] * W
    a = R.inputs("all_to_all", 5, W, 5)
    for r in range(W):
        assert all(x is a[q][r] for q, x in enumerate(R.expected("all_to_all", a, r, 0)))
    u = R.inputs("all_to_all_uneven", 5, W, 6)
    assert [[c.numel() for c in per_rank] for per_rank in u] == [[5, 10, 15]] * W
    assert [x.numel() for x in R.expected("all_to_all_uneven", u, 1, 0)] == [10, 10, 10]
    assert all(x is u[q][1] for q, x in enumerate(R.expected("all_to_all_uneven", u, 1, 0)))


def test_explain_names_the_tile_the_vector_and_the_source():
    ins = R.inputs("all_gather", 3 * T + 5, 2, 9)
    want = R.expected("all_gather", ins, 0, 0)
    got = [want[0], want[1].clone()]
    got[1][T:2 * T] = ins[0][0][2 * T:3 * T]  # tile 1 of output 1 taken from tile 2 of rank 0
    line = R.explain(got, want, ins, [(0, 0), (1, 0)])
    assert "output 1" in line and "first at +4096 (tile 1, vector 0, byte 0; source rank 1 chunk 0)" in line, line
    assert "rank 0 chunk 0 offset 8192 of the inputs (tile 2, vector 0)" in line, line
    assert R.explain(want, want, ins, [(0, 0), (1, 0)]) == ""


# ------------------------------------------------------------------------------------------ sensitivity
def _rejected(ins, coll, nbytes, world, rank, root):
    """{mutation: the comparison told the mutated outputs from the expected ones}."""
    want = R.flat(R.expected(coll, ins, rank, root))
    out = {}
    for name, mutate in R.MUTATIONS.items():
        m = mutate(coll, ins, rank, root, world)
        assert m is not None, (coll, name)  # the size below gives every mutation something to change
        out[name] = not R.identical(R.flat(m), want)
    return out


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("coll", R.COLLS)
def test_the_comparison_rejects_what_a_wrong_engine_delivers(coll, world):
    # rows, a partial last row and a ragged tile (the main size of the GPU plan); a non-root rank that receives
    nbytes = C.rows(world)[0]
    root = world - 1
    rank = root if coll == "gather" else 0
    got = _rejected(R.inputs(coll, nbytes, world, 77), coll, nbytes, world, rank, root)
    assert sorted(got) == sorted(R.MUTATIONS) and all(got.values()), got
    # ... and why these tests exist: with one constant per (rank, chunk), as the older tests fill their payloads,
    # the same comparison passes a kernel that permutes tiles, rotates the owners inside a chunk, shifts the data
    # by a vector or misplaces the seam between the zero-copy body and the rest
    const = _rejected(R.constant_inputs(coll, nbytes, world), coll, nbytes, world, rank, root)
    missed = sorted(k for k, v in const.items() if not v)
    assert missed == ["rotate_owner", "seam", "shift16", "swap_tiles"], const


# ------------------------------------------------------------------------------------------ the inputs
_CHECKED = set()


@pytest.mark.parametrize("mode,world", [(m, w) for m in MODES for w in MODES[m]])
def test_no_two_input_vectors_of_a_case_are_equal(mode, world):
    # a condition on the inputs, not a measurement: within one case every 16-byte vector of every rank's input is
    # distinct, so a vector delivered from any other place differs from the one expected (a seed that breaks
    # this is to be changed, not the check)
    plan = C.plan_for(mode, world)
    for entry in plan:
        if (world, entry) in _CHECKED:  # (the modes share most of their entries, and with them the inputs)
            continue
        _CHECKED.add((world, entry))
        nrows, distinct = R.distinct_vectors(C.case_inputs(entry, world))
        assert nrows == distinct, (C.case_key(entry), nrows, distinct)


def test_the_cut_sizes_take_three_launches():
    # under the per_call_max each form passes (C.per_call_max: the whole staging cap for broadcast, all_gather and
    # gather, a W-th of it for scatter and all_to_all), by the model of ipc_chunked that C.launches is
    for world in (2, 3):
        for form in C.CUT_FORMS:
            n = C.cut_size(form, world)
            assert C.launches(n, form, world) == 3 and C.launches(n - T - 5, form, world) == 2, (form, world, n)
            assert n < 3 << 20 and n % T == 5
            whole = C.FORMS[form] in ("broadcast", "all_gather", "gather")
            assert (n > 2 * C.STAGING_FLOOR - 2 * world * T) == whole, (form, world, n)
            assert any(e[0] == form and e[2] == n for e in C.plan_for("staged_cut", world))


# ------------------------------------------------------------------------------------------ the shm transport
def _plan(world):
    # every form, size, dtype view, root and misalignment of the staged GPU plan, and the LL plan's two largest
    return C.plan_for("staged", world) + tuple(e for e in C.plan_for("ll", world) if e[2] >= C.LL_CAP)


@pytest.mark.parametrize("world", [2, 3])
def test_cpu_tensors_through_the_shm_transport(world):
    plan = _plan(world)
    res = launch(C.copies, world, args=("cpu", plan))
    # 12 sizes x 10 forms, 3 dtype views x 10 forms, W - 1 other roots x 4 rooted forms, 6 misalignments x 10 forms
    assert len(plan) == 120 + 30 + 4 * (world - 1) + 60
    for r, got in enumerate(res):
        bad = {k: v for k, v in got.items() if not v[0]}
        assert not bad, (r, bad)
        assert len(got) == len(plan), sorted(got)
