"""Exact bytes of the copy collectives (broadcast, all_gather, gather, scatter, all_to_all in every call form)
on every engine, the ranks sharing GPU 0: one launch per (mode, world), the environment forcing one protocol.

Every case (tests/_workers_copy.py `copies`) compares every output tensor byte for byte with the routing rule
of tests/_copy_ref.py, inside guard bands, and checks that inputs and non-outputs are untouched. The engine
label of every case is asserted, so a size cannot pass on another path, and so is the number of cases.
docs/collectives.md "Copy collectives: what a call guarantees" states the contract.
"""
import pytest

from tests import _workers_copy as C
from tests.test_backend_gpu import _gpu_launch

pytestmark = pytest.mark.gpu

_THRESHOLDS = {"PDCC_IPC_LL_MAX": "0", "PDCC_IPC_1SHOT_MAX": "8K"}  # C.ONESHOT
_STAGED = {"PDCC_ALGO": "ipc", "PDCC_IPC_ZC": "0", **_THRESHOLDS}
_ZC = {"PDCC_IPC_ZC_MIN": "16K", **_THRESHOLDS}  # C.ZC_MIN
_ENV = {
    # (the LL plan in two launches, each within 1.5x the LL launch of tests/test_exact_gpu.py: every size; the
    # dtype views, roots and misalignments)
    "ll": {"PDCC_ALGO": "ipc"},
    "ll_views": {"PDCC_ALGO": "ipc"},
    "staged": _STAGED,
    # the smallest staging cap: see C.STAGING_FLOOR for the line that sets the floor
    "staged_cut": {**_STAGED, "PDCC_IPC_MAX_STAGING": "1M"},
    "w8": _STAGED,
    "zc": {"PDCC_ALGO": "ipc", **_ZC},
    "dyn": {"PDCC_ALGO": "ipc_dyn", "PDCC_IPC_DYN_MIN_ROWS": "1", **_ZC},
    "sdma": {"PDCC_ALGO": "ipc_sdma", **_ZC},
    "host": {"PDCC_ALGO": "host"},
}
_WORLDS = {"ll": (2, 3, 4), "ll_views": (2, 3, 4), "staged": (2, 3, 4), "staged_cut": (2, 3), "zc": (2, 3),
           "dyn": (2, 3), "sdma": (2, 3), "host": (2, 3)}


def _staged_label(form, n, oneshot=C.ONESHOT):
    if form == "broadcast":
        return "ipc_1shot" if n <= oneshot else "ipc_2shot"
    return "ipc"


def want_label(mode, entry):
    """The engine label a case must record (None: recorded, not asserted).

    From tests/golden/engine_labels.json (its rows of the aligned calls of every form under ipc, ipc_staged,
    ipc_dyn, ipc_sdma and host: LL, 1-shot / staged copy, zero copy, and the separate-list scatter and
    all_to_all staying staged under zero copy): every label of an aligned uint8 case whose bytes per chunk are a
    multiple of 16. Recorded from a run of this file, after reading csrc/backend/gpu_ops.cpp: the labels of
    misaligned views and of chunk sizes that are no multiple of 16 bytes under zero copy. Outside LL the
    front-end copies a tensor that is not 16-byte aligned to an aligned temporary and copies outputs back
    (gpu_util.h `prep_in` / `prep_out`) on every engine -- staged, zero copy, sdma, host -- so the misaligned
    cases of those modes test that copy and copy-back, not the kernels or hipMemcpyAsync at odd addresses; only
    the LL kernels run in place there. A single input stays zero-copy on its temporary, while the chunks of one
    flat input (scatter from x.chunk(W), all_to_all_single) stop being one buffer and the call is staged, so
    zero copy reads those two forms in place only at chunk sizes that are multiples of 16 bytes."""
    form, dtn, n, root, smis, dmis = entry
    if form == "all_to_all_uneven":
        return None
    if mode == "host":
        return "host"
    if mode in ("ll", "ll_views"):
        return "ipc_ll" if n <= C.LL_CAP else _staged_label(form, n, 512 << 10)  # (the default 1-shot limit)
    if mode in ("staged", "staged_cut", "w8"):
        return _staged_label(form, n)
    gathers = C.FORMS[form] == "all_gather"
    if n < C.ZC_MIN:
        return "ipc_dyn" if mode == "dyn" and gathers else _staged_label(form, n)
    if form in ("scatter_list", "all_to_all_list"):
        return "ipc"
    if form in ("scatter_flat", "all_to_all_single") and (n % 16 or smis):
        return "ipc"
    if mode == "sdma":
        return "ipc_sdma_zc"
    if mode == "dyn" and gathers:
        return "ipc_dyn_zc"
    return "ipc_2shot_zc" if form == "broadcast" else "ipc_zc"


def _run(mode, world, count):
    plan = C.plan_for(mode, world)
    assert len(plan) == count, len(plan)
    res = _gpu_launch(C.copies, world, args=("cuda", plan), env={"PDCC_AUTOTUNE": "0", **_ENV[mode]}, timeout_s=120)
    assert len(res) == world
    for r, got in enumerate(res):
        bad = {k: v for k, v in got.items() if not v[0]}
        assert not bad, (r, bad)
        assert len(got) == count, (len(got), count, sorted(got))
        labels = {C.case_key(e): (got[C.case_key(e)][1], want_label(mode, e)) for e in plan}
        wrong = {k: v for k, v in labels.items() if v[1] is not None and v[0] != v[1]}
        assert not wrong, (r, wrong)
    return res


def _count(mode, world):
    # per size 10 forms; 3 dtype views x 10 forms; W - 1 other roots x 4 rooted forms; 6 misalignments x 10 forms
    sizes = {"ll": 12, "ll_views": 0, "staged": 10, "staged_cut": 10, "zc": 7, "dyn": 7, "sdma": 7, "host": 4}[mode]
    if world == 2 and mode in ("zc", "dyn", "sdma"):
        sizes -= 1  # 2 W x 4096 is the lowered zero-copy threshold itself there
    extra = {"staged_cut": 9, "dyn": 3}.get(mode, 0)  # the cut sizes of 9 forms; 37 tiles of the 3 all_gather forms
    views = 0 if mode == "ll" else 30 + 4 * (world - 1) + 60  # (the LL plan runs them in a launch of their own)
    return 10 * sizes + views + extra


@pytest.mark.parametrize("mode,world", [(m, w) for m in _WORLDS for w in _WORLDS[m]])
def test_copy_collectives_every_engine(mode, world):
    res = _run(mode, world, _count(mode, world))
    if mode == "ll":  # the largest LL payload is LL, one byte more is not
        for got in res:
            for form in C.FORMS:
                if form == "all_to_all_uneven":
                    continue
                assert got[f"{form}/uint8/{C.LL_CAP}/root{world - 1}/src+0/dst+0"][1] == "ipc_ll"
                assert not got[f"{form}/uint8/{C.LL_CAP + 1}/root{world - 1}/src+0/dst+0"][1].endswith("_ll")
    if mode == "staged_cut":
        # every form ran at a size past two pieces of the per_call_max it passes to ipc_chunked at the staging
        # floor (C.per_call_max names the lines; C.launches models the cut, the engine reports no launch count)
        for form in C.CUT_FORMS:
            n = C.cut_size(form, world)
            assert C.launches(n, form, world) >= 3, (form, n)
            assert all(f"{form}/uint8/{n}/root{world - 1}/src+0/dst+0" in got for got in res), (form, n)


def test_copy_collectives_world8():
    # the k_ipc_copy<8> instantiation with data that tells owners apart: rows, a partial last row, a ragged tile
    _run("w8", 8, 9)
