"""Exact values of the coalesced collectives (allreduce_coalesced, allgather_into_tensor_coalesced,
reduce_scatter_tensor_coalesced: csrc/backend/coalesced.cpp) on every engine, the ranks sharing GPU 0: one launch
per (mode, world), the environment forcing one protocol.

Every case (tests/_workers_coalesced.py `coalesced`) compares every member with a reference that knows nothing
about packing, exactly, inside guard bands, and checks that the call recorded one collective, that inputs are
untouched and that an async call hands back one Work. The engine label of every case is asserted against
`C.engine_label` (written from csrc/backend/gpu_ops.cpp and tests/golden/engine_labels.json), so a list cannot
pass on another protocol, and so is the number of cases. docs/collectives.md "Coalesced collectives: what a
call guarantees" states the contract.
"""
import pytest

from tests import _workers_coalesced as C
from tests.test_backend_gpu import _NUMERICS_ENV, _gpu_launch
from tests.test_copy_gpu import _ENV as _COPY_ENV

pytestmark = pytest.mark.gpu

# the thresholds of tests/test_copy_gpu.py: the packed buffers of these lists (16 to 64 KiB) reach every bulk protocol
_BULK = {"PDCC_IPC_LL_MAX": "0", "PDCC_IPC_1SHOT_MAX": "8K"}  # C.ONESHOT
_ZC = {**_BULK, "PDCC_IPC_ZC_MIN": "16K"}                      # C.ZC_MIN
_ENV = {
    "ll": _NUMERICS_ENV["ll"][0],
    "oneshot": _NUMERICS_ENV["oneshot"][0],  # (the default 1-shot limit: every list is 1-shot)
    "twoshot": {**_NUMERICS_ENV["twoshot"][0], **_BULK},
    "zc": {**_NUMERICS_ENV["zc"][0], **_ZC},
    "dyn": {**_NUMERICS_ENV["dyn"][0], "PDCC_IPC_DYN_MIN_ROWS": "1", **_ZC},
    "push": {**_NUMERICS_ENV["push"][0], **_ZC},
    "staged_algo": {**_NUMERICS_ENV["staged_algo"][0], **_ZC},
    "sdma": _COPY_ENV["sdma"],
    "host": _COPY_ENV["host"],
    "w8": {**_NUMERICS_ENV["twoshot"][0], **_BULK},
    "w1": {},
}
_WORLDS = {"ll": (2, 3, 4), "oneshot": (2, 3, 4), "twoshot": (2, 3, 4), "zc": (2, 3), "dyn": (2, 3), "push": (2, 3),
           "staged_algo": (2, 3), "sdma": (2, 3), "host": (2, 3)}


def _run(mode, world, with_errors=True):
    plan = C.plan_for(mode, world)
    b2b = C.b2b_for(mode, world)
    assert len(plan) == C.case_count(mode, world), len(plan)
    res = _gpu_launch(C.coalesced, world, args=("cuda", plan, b2b, with_errors),
                      env={"PDCC_AUTOTUNE": "0", **_ENV[mode]}, timeout_s=120)
    assert len(res) == world
    want = {C.case_key(c): C.engine_label(mode, c, world) for c in plan}
    want["back_to_back"] = C.engine_label(mode, b2b[-1], world)
    nerr = C.ERRORS["cuda"] if with_errors else 0
    for r, got in enumerate(res):
        bad = {k: v for k, v in got.items() if not v[0]}
        assert not bad, (r, bad)
        assert len(got) == len(plan) + 1 + 2 * nerr, (len(got), len(plan), sorted(got))
        wrong = {k: (got[k][1], w) for k, w in want.items() if got[k][1] != w}
        assert not wrong, (r, wrong)
        after = {v[1] for k, v in got.items() if k.startswith("after/")}
        assert after <= {C.engine_label(mode, C.AFTER_ERROR, world)}, after
    return res


@pytest.mark.parametrize("mode,world", [(m, w) for m in _WORLDS for w in _WORLDS[m]])
def test_coalesced_collectives_every_engine(mode, world):
    res = _run(mode, world)
    labels = {v[1] for got in res for v in got.values()}
    # the mode's own protocol ran (the expected labels above are per case; this guards the table itself)
    own = {"ll": "ipc_ll", "oneshot": "ipc_1shot", "twoshot": "ipc_2shot", "zc": "ipc_2shot_zc", "dyn": "ipc_2shot_dyn_zc",
           "push": "ipc_push_zc", "staged_algo": "ipc_2shot", "sdma": "ipc_sdma_zc", "host": "host"}[mode]
    assert own in labels, labels
    if mode in ("zc", "dyn"):
        assert {"ipc_dyn_zc" if mode == "dyn" else "ipc_zc"} <= labels, labels
    if mode != "host" and "all_reduce" in C.MODES[mode]:  # int16 has no kernel: the label says the host engine ran
        for got in res:
            assert {v[1] for k, v in got.items() if k.startswith("all_reduce/ragged/int16/")} == {"host"}


def test_coalesced_collectives_world8():
    # the W = 8 kernels, staged: 8 descriptors per member of the gather's unpack and the reduce-scatter's pack
    _run("w8", 8, with_errors=False)


def test_coalesced_collectives_world1():
    # a world of one returns the inputs bit for bit, guards intact, and records "local"
    res = _run("w1", 1)
    assert {v[1] for k, v in res[0].items() if not k.startswith(("error/", "back_to_back"))} == {"local"}
