"""Rank function and plans of the exact-byte tests of the copy collectives (tests/test_copy_gpu.py,
tests/test_copy_cpu.py): broadcast, all_gather, gather, scatter and all_to_all in every call form.

Every rank regenerates all ranks' input bytes from seeds (tests/_copy_ref.py `inputs`), runs the collective
on its own, and compares every output tensor byte for byte with `expected`, the routing rule of the
collective. Every tensor handed to a call is a slice of a byte arena with GUARD bytes of a position-dependent
pattern on both sides, `mis` bytes into a 16-byte-aligned slot; outputs hold another such pattern before the
call. A case passes if the outputs are exact, every guard is intact and every input still holds its bytes.
"""
import torch

from tests import _copy_ref as R
from tests import _exact as E
from tests._workers_exact import GUARD, Guarded, _dev

T = R.T
# form -> the collective whose routing rule it follows
FORMS = {"broadcast": "broadcast",
         "all_gather_list": "all_gather",          # a list of separate tensors
         "all_gather_flat": "all_gather",          # a list that is out.chunk(W)
         "all_gather_into_tensor": "all_gather",
         "gather": "gather",
         "scatter_flat": "scatter",                # from x.chunk(W): read in place under zero copy
         "scatter_list": "scatter",                # from separate tensors
         "all_to_all_list": "all_to_all",
         "all_to_all_single": "all_to_all",
         "all_to_all_uneven": "all_to_all_uneven"}  # all_to_all_single, rank r sends q + 1 rows to rank q
ROOTED = ("broadcast", "gather", "scatter_flat", "scatter_list")
SPARE = 16  # room behind the payload slot for the misalignment


class Slot(Guarded):
    """A `Guarded` whose tensor starts `mis` bytes into the 16-byte-aligned payload slot: `payload` (CPU
    bytes) copied there, `.t` the view of dtype `dt` to hand to the collective. `.after()` reads the arena
    back once: (the payload bytes now, whether every byte outside them still holds the pattern)."""

    def __init__(self, payload, d, salt, mis=0, dt=torch.uint8):
        assert payload.dtype == torch.uint8 and payload.dim() == 1 and 0 <= mis < SPARE
        self.nbytes = payload.numel()
        self.lo = GUARD + mis
        self.fill = payload
        self.pat = E.pattern(2 * GUARD + SPARE + self.nbytes, salt)
        host = self.pat.clone()
        host[self.lo:self.lo + self.nbytes] = payload
        self.arena = host.to(d) if d.type != "cpu" else host
        assert self.arena.data_ptr() % 16 == 0
        self.t = self.arena[self.lo:self.lo + self.nbytes].view(dt)
        assert self.t.data_ptr() % 16 == mis

    def after(self):
        a = self.arena.cpu()
        end = self.lo + self.nbytes
        whole = bool(torch.equal(a[:self.lo], self.pat[:self.lo]) and torch.equal(a[end:], self.pat[end:]))
        return a[self.lo:end], whole

    def intact(self):
        return self.after()[1]


def _seed(form, dtn, nbytes, root, smis, dmis):
    return 17 + nbytes % 99991 + 100003 * (list(FORMS).index(form) + 16 * (root + 8 * (smis + 16 * dmis))) + len(dtn)


def case_inputs(entry, world):
    """Every rank's input chunks of one plan entry (the same on whichever rank, or test, builds them)."""
    form, dtn, nbytes, root, smis, dmis = entry
    seed = _seed(*entry)
    while True:
        ins = R.inputs(FORMS[form], nbytes, world, seed)
        if nbytes >= 16:
            return ins
        # chunks of a few random bytes may agree: a seed under which two do is replaced by the next, so that
        # no two input vectors of a case are equal (tests/test_copy_cpu.py checks that for every entry)
        nrows, distinct = R.distinct_vectors(ins)
        if nrows == distinct:
            return ins
        seed += 7919


def case_key(entry):
    form, dtn, nbytes, root, smis, dmis = entry
    return f"{form}/{dtn}/{nbytes}/root{root}/src+{smis}/dst+{dmis}"


def _sources(coll, rank, root, world):
    if coll == "broadcast":
        return [(root, 0)]
    if coll in ("all_gather", "gather"):
        return [(q, 0) for q in range(world)]
    if coll == "scatter":
        return [(root, rank)]
    return [(q, rank) for q in range(world)]


def _case(dist, entry, rank, size, d):
    """Runs one plan entry; returns (input slots, [(output slot, byte lengths of its output tensors)])."""
    form, dtn, n, root, smis, dmis = entry
    dt = E.DTYPES[dtn]
    coll = FORMS[form]
    ins = case_inputs(entry, size)
    salt = [1000 * (rank + 1)]

    def slot(payload, mis, dtype=dt):
        salt[0] += 1
        return Slot(payload, d, salt[0], mis, dtype)

    def blank(nbytes, mis, dtype=dt):  # an output: a pattern of its own, so an unwritten byte shows
        salt[0] += 1
        return Slot(E.pattern(nbytes, 7 * salt[0]), d, salt[0], mis, dtype)

    if form == "broadcast":  # the tensor is input on the root, output elsewhere (and compared on both)
        s = slot(ins[rank][0], smis if rank == root else dmis)
        dist.broadcast(s.t, src=root)
        return [], [(s, [n])]
    if coll in ("all_gather", "gather"):
        si = slot(ins[rank][0], smis)
        if form == "gather":
            so = [blank(n, dmis) for _ in range(size)] if rank == root else []
            dist.gather(si.t, gather_list=[o.t for o in so] if rank == root else None, dst=root)
            return [si], [(o, [n]) for o in so]
        if form == "all_gather_list":
            so = [blank(n, dmis) for _ in range(size)]
            dist.all_gather([o.t for o in so], si.t)
            return [si], [(o, [n]) for o in so]
        so = blank(size * n, dmis)
        if form == "all_gather_flat":
            dist.all_gather(list(so.t.chunk(size)), si.t)
        else:
            dist.all_gather_into_tensor(so.t, si.t)
        return [si], [(so, [n] * size)]
    if coll == "scatter":
        so = blank(n, dmis)
        si = []
        lst = None
        if rank == root and form == "scatter_flat":
            si = [slot(R.flat(ins[root]), smis)]
            lst = list(si[0].t.chunk(size))
        elif rank == root:
            si = [slot(c, smis) for c in ins[root]]
            lst = [s.t for s in si]
        dist.scatter(so.t, scatter_list=lst, src=root)
        return si, [(so, [n])]
    if form == "all_to_all_list":
        si = [slot(c, smis) for c in ins[rank]]
        so = [blank(n, dmis) for _ in range(size)]
        dist.all_to_all([o.t for o in so], [s.t for s in si])
        return si, [(o, [n]) for o in so]
    si = slot(R.flat(ins[rank]), smis)
    if form == "all_to_all_single":
        so = blank(size * n, dmis)
        dist.all_to_all_single(so.t, si.t)
        return [si], [(so, [n] * size)]
    assert form == "all_to_all_uneven"
    so = blank(size * (rank + 1) * n, dmis)
    cols = si.t.numel() // (size * (size + 1) // 2)  # elements per row of n bytes
    dist.all_to_all_single(so.t.view(-1, cols), si.t.view(-1, cols), output_split_sizes=[rank + 1] * size,
                           input_split_sizes=[q + 1 for q in range(size)])
    return [si], [(so, [(rank + 1) * n] * size)]


def _verdict(entry, rank, size, si, so, label):
    form, dtn, n, root, smis, dmis = entry
    coll = FORMS[form]
    ins = case_inputs(entry, size)
    want = R.expected(coll, ins, rank, root)
    got, whole, notes = [], True, []
    for s, lens in so:
        now, ok = s.after()
        whole = whole and ok
        at = 0
        for ln in lens:
            got.append(now[at:at + ln])
            at += ln
        assert at == s.nbytes
    exact = len(got) == len(want) and all(R.identical(g, w) for g, w in zip(got, want))
    if not exact:
        notes.append(R.explain(got, want, ins, _sources(coll, rank, root, size)))
    kept = True
    for k, s in enumerate(si):
        now, ok = s.after()
        whole = whole and ok
        if not R.identical(now, s.fill):
            kept = False
            notes.append(f"input {k} changed, first at +{int((now != s.fill).nonzero()[0])}")
    if not whole:
        notes.append("guard bytes changed")
    return [exact and kept and whole, label, "; ".join(notes)]


def copies(rank, size, device="cpu", plan=()):
    """`plan`: ((form, dtype name, bytes per chunk, root, src_misalign, dst_misalign), ...).
    Returns {case: [ok, engine label, detail]}."""
    import torch.distributed as dist

    d = _dev(device)
    # the ranks share this machine's cores (see _workers_exact.reductions)
    torch.set_num_threads(1 if d.type == "cpu" else 4)
    label = lambda: ""  # noqa: E731
    if d.type == "cuda":
        from pytorch_distributed_collective_communication_amd.parallel import backend as be

        label = be.native_backend(None, "cuda").last_algo
    out = {}
    for entry in plan:
        key = case_key(entry)
        assert key not in out, key
        si, so = _case(dist, entry, rank, size, d)
        lab = label()
        out[key] = _verdict(entry, rank, size, si, so, lab)
    dist.barrier()
    return out


# ------------------------------------------------------------------------------------------------ plans
SMALL = (1, 15, 17, T - 1, T, T + 1)
LL_CAP = 256 << 10   # kern::kLLMaxBytes, the default PDCC_IPC_LL_MAX
ZC_MIN = 16 << 10    # PDCC_IPC_ZC_MIN as the zc / dyn / sdma modes lower it
ONESHOT = 8 << 10    # PDCC_IPC_1SHOT_MAX as every mode but ll lowers it
# The staging cap. IpcComm's constructor (csrc/device/ipc_comm.cpp, `max_staging_(std::max<size_t>(max_staging,
# 1u << 20))`) raises any PDCC_IPC_MAX_STAGING below 1 MiB to 1 MiB; config.cpp takes the value as it is.
STAGING_FLOOR = 1 << 20
VIEW_DTYPES = ("bfloat16", "float32", "int64")
MISALIGN = tuple((s, d) for m in (4, 1) for s, d in ((m, 0), (0, m), (m, m)))
CUT_FORMS = tuple(f for f in FORMS if f != "all_to_all_uneven")  # (the IPC all_to_all takes equal splits only)


def rows(world):
    """Several rows with a partial last row and a ragged tile; whole rows; whole tiles with a partial last row;
    a rest shorter than one vector."""
    return ((2 * world + 1) * T + 5, 2 * world * T, 2 * world * T + T, 2 * world * T + 3)


def per_call_max(form, world, cap=STAGING_FLOOR):
    """The `per_call_max` a staged call of `form` hands to ipc_chunked when IpcComm::chunk_cap() is `cap`, read
    from csrc/backend/gpu_ops.cpp (the bytes it is compared with are the call's bytes per chunk):
      broadcast                      enqueue_broadcast, lines 498 / 500:  ic.chunk_cap()
      all_gather (3 forms), gather   enqueue_allgather, line 545:         ic.chunk_cap()
      scatter (2 forms)              enqueue_scatter, line 623:           ic.chunk_cap() / size_
      all_to_all (3 forms)           enqueue_alltoall, line 741:          ic.chunk_cap() / size_"""
    return cap // world if FORMS[form] in ("scatter", "all_to_all") else cap


def launches(nbytes, form, world):
    """A model of ProcessGroupMI355X::ipc_chunked (csrc/backend/gpu_ops.cpp lines 67-85), not a reading of the
    engine: the launches it issues for a staged call of `nbytes` per chunk at the staging floor -- per_call_max
    (above) rounded down to whole rows of W tiles, at least one row, and one launch per such piece. The tests
    use it to show that the cut sizes below are past two pieces under the cap each form really passes; that the
    pieces arrive where they belong is what the byte comparison of those cases shows."""
    row = world * T
    chunk = per_call_max(form, world) // row * row or row
    return -(-nbytes // chunk)


def cut_size(form, world):
    """Bytes per chunk that ipc_chunked cuts into 3 launches at the staging floor: two whole pieces (the
    form's per_call_max rounded down to rows of W tiles) and a third of one tile and a ragged 5 bytes."""
    row = world * T
    return 2 * (per_call_max(form, world) // row * row) + T + 5


def plan_for(mode, world):
    """The plan of one launch. Sizes are bytes per chunk; the root is the last rank except in the root sweep.
    The LL plan takes two launches: `ll` runs every size, `ll_views` the dtype views, the roots and the
    misalignments at the main size."""
    last = world - 1
    if mode == "w8":  # the W = 8 instantiation: the three multi-row sizes of three collectives
        return tuple((f, "uint8", n, last, 0, 0) for n in rows(world)[:3]
                     for f in ("broadcast", "all_gather_list", "all_to_all_single"))
    sizes = list(rows(world))
    if mode in ("ll", "staged", "staged_cut"):
        sizes = list(SMALL) + sizes
    if mode in ("zc", "dyn", "sdma"):
        sizes += [ZC_MIN - 1, ZC_MIN, ZC_MIN + T + 1]
    if mode == "ll":
        sizes += [LL_CAP, LL_CAP + 1]
    sizes = list(dict.fromkeys(sizes))
    main = rows(world)[0]
    by_size = [(f, "uint8", n, last, 0, 0) for n in sizes for f in FORMS]
    views = []
    for dtn in VIEW_DTYPES:  # the same bytes seen through wider elements
        es = torch.empty(0, dtype=E.DTYPES[dtn]).element_size()
        views += [(f, dtn, main // es * es, last, 0, 0) for f in FORMS]
    views += [(f, "uint8", main, root, 0, 0) for root in range(last) for f in ROOTED]
    views += [(f, "uint8", main, last, s, d) for s, d in MISALIGN for f in FORMS]
    plan = by_size if mode == "ll" else views if mode == "ll_views" else by_size + views
    if mode == "staged_cut":
        plan += [(f, "uint8", cut_size(f, world), last, 0, 0) for f in CUT_FORMS]
    if mode == "dyn":  # a few dozen tiles: several work items per call with PDCC_IPC_DYN_MIN_ROWS=1
        plan += [(f, "uint8", 37 * T + 5, last, 0, 0) for f in FORMS if FORMS[f] == "all_gather"]
    assert len({case_key(e) for e in plan}) == len(plan)
    return tuple(plan)
