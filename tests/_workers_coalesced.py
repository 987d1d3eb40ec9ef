"""Member lists, rank function and plans of the exact-value tests of the coalesced collectives
(tests/test_coalesced_gpu.py, tests/test_coalesced_cpu.py): allreduce_coalesced, allgather_into_tensor_coalesced
and reduce_scatter_tensor_coalesced of csrc/backend/coalesced.cpp, through torch's `_coalescing_manager`,
`dist.all_reduce_coalesced` and the two direct functions of `distributed.py`, sync and async.

The reference knows nothing about packing. Every rank regenerates all ranks' CPU members from seeds (they depend
on the member index, the rank and the position), runs the call on its own, and compares member by member:
all-reduce member i with `E.fold` over the ranks' members i, gather output i with the ranks' inputs i concatenated
(as bytes), reduce-scatter output i with `E.fold` over the ranks of chunk `rank` of their inputs i. `E.same`, no
tolerance. Every tensor handed to a call is a view into an `Arena`, a `Guarded` that holds a whole member list:
GUARD bytes of a position-dependent pattern at both ends and at least GAP such bytes between two members, so an
unpack that writes a whole vector where a member has four bytes changes a guard byte. A case passes if its
results are exact, every guard byte is intact, the inputs of a gather or reduce-scatter still hold their bytes,
the backend recorded exactly one collective for the call, and an async call handed back one Work that carries
the members.
"""
import functools
import zlib

import torch

from tests import _exact as E
from tests._workers_exact import GUARD, Guarded, _dev

GAP = 48                 # pattern bytes between two members of an arena, at least (three vectors)
COLLS = ("all_reduce", "all_gather", "reduce_scatter")
ENTRIES = ("mgr", "mgr_async", "api", "api_async")  # _coalescing_manager; all_reduce_coalesced / distributed.py
T = 4096                 # kern::kTileBytes
LL_CAP = 256 << 10       # kern::kLLMaxBytes, the default PDCC_IPC_LL_MAX
ONESHOT_DEFAULT = 512 << 10  # the default PDCC_IPC_1SHOT_MAX (config.h)
ONESHOT = 8 << 10        # PDCC_IPC_1SHOT_MAX as the bulk modes lower it
ZC_MIN = 16 << 10        # PDCC_IPC_ZC_MIN as the zero-copy modes lower it
K2_LAUNCH = 64           # descriptors per K2 launch (tests/test_exact_gpu.py test_k2_multi_copy_...)


def _many(count):
    """`count` members: one of 16 KiB + 4 B, so that the packed buffer reaches the bulk protocols whatever the
    count, then small ones of eight lengths, padded and unpadded slots mixed."""
    small = (4, 1000, 36, 520, 16, 500, 8, 260)
    return ((16 << 10) + 4,) + tuple(small[i % len(small)] for i in range(count - 1))


def many_counts(coll, world):
    """Member counts around the K2 per-launch limit. The all-reduce packs and unpacks one descriptor per member;
    the gather's unpack and the reduce-scatter's pack take `world` per member."""
    per = 1 if coll == "all_reduce" else world
    return tuple(sorted({(K2_LAUNCH - 1) // per, K2_LAUNCH // per, K2_LAUNCH // per + 1, 2 * K2_LAUNCH // per + 1}))


# name -> members: a length in BYTES (elements: bytes // element size, at least one; 0 stays empty), or
# (bytes, kind) with kind "off" (the base one element off 16-byte alignment), "t" (a non-contiguous .t() view)
# or "2d" (a contiguous 2-D tensor), or (bytes, kind, dtype name) in the gather's mixed-dtype list
LISTS = {
    "ragged": (1, 15, 16, 17, 4095, 4096, 4097, 12288 + 4),
    "empty": (0, 4097, 16, 0, 12288 + 4, 17, 0),
    "all_empty": (0, 0, 0),
    "exact16": (16, 4096, 32, 12288, 4080, 64),
    "views": ((4099, "off"), (6 * 1024 + 24, "t"), (8192, "2d"), 4100),
    "one": (5 * 4096 + 4,),
    "mixed": ((17, "flat", "uint8"), (4097, "flat", "bool"), (33, "flat", "float8_e4m3fn"),
              (4095, "flat", "float8_e5m2"), (4098, "flat", "bfloat16"), (12292, "flat", "float32"),
              (4104, "off", "int64"), (2, "flat", "int16")),
}
MANY = sorted({k for c in COLLS for w in (2, 3, 4, 8) for k in many_counts(c, w)})
LISTS.update({f"many{k}": _many(k) for k in MANY})


def _esize(dt):
    return torch.empty(0, dtype=dt).element_size()


def members_of(lst, dtn):
    """[(elements, kind, dtype)] of list `lst` at dtype `dtn`."""
    out = []
    for m in LISTS[lst]:
        nbytes, kind, mdt = (m, "flat", None) if isinstance(m, int) else (tuple(m) + (None,))[:3]
        dt = E.DTYPES[mdt or dtn]
        n = 0 if nbytes == 0 else max(1, nbytes // _esize(dt))
        if kind == "t":
            n = max(3, n // 3 * 3)
        if kind == "2d":
            n = max(2, n // 2 * 2)
        out.append((n, kind, dt))
    return out


def _shape(n, kind):
    return (n // 3, 3) if kind == "t" else (2, n // 2) if kind == "2d" else (n,)


def packed_bytes(lst, dtn):
    """The bytes the engine keys on: a single member as it is (the shortcut to the plain collective), else the
    members in 16-byte slots (pack_layout of csrc/backend/coalesced.cpp). Used for the expected engine label
    only; the expected values never see it."""
    nb = [n * _esize(dt) for n, _, dt in members_of(lst, dtn)]
    return nb[0] if len(nb) == 1 else sum((b + 15) // 16 * 16 for b in nb)


# ------------------------------------------------------------------------------------------------ arenas
class Arena(Guarded):
    """A `Guarded` of several members: `members` is [(CPU tensor as the collective is to see it, kind)], `.ts`
    the views to hand to the call. `.read()` copies the arena back once: (the members now, as CPU views of that
    copy; whether every byte outside the members still holds the pattern)."""

    def __init__(self, members, d, salt=0):
        at = GUARD
        self.specs = []
        for x, kind in members:
            at = (at + 15) // 16 * 16 + (x.element_size() if kind == "off" else 0)
            self.specs.append((at, x.dtype, tuple(x.shape), kind))
            at += x.numel() * x.element_size() + GAP
        total = (at + 15) // 16 * 16 + GUARD
        self.nbytes = total - 2 * GUARD
        self.pat = E.pattern(total, salt)
        self.guard = torch.ones(total, dtype=torch.bool)
        host = self.pat.clone()
        for (lo, dt, shape, kind), (x, _) in zip(self.specs, members):
            mem = x.t() if kind == "t" else x  # the bytes in memory order
            raw = mem.contiguous().reshape(-1).view(torch.uint8)
            host[lo:lo + raw.numel()] = raw
            self.guard[lo:lo + raw.numel()] = False
        self.arena = host.to(d) if d.type != "cpu" else host
        assert self.arena.data_ptr() % 16 == 0
        self.ts = self.views(self.arena)
        for t, (lo, dt, shape, kind) in zip(self.ts, self.specs):
            assert t.is_contiguous() == (kind != "t"), (shape, kind)
            assert t.numel() == 0 or (t.data_ptr() % 16 == 0) == (kind != "off"), (shape, kind)
        self.t = self.ts[0]

    def views(self, buf):
        out = []
        for lo, dt, shape, kind in self.specs:
            n = 1
            for s in shape:
                n *= s
            raw = buf[lo:lo + n * _esize(dt)].view(dt)
            out.append(raw.view(shape[1], shape[0]).t() if kind == "t" else raw.view(shape))
        return out

    def read(self):
        a = self.arena.cpu()
        return self.views(a), bool(torch.equal(a[self.guard], self.pat[self.guard]))

    def intact(self):
        return self.read()[1]


# ------------------------------------------------------------------------------------------------ inputs
def _seed(coll, lst, dtn):
    return 7 + zlib.crc32(f"{coll}/{lst}/{dtn}".encode()) % 50021


def _generate(coll, dt, n, world, seed, how):
    """Every rank's flat member of n elements."""
    if n == 0:
        return [torch.empty(0, dtype=dt) for _ in range(world)]
    if coll == "all_gather":  # bytes only: every bit pattern, NaN encodings included
        return [E.random_bits(n, dt, seed + 31 * r) for r in range(world)]
    if how == "mixed":  # a fold in another rank order differs
        return E.mixed_magnitudes(n, dt, world, seed)
    if dt.is_floating_point and n < 8:
        # (collective_inputs puts a NaN at the head of rank 0: two members of a few elements would both be NaN)
        return [E.random_values(n, dt, seed + 31 * r) for r in range(world)]
    return E.collective_inputs(n, dt, seed, world)


@functools.lru_cache(maxsize=64)
def inputs(coll, lst, dtn, how, world):
    """[member][rank] -> the CPU tensor rank `rank` hands in as member i, shaped as the call is to see it (a
    reduce-scatter input holds `world` chunks). The same on whichever rank, or test, builds them."""
    out = []
    for i, (n, kind, dt) in enumerate(members_of(lst, dtn)):
        full = n * world if coll == "reduce_scatter" else n
        flat = _generate(coll, dt, full, world, _seed(coll, lst, dtn) + 1009 * (i + 1), how)
        out.append([x.reshape(_shape(full, kind)) for x in flat])
    return out


@functools.lru_cache(maxsize=256)
def expected(coll, lst, dtn, how, op, world, rank):
    """The members after the call, by the rule of the collective alone."""
    want = []
    for (n, kind, dt), xs in zip(members_of(lst, dtn), inputs(coll, lst, dtn, how, world)):
        flat = [x.reshape(-1) for x in xs]
        if coll == "all_reduce":
            want.append(E.fold(flat, op, dt).reshape(_shape(n, kind)))
        elif coll == "all_gather":
            want.append(torch.cat(flat))
        else:
            want.append(E.fold([x[rank * n:(rank + 1) * n] for x in flat], op, dt).reshape(_out_shape(n, kind)))
    return want


def _out_shape(n, kind):
    return _shape(n, "flat" if kind == "t" else kind)  # outputs are contiguous


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def compare(coll, got, want, srcs=None):
    """Notes on every member that differs (none: exact). The gather compares bytes, the reductions values with
    `E.same` (NaN positions matter, NaN encodings do not; bool: the bytes)."""
    notes = []
    if len(got) != len(want):
        return [f"{len(got)} members, expected {len(want)}"]
    for i, (g, w) in enumerate(zip(got, want)):
        if coll == "all_gather":
            if g.dtype != w.dtype or not torch.equal(_bytes(g), _bytes(w)):
                bad = (_bytes(g) != _bytes(w)).nonzero().flatten() if g.numel() == w.numel() else []
                notes.append(f"member {i}: {len(bad)} bytes differ" + (f", first at +{int(bad[0])}" if len(bad) else ""))
        elif not E.same(g, w):
            if g.dtype == w.dtype and g.shape == w.shape and srcs is not None:
                notes.append("member %d: %d differ; (i, inputs, got, want): %s" %
                             ((i,) + E.mismatch(g.contiguous(), w.contiguous(), [s.contiguous() for s in srcs[i]], 2)))
            else:
                notes.append(f"member {i}: differs ({g.dtype} {tuple(g.shape)} vs {w.dtype} {tuple(w.shape)})")
    return notes


# ------------------------------------------------------------------------------------------------ cases
def case_key(case):
    coll, lst, dtn, op, entry, how = case
    return f"{coll}/{lst}/{dtn}/{op}/{entry}" + ("" if how == "std" else f"/{how}")


def build(case, rank, world, d):
    """(input arena, output arena or None) of one case on rank `rank`."""
    coll, lst, dtn, op, entry, how = case
    ms = members_of(lst, dtn)
    xs = inputs(coll, lst, dtn, how, world)
    salt = 1000 * (rank + 1) + zlib.crc32(case_key(case).encode()) % 997
    ain = Arena([(x[rank], kind) for x, (n, kind, dt) in zip(xs, ms)], d, salt)
    if coll == "all_reduce":
        return ain, None
    blanks = []
    for i, (n, kind, dt) in enumerate(ms):  # outputs: a pattern of their own, so an unwritten byte shows
        m = n * world if coll == "all_gather" else n
        okind = ("off" if kind == "off" else "flat") if coll == "all_gather" else ("flat" if kind == "t" else kind)
        blank = E.pattern(m * _esize(dt), 7 * salt + i).view(dt)
        blanks.append((blank.reshape(_shape(m, okind)), okind))
    return ain, Arena(blanks, d, salt + 1)


def issue(dist, pdist, case, ain, aout, d, force_async=False):
    """Starts the call of `case`; returns (waitable or None, notes on the Work)."""
    coll, lst, dtn, op, entry, how = case
    rop = getattr(dist.ReduceOp, op)
    asy = entry.endswith("_async")
    assert asy or not force_async
    ins = ain.ts
    outs = aout.ts if aout is not None else ins
    notes = []
    if entry.startswith("mgr"):
        with dist._coalescing_manager(device=d, async_ops=asy) as cm:
            for o, x in zip(outs, ins):
                if coll == "all_reduce":
                    dist.all_reduce(x, op=rop)
                elif coll == "all_gather":
                    dist.all_gather_into_tensor(o, x)
                else:
                    dist.reduce_scatter_tensor(o, x, op=rop)
        if not asy:
            return None, notes
        if len(cm.works) != 1:
            notes.append(f"{len(cm.works)} Works from the coalescing manager")
        return cm, notes
    if coll == "all_reduce":
        fut = dist.all_reduce_coalesced(ins, op=rop, async_op=asy)
        assert (fut is not None) == asy
        return fut, notes
    if coll == "all_gather":
        w = pdist.all_gather_into_tensor_coalesced(outs, ins, async_op=asy)
    else:
        w = pdist.reduce_scatter_tensor_coalesced(outs, ins, op=rop, async_op=asy)
    assert (w is not None) == asy
    # the single collective's Work carries the members (a list of one is the plain collective: its Work may carry
    # the output as W chunks)
    res = [t.data_ptr() for t in w.result()] if asy else []
    if asy and (res[:1] if len(outs) == 1 else res) != [o.data_ptr() for o in outs]:
        notes.append("the Work does not carry the members")
    return w, notes


def verdict(case, rank, world, ain, aout, label, notes, srcs=True):
    """[ok, engine label, detail] of a finished case: exact members, intact guards, untouched inputs."""
    coll, lst, dtn, op, entry, how = case
    notes = list(notes)
    xs = inputs(coll, lst, dtn, how, world)
    got_in, whole = ain.read()
    if coll == "all_reduce":
        got = got_in
    else:
        got, ok = aout.read()
        whole = whole and ok
        for i, (g, x) in enumerate(zip(got_in, xs)):
            if not torch.equal(_bytes(g), _bytes(x[rank])):
                notes.append(f"input {i} changed")
    per_member = [[x[q].reshape(-1) for q in range(world)] for x in xs] if coll == "all_reduce" and srcs else None
    notes += compare(coll, got, expected(coll, lst, dtn, how, op, world, rank), per_member)
    if not whole:
        notes.append("guard bytes changed")
    return [not notes, label, "; ".join(notes)[:600]]


def _raises(fn, *needles):
    try:
        fn()
    except (RuntimeError, ValueError, TypeError) as e:
        return [all(n in str(e) for n in needles), "", str(e).splitlines()[0][:300]]
    return [False, "", "no error"]


def errors(dist, pdist, rank, world, d):
    """The calls that must raise, on every rank, and an exact call on the same group after each."""
    out = {}
    f32 = torch.ones(8, dtype=torch.float32, device=d)
    i32 = torch.ones(8, dtype=torch.int32, device=d)

    def mixed_all_reduce():
        with dist._coalescing_manager(device=d, async_ops=False):
            dist.all_reduce(f32)
            dist.all_reduce(i32)

    out["error/all_reduce/mixed_dtypes"] = _raises(mixed_all_reduce, "allreduce_coalesced: tensor 1 has dtype",
                                                   "(a reduction is coalesced over one dtype)")
    out["error/reduce_scatter/mixed_dtypes"] = _raises(
        lambda: pdist.reduce_scatter_tensor_coalesced([f32, i32], [f32.repeat(world), i32.repeat(world)]),
        "reduce_scatter_tensor_coalesced: tensor 1 has dtype", "(a reduction is coalesced over one dtype)")
    premul = dist._make_nccl_premul_sum(2.0)
    out["error/reduce_scatter/premul_sum"] = _raises(
        lambda: pdist.reduce_scatter_tensor_coalesced([f32, f32.clone()], [f32.repeat(world), f32.repeat(world)],
                                                      op=premul), "PREMUL_SUM is not supported")
    if d.type == "cpu":
        # (CPU tensors only: there the dtype is checked before any rank communicates; on a GPU tensor the
        # reduction has no kernel and the host engine finds out in the middle of its exchange)
        b = [torch.ones(40, dtype=torch.bool), torch.zeros(24, dtype=torch.bool)]

        def avg_bool():
            with dist._coalescing_manager(device=d, async_ops=False):
                for t in b:
                    dist.all_reduce(t, op=dist.ReduceOp.AVG)

        out["error/all_reduce/avg_bool"] = _raises(avg_bool, "AVG on bool")
    return out


def coalesced(rank, size, device="cpu", plan=(), b2b=(), with_errors=True):
    """`plan`: ((collective, list, dtype name, op, entry point, "std" | "mixed"), ...); `b2b`: cases with async
    entry points, issued back to back without a wait in between. Returns {case: [ok, engine label, detail]}."""
    import torch.distributed as dist

    import pytorch_distributed_collective_communication_amd.distributed as pdist
    from pytorch_distributed_collective_communication_amd.parallel import backend as be

    d = _dev(device)
    # the ranks share this machine's cores (see _workers_exact.reductions)
    torch.set_num_threads(1 if d.type == "cpu" else 4)
    b = be.native_backend(None, d.type)

    def colls():  # collectives the backend recorded so far (as _workers.coalesced_probe counts them)
        return sum(v[0] for k, v in b.stats().items() if not k.startswith(("coalesced/", "rccl_comm/")))

    out = {}
    for case in plan:
        key = case_key(case)
        assert key not in out, key
        ain, aout = build(case, rank, size, d)
        c0 = colls()
        w, notes = issue(dist, pdist, case, ain, aout, d)
        if w is not None:
            w.wait()
        lab = b.last_algo()
        if colls() - c0 != 1:
            notes.append(f"{colls() - c0} collectives recorded for one call")
        out[key] = verdict(case, rank, size, ain, aout, lab, notes)
    if b2b:
        # every call takes its flat buffers from the caching allocator while the earlier collectives may still
        # run on the comm stream: none may be handed a buffer another one still reads or writes
        arenas = [build(case, rank, size, d) for case in b2b]
        c0 = colls()
        started = [issue(dist, pdist, case, ain, aout, d, force_async=True) for case, (ain, aout) in zip(b2b, arenas)]
        for w, _ in started:
            w.wait()
        lab = b.last_algo()
        notes, ok = [], True
        if colls() - c0 != len(b2b):
            notes.append(f"{colls() - c0} collectives recorded for {len(b2b)} calls")
        for case, (ain, aout), (_, n) in zip(b2b, arenas, started):
            v = verdict(case, rank, size, ain, aout, lab, n)
            if not v[0]:
                notes.append(f"{case_key(case)}: {v[2]}")
        out["back_to_back"] = [not notes, lab, "; ".join(notes)[:900]]
    if with_errors:
        after = AFTER_ERROR
        for key, v in errors(dist, pdist, rank, size, d).items():
            out[key] = v
            ain, aout = build(after, rank, size, d)  # the group still works, exactly
            issue(dist, pdist, after, ain, aout, d)
            out[key.replace("error/", "after/")] = verdict(after, rank, size, ain, aout, b.last_algo(), [])
    dist.barrier()
    return out


# ------------------------------------------------------------------------------------------------ plans
OTHER_LISTS = ("empty", "all_empty", "exact16", "views", "one")
GATHER_DTYPES = ("uint8", "bfloat16", "float32", "int64")  # element widths 1, 2, 4, 8
# mode -> the collectives it runs
MODES = {"ll": COLLS, "oneshot": COLLS, "twoshot": COLLS, "zc": COLLS, "dyn": COLLS, "push": ("all_reduce",),
         "staged_algo": COLLS, "sdma": ("all_gather",), "host": COLLS, "cpu": COLLS, "w8": COLLS, "w1": COLLS}


def plan_for(mode, world):
    """The cases of one launch. The first case of every collective (the ragged float32 SUM whose result depends
    on the rank order; for the gather ragged uint8) runs through all four entry points; over the other cases the
    entry points rotate, so each runs about a quarter of them."""
    plan = []
    for coll in MODES[mode]:
        manys = [f"many{k}" for k in many_counts(coll, world)]
        if mode == "w8":  # the W = 8 instantiation: the `many` lists
            lists = manys
        elif mode == "w1":
            lists = ["ragged", "empty", "views", "one"]
        else:
            lists = ["ragged"] + list(OTHER_LISTS) + manys
        cases = []
        if coll == "all_gather":
            cases += [(lst, "float32" if lst == "views" else "uint8", "SUM", "std") for lst in lists]
            if "ragged" in lists:
                cases += [("ragged", dtn, "SUM", "std") for dtn in GATHER_DTYPES[1:]] + [("mixed", "uint8", "SUM", "std")]
        else:
            for lst in lists:  # a float sum that depends on the order of the ranks, and SUM of full-range integers
                cases += [(lst, "float32", "SUM", "mixed"), (lst, "int32", "SUM", "std")]
            if mode not in ("w8", "w1"):
                cases += [("ragged", dtn, op, "std") for dtn, dt in E.DTYPES.items() for op in E.ops_for(dt)]
        lst, dtn, op, how = cases[0]
        plan += [(coll, lst, dtn, op, e, how) for e in ENTRIES]
        plan += [(coll, lst, dtn, op, ENTRIES[i % 4], how) for i, (lst, dtn, op, how) in enumerate(cases[1:])]
    assert len({case_key(c) for c in plan}) == len(plan)
    return tuple(plan)


def case_count(mode, world):
    """Cases of plan_for: per reduction 2 per list, 77 (dtype, op) pairs on the ragged list, 3 further entry
    points of the first case; per gather 1 per list, 3 more dtypes and the mixed list on ragged, 3 entry points."""
    total = 0
    for coll in MODES[mode]:
        manys = len(many_counts(coll, world))
        lists = manys if mode == "w8" else 4 if mode == "w1" else 6 + manys
        full = mode not in ("w8", "w1")
        if coll == "all_gather":
            total += lists + (4 if mode != "w8" else 0) + 3
        else:
            total += 2 * lists + (77 if full else 0) + 3
    return total


# the calls that must raise, each followed by an exact call: mixed dtypes (all-reduce, reduce-scatter),
# PREMUL_SUM, and on CPU tensors AVG on bool
ERRORS = {"cpu": 4, "cuda": 3}
AFTER_ERROR = ("all_reduce", "ragged", "int32", "SUM", "api", "std")


def b2b_for(mode, world):
    """Four async calls of different lists and sizes, over the collectives the mode runs."""
    picks = (("ragged", "float32", "SUM", "mgr_async", "mixed"), ("many", "int32", "SUM", "api_async", "std"),
             ("exact16", "int32", "MAX", "mgr_async", "std"), ("views", "float32", "SUM", "api_async", "mixed"))
    out = []
    for i, (lst, dtn, op, entry, how) in enumerate(picks):
        coll = MODES[mode][i % len(MODES[mode])]
        if lst == "many":
            lst = f"many{many_counts(coll, max(world, 2))[-1]}"
        if coll == "all_gather":
            dtn, op, how = ("float32" if lst == "views" else "uint8"), "SUM", "std"
        out.append((coll, lst, dtn, op, entry, how))
    return tuple(out)


def engine_label(mode, case, world):
    """The label a GPU case must record, from csrc/backend/gpu_ops.cpp (choose, enqueue_allreduce,
    enqueue_allgather, enqueue_reduce_scatter, ipc_run and record()'s "_zc") at the thresholds
    tests/test_coalesced_gpu.py sets, and the *_coalesced rows of tests/golden/engine_labels.json: a coalesced
    call records the label of the plain collective at the packed size (the whole buffer of an all-reduce, one
    rank's block of the other two)."""
    coll, lst, dtn, op, entry, how = case
    nbytes = packed_bytes(lst, dtn)
    if nbytes == 0 or world == 1:
        return "local"  # gpu_allreduce / gpu_allgather / gpu_reduce_scatter return early
    if mode == "host" or (dtn == "int16" and coll != "all_gather"):
        return "host"   # forced; or no kernel for the dtype (red_spec: kok false), no RCCL among ranks of one GPU
    if mode == "ll" and nbytes <= LL_CAP:
        return "ipc_ll"
    zc = mode in ("zc", "dyn", "push", "sdma") and nbytes >= ZC_MIN
    if coll == "all_reduce":
        if nbytes <= (ONESHOT_DEFAULT if mode in ("ll", "oneshot") else ONESHOT):
            return "ipc_1shot"
        base = {"push": "ipc_push", "dyn": "ipc_2shot_dyn"}.get(mode, "ipc_2shot")
        return base + ("_zc" if zc and nbytes >= world * T else "")  # (zero copy takes whole rows of W tiles)
    if coll == "all_gather" and mode == "sdma" and zc:
        return "ipc_sdma_zc"
    if coll == "reduce_scatter" and nbytes % 16:
        # (only a list of one: the plain reduce_scatter_tensor. Its chunks are not all 16-byte aligned then,
        # prep_in copies them, they stop being one buffer and nothing is exported: gpu_reduce_scatter, is_flat)
        zc = False
    return ("ipc_dyn" if mode == "dyn" else "ipc") + ("_zc" if zc else "")
