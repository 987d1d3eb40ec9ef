"""Data, the plain-torch expectation and the rank workers of the tests of the fused AdamW step that emits the parameter
wire (docs/collectives.md "Parameter wire from the step")."""
import functools

import torch

from tests import _workers_adamw8 as W8
from tests._workers_adamw import HP
from tests._workers_clip import DTYPES
from tests._workers_mx import _dev

FMT = W8.FMT
NUMELS = (40, 4096 + 36, 2 * 4096 + 32 * 5 + 3, 32 * 31761)
TOTAL, MAX_NORM = 4e4, 1.0  # a total that clips (coefficient 1 / 200)
KEYS = ("master", "exp_avg", "exp_avg_sq", "param_out", "wire")


def _ops():
    from pytorch_distributed_collective_communication_amd import ops

    return ops


@functools.lru_cache(maxsize=None)
def data(n, dtn, state):
    """CPU inputs of one step (tests/_workers_adamw8.py data; `state` None: the moments unpacked to f32) whose new
    master has an inf in block 0, a tiny element in block 1 and, from 96 elements on, an all-zero block 2."""
    x = {k: v.clone() for k, v in W8.data(n, dtn).items()}
    x["master"][3], x["master"][33] = float("inf"), x["master"][32:40].abs().max() * 2.0 ** -30
    x["master"][W8.ZERO] = 0
    if state is None:
        x["exp_avg"], x["exp_avg_sq"] = (t.contiguous() for t in _ops().adamw_state_unpack(x["exp_avg"], x["exp_avg_sq"], n))
    return x


@functools.lru_cache(maxsize=None)
def expected(n, dtn, state, wire, device="cpu"):
    """What one clipped step of `data` leaves: adamw_step_reference's master, state and param_out (of the gradient's
    dtype) on the same inputs on `device` -- the plain torch operations of the device the step under test runs on --
    and mx_quantize_reference of that param_out. Computed once per case and shared."""
    ops, d = _ops(), _dev(device)
    x = {k: v.clone().to(d) for k, v in data(n, dtn, state).items()}
    x["param_out"] = torch.zeros(n, dtype=DTYPES[dtn], device=d)
    ops.adamw_step_reference(x["grad"], x["master"], x["exp_avg"], x["exp_avg_sq"], step=3, param_out=x["param_out"],
                             total=torch.tensor([TOTAL], dtype=torch.float64, device=d), max_norm=MAX_NORM,
                             state_format=state, **HP)
    x = {k: v.cpu() for k, v in x.items()}
    x["wire"] = ops.mx_quantize_reference(x["param_out"], 1, wire=wire)
    return x


def step(x, wire, state, device="cpu", param_out=True, fn=None, max_blocks=0, **kw):
    """One clipped step of ops.adamw_step (or `fn`) with wire_out on copies of the CPU inputs `x` on `device`; the
    wire buffer carries 64 guard bytes behind it. Returns the CPU results under KEYS."""
    ops, d = _ops(), _dev(device)
    t = {k: v.clone().to(d) for k, v in x.items()}
    nb = ops.mx_wire_bytes(t["grad"].numel(), 1, wire=wire)
    buf = torch.full((nb + 64,), 0xA5, dtype=torch.uint8, device=d)
    po = torch.zeros_like(t["grad"]) if param_out else None
    dt = {} if param_out else {"wire_dtype": t["grad"].dtype}
    more = {} if fn is not None else {"max_blocks": max_blocks}  # (the reference has no grid)
    (fn or ops.adamw_step)(t["grad"], t["master"], t["exp_avg"], t["exp_avg_sq"], step=3, param_out=po,
                           total=torch.tensor([TOTAL], dtype=torch.float64, device=d), max_norm=MAX_NORM,
                           state_format=state, wire_out=buf[:nb], wire=wire, **dt, **more, **HP, **kw)
    assert bool((buf[nb:] == 0xA5).all()), "guard bytes behind the wire"
    assert torch.equal(t["grad"].cpu().view(torch.uint8), x["grad"].view(torch.uint8))
    return {**{k: t[k].cpu() for k in KEYS[:3]}, "param_out": None if po is None else po.cpu(), "wire": buf[:nb].cpu()}


def same_bytes(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@functools.lru_cache(maxsize=None)
def ran(n, dtn, state, wire, device, max_blocks=0):
    """`step` of `data` on `device`, once per case."""
    return step(data(n, dtn, state), wire, state, device, max_blocks=max_blocks)


def check_wire(got, n, wire):
    """The emitted buffer is, byte for byte and over all of it, mx_quantize_reference of the call's own param_out: the
    inf block, the zero block and the blank tail among it; param_out is the master rounded once."""
    ops = _ops()
    assert same_bytes(got["wire"], ops.mx_quantize_reference(got["param_out"], 1, wire=wire)), "wire of param_out"
    ok = ~got["master"].isnan()
    assert torch.equal(got["param_out"][ok], got["master"].to(got["param_out"].dtype)[ok])
    cb, blocks = ops.mx_chunk_blocks(n, 1, wire=wire), -(-n // 32)
    scales = got["wire"][-cb:]
    assert scales[0] == 255 and bool((scales[blocks:] == 127).all()) and (n < 96 or scales[2] == 127)


def check_reference(got, ref):
    """Master, state, param_out and the wire against `expected`, byte for byte (printed first: per tensor the bytes
    that differ and the largest difference)."""
    for k in KEYS:
        if got[k].dtype != torch.uint8:
            bad = got[k].view(torch.uint8) != ref[k].view(torch.uint8)
            print(k, int(bad.sum()), float((got[k].double() - ref[k].double()).abs().nan_to_num(0.0).max()))
    for k in KEYS:
        assert same_bytes(got[k], ref[k]), k


def check_spans(device, wire="mxfp6_e2m3", fn=None):
    """Packed state of 3 * 64 elements stepped as three spans with state_offset 0 / 64 / 128, each with its own wire,
    against one whole-shard reference step; then the ValueErrors of state_offset."""
    ops, n, d = _ops(), 192, _dev(device)
    x, ref = data(n, "bfloat16", FMT), expected(n, "bfloat16", FMT, wire, device)
    t = {k: v.clone().to(d) for k, v in x.items()}
    total = torch.tensor([TOTAL], dtype=torch.float64, device=d)
    call = lambda g, m, off, **kw: (fn or ops.adamw_step)(  # noqa: E731
        g, m, t["exp_avg"], t["exp_avg_sq"], step=3, total=total, max_norm=MAX_NORM, state_format=FMT, state_offset=off,
        wire_dtype=torch.bfloat16, wire=wire, **kw, **HP)
    for off in (0, 64, 128):
        w = torch.empty(ops.mx_wire_bytes(64, 1, wire=wire), dtype=torch.uint8, device=d)
        call(t["grad"][off:off + 64], t["master"][off:off + 64], off, wire_out=w)
        assert same_bytes(w.cpu(), ops.mx_quantize_reference(ref["param_out"][off:off + 64], 1, wire=wire)), off
    whole = step(x, wire, FMT, device, param_out=False)  # one launch over the whole shard on the same device
    assert all(same_bytes(t[k].cpu(), whole[k]) for k in KEYS[:3]), "three spans against one launch"
    for off, m in ((16, 64), (0, 48), (32 * 16 - 32, 64), (-32, 64)):  # no multiple of 32 (twice), past the state, negative
        try:
            call(torch.zeros(m, dtype=torch.bfloat16, device=d), torch.zeros(m, device=d), off)
            raise AssertionError((off, m))
        except ValueError:
            pass
    assert all(same_bytes(t[k].cpu(), ref[k]) for k in KEYS[:3]), "against the whole-shard reference step"


def zero(rank, size, device="cuda"):
    """Two steps of ShardedOptimizer(ps, "adamw", param_wire=w, max_grad_norm=1.0, overlap=False) with two buckets, on a
    bf16 and an f32 model, FP8 and FP4 wires, both state formats. `flat` must be, bit for bit, the dequantized
    concatenation of every rank's reference wire of its master slice of each bucket. {case: [fused, flat ok]} and
    whether a rotation turns the fusion off."""
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd.parallel.zero import ShardedOptimizer

    ops, d, out = _ops(), _dev(device), {}
    for dtn in ("bfloat16", "float32"):
        for w in ("mxfp8_e4m3", "mxfp4_e2m1"):
            for state in (None, FMT):
                torch.manual_seed(7)
                ps = list(torch.nn.Linear(40, 9).to(d).to(DTYPES[dtn]).parameters())
                opt = ShardedOptimizer(ps, "adamw", param_wire=w, max_grad_norm=1.0, overlap=False, state_format=state,
                                       bucket_bytes=64, **HP)
                (s,), ok = opt.spaces, len(opt.spaces[0].buckets) == 2
                for n in (1, 2):
                    for i, p in enumerate(ps):
                        p.grad.copy_(W8.hand_grad(p.shape, rank, n, i))
                    opt.step()
                    masters = [torch.empty_like(s.master) for _ in range(size)]
                    dist.all_gather(masters, s.master)
                    for b in s.buckets:
                        every = torch.cat([ops.mx_quantize_reference(m[b.soff:b.soff + b.shard].cpu().to(s.dtype), 1, wire=w)
                                           for m in masters])
                        want = ops.mx_dequantize_shards_reference(every, b.shard, s.dtype, size, wire=w)
                        ok = ok and same_bytes(s.flat[b.off:b.off + b.padded].cpu(), want.reshape(-1))
                out[f"{dtn} {w} {state}"] = [opt.fused_param_wire, ok]
                opt.remove_hooks()
    opt = ShardedOptimizer(list(torch.nn.Linear(6, 5).to(d).parameters()), "adamw", param_wire="mxfp8_e4m3",
                           param_rotation="hadamard", overlap=False)
    out["rotation"] = [opt.fused_param_wire, True]
    opt.remove_hooks()
    return out


def gather_input_wire(rank, size):
    """CPU, two ranks: all_gather_compressed(input_wire=Q(input)) equals the call without it, and the two refusals."""
    from pytorch_distributed_collective_communication_amd.parallel.compressed import all_gather_compressed

    ops, out = _ops(), {}
    for wire in ops.MX_WIRES:
        x = W8.clip_data(100, 7 + rank, torch.bfloat16)
        a, b = torch.zeros(size * 100, dtype=torch.bfloat16), torch.zeros(size * 100, dtype=torch.bfloat16)
        all_gather_compressed(a, x, wire=wire)
        all_gather_compressed(b, x, wire=wire, input_wire=ops.mx_quantize_reference(x, 1, wire=wire))
        out[wire] = same_bytes(a, b) and bool(a.any())
    for name, kw in (("stochastic", dict(rounding="stochastic", seed=1)), ("rotation", dict(rotation="hadamard"))):
        try:
            all_gather_compressed(a, x, input_wire=ops.mx_quantize_reference(x, 1), **kw)
            out[name] = False
        except ValueError:
            out[name] = True
    return out
