#!/usr/bin/env python3
"""The fused AdamW step that emits the parameter wire next to the sequence it replaces, in one run and on the same
tensors (interleaved rounds, medians; nothing here is a pass / fail gate).

One process, GPU 0. At 64 MiB and 1 GiB of parameter shard, for f32 and bf16 parameters, both state formats and the
three wires, two ways from (gradient shard, f64 total) to (new state, new master, parameter wire):
  * fused:  one ops.adamw_step(..., param_out=None, wire_out=w, wire=F, wire_dtype=dtype);
  * split:  ops.adamw_step(..., param_out=param_shard) followed by ops.mx_quantize(param_shard, 1, out=w, wire=F):
            what ShardedOptimizer(params, "adamw", param_wire=F) ran before.
Both step the same master and state (a step is a step whichever way took it), alternating inside every round. Times are
device events around back-to-back calls after a warm-up call; per case the file holds the median, minimum and maximum
over the rounds in microseconds, the ratio of the medians, the ratio of the bytes either way has to move (arithmetic),
and whether the difference is beyond the run's own spread (one way's slowest round below the other's fastest). The
step as a whole across GPUs (reduce-scatter, this, all-gather) is not measured here.

    python scripts/adamw_wire_bench.py [--rounds 7] [--out profiles/zero/adamw_wire_kernels.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adamw_bench import HP  # noqa: E402
from mx_rot_bench import timeit  # noqa: E402

WIRES = {"fp8": "mxfp8_e4m3", "fp4": "mxfp4_e2m1", "fp6": "mxfp6_e2m3"}


def ways_for(mib, dtn, state, wire, ops, torch, dev):
    """({way: fn}, bytes fused, bytes split); the buffers live in the closures."""
    dt, esize = {"f32": (torch.float32, 4), "bf16": (torch.bfloat16, 2)}[dtn]
    n = (mib << 20) // esize
    grad = (torch.randn(n, device=dev) * 1e-2).to(dt)
    shard = torch.empty(n, dtype=dt, device=dev)
    total, master = ops.sumsq([grad]), torch.randn(n, device=dev)
    nb, nw = ops.mx_wire_bytes(n, 1), ops.mx_wire_bytes(n, 1, wire=wire)
    w = torch.empty(nw, dtype=torch.uint8, device=dev)
    if state is None:
        m, v, sbytes = torch.zeros(n, device=dev), torch.zeros(n, device=dev), 16 * n
    else:  # (the state of zeros: payload 0, scale bytes 127)
        m, v = (torch.cat([torch.zeros(nb - nb // 33, dtype=torch.uint8, device=dev),
                           torch.full((nb // 33,), 127, dtype=torch.uint8, device=dev)]) for _ in range(2))
        sbytes = 4 * nb
    count, kw = [0], dict(total=total, max_norm=1.0, **({} if state is None else {"state_format": state}), **HP)

    def fused():
        count[0] += 1
        ops.adamw_step(grad, master, m, v, step=count[0], wire_out=w, wire=wire, wire_dtype=dt, **kw)

    def split():
        count[0] += 1
        ops.adamw_step(grad, master, m, v, step=count[0], param_out=shard, **kw)
        ops.mx_quantize(shard, 1, out=w, wire=wire)

    step = n * (esize + 8) + sbytes  # grad, the master read and written, the state read and written
    return {"fused": fused, "split": split}, step + nw, step + n * esize + n * esize + nw


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024], help="MiB of parameter shard")
    ap.add_argument("--out", default=os.path.join("profiles", "zero", "adamw_wire_kernels.json"))
    a = ap.parse_args()

    import torch

    from pytorch_distributed_collective_communication_amd import ops

    assert torch.cuda.is_available(), "adamw_wire_bench.py measures on a GPU; there is no fallback"
    dev = torch.device("cuda", 0)
    rows = {}
    for mib in a.sizes:
        for dtn in ("f32", "bf16"):
            for sn, state in (("state32", None), ("state8", "mxfp8_e4m3")):
                for wn, wire in WIRES.items():
                    ways, bf, bs = ways_for(mib, dtn, state, wire, ops, torch, dev)
                    raw = {k: [] for k in ways}
                    iters = 20 if mib <= 64 else 5
                    for _ in range(a.rounds):
                        for key, fn in ways.items():  # the ways alternate inside every round
                            raw[key].append(timeit(fn, iters) * 1e6)
                    row = {k: {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2),
                               "us_max": round(max(v), 2)} for k, v in raw.items()}
                    row["time_ratio_fused_over_split"] = round(row["fused"]["us_median"] / row["split"]["us_median"], 3)
                    row["bytes_ratio_fused_over_split"] = round(bf / bs, 3)
                    row["fused_tb_per_s"] = round(bf / row["fused"]["us_median"] / 1e6, 3)
                    row["beyond_the_spread"] = (row["fused"]["us_max"] < row["split"]["us_min"]
                                                or row["split"]["us_max"] < row["fused"]["us_min"])
                    rows[f"{dtn}_{mib}MiB_{sn}_{wn}"] = row
                    print(f"{dtn}_{mib}MiB_{sn}_{wn}", row["fused"]["us_median"], row["split"]["us_median"],
                          row["time_ratio_fused_over_split"], row["bytes_ratio_fused_over_split"],
                          row["beyond_the_spread"], flush=True)
                    del ways
                    torch.cuda.empty_cache()
    doc = {
        "what": "ops.adamw_step(wire_out=...) (one kernel: clip coefficient, AdamW, the parameter wire) next to "
                "ops.adamw_step(param_out=param_shard) + ops.mx_quantize(param_shard, 1), in the same run on the same "
                "tensors: device-event microseconds per call (median, min, max over interleaved rounds), the ratio of "
                "the medians and of the bytes (arithmetic). One GPU; the whole ZeRO step across GPUs is not measured",
        "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "rows": rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
