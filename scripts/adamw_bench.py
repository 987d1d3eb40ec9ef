#!/usr/bin/env python3
"""The fused AdamW shard step next to the compositions it replaces, in one run and on the same shapes (interleaved
rounds, medians; nothing here is a pass / fail gate).

One process, GPU 0. At 64 MiB and 1 GiB of parameter shard, for f32 and bf16 parameters, three ways of taking a shard
from (gradient shard, f64 total) to (new state, new master, param_shard):
  * hip:      one ops.adamw_step(grad, master, exp_avg, exp_avg_sq, total=..., param_out=param_shard);
  * hip8:     the same call with state_format="mxfp8_e4m3": the two moments as block-scaled 8-bit buffers
              (docs/collectives.md "8-bit AdamW state"), dequantized and requantized in the same pass;
  * foreach:  ops.clip_scale(grad, total, c, out=f32 master gradient; in place for f32) + torch.optim.AdamW(foreach=True)
              .step() on the master + param_shard.copy_(master): what ShardedOptimizer(torch.optim.AdamW,
              max_grad_norm=c) runs today;
  * fused:    the same with torch.optim.AdamW(fused=True).
Every way owns its own state, so all three keep stepping from round to round. The ways alternate inside every
round. Times are device events around back-to-back calls after a warm-up call; per case the file holds the median,
minimum and maximum over the rounds in microseconds, the bytes the hip kernel has to move (grad + three f32 reads +
three f32 writes + param_shard) over its median (TB/s), the ratios of the medians, and whether each difference is
beyond the run's own spread (one way's slowest round below the other's fastest). The step as a whole across GPUs
(reduce-scatter, this, all-gather) is not measured here.

    python scripts/adamw_bench.py [--rounds 7] [--out profiles/zero/adamw_kernels.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_rot_bench import timeit  # noqa: E402

HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def ways_for(mib, dtn, ops, torch, dev):
    """({way: fn}, bytes the hip kernel moves); the buffers live in the closures."""
    dt, esize = {"f32": (torch.float32, 4), "bf16": (torch.bfloat16, 2)}[dtn]
    n = (mib << 20) // esize
    grad = (torch.randn(n, device=dev) * 1e-2).to(dt)
    shard = torch.empty(n, dtype=dt, device=dev)
    total = ops.sumsq([grad])
    ways = {}

    master, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    count = [0]

    def hip():
        count[0] += 1
        ops.adamw_step(grad, master, m, v, step=count[0], param_out=shard, total=total, max_norm=1.0, **HP)

    ways["hip"] = hip
    master8 = torch.randn(n, device=dev)
    nb = ops.mx_wire_bytes(n, 1)  # (the state of zeros: payload 0, scale bytes 127)
    m8, s8 = (torch.cat([torch.zeros(nb - nb // 33, dtype=torch.uint8, device=dev),
                         torch.full((nb // 33,), 127, dtype=torch.uint8, device=dev)]) for _ in range(2))
    count8 = [0]

    def hip8():
        count8[0] += 1
        ops.adamw_step(grad, master8, m8, s8, step=count8[0], param_out=shard, total=total, max_norm=1.0,
                       state_format="mxfp8_e4m3", **HP)

    ways["hip8"] = hip8
    for name, kw in (("foreach", dict(foreach=True)), ("fused", dict(fused=True))):
        mw = torch.randn(n, device=dev)
        mg = grad.clone() if dt == torch.float32 else torch.empty(n, device=dev)
        src = mg if dt == torch.float32 else grad  # (f32: scaled in place, as the optimizer does; coefficient < 1 shrinks
        mw.grad = mg                               #  it from call to call, which changes no timing)
        opt = torch.optim.AdamW([mw], **HP, **kw)

        def composed(opt=opt, mw=mw, mg=mg, src=src):
            ops.clip_scale(src, total, 1.0, out=mg)
            opt.step()
            shard.copy_(mw)

        ways[name] = composed
    return ways, n * (esize + 12 + 12 + esize), n * (esize + 4 + 4 + esize) + 4 * nb


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024], help="MiB of parameter shard")
    ap.add_argument("--out", default=os.path.join("profiles", "zero", "adamw_kernels.json"))
    a = ap.parse_args()

    import torch

    from pytorch_distributed_collective_communication_amd import ops

    assert torch.cuda.is_available(), "adamw_bench.py measures on a GPU; there is no fallback"
    dev = torch.device("cuda", 0)
    rows = {}
    for mib in a.sizes:
        for dtn in ("f32", "bf16"):
            ways, nbytes, nbytes8 = ways_for(mib, dtn, ops, torch, dev)
            raw = {k: [] for k in ways}
            iters = 20 if mib <= 64 else 5
            for _ in range(a.rounds):
                for key, fn in ways.items():  # the ways alternate inside every round
                    raw[key].append(timeit(fn, iters) * 1e6)
            row = {k: {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2),
                       "us_max": round(max(v), 2), "us_rounds": [round(u, 2) for u in v]} for k, v in raw.items()}
            row["bytes"] = nbytes
            row["hip_tb_per_s"] = round(nbytes / row["hip"]["us_median"] / 1e6, 3)
            row["bytes_hip8"] = nbytes8
            row["hip8_tb_per_s"] = round(nbytes8 / row["hip8"]["us_median"] / 1e6, 3)
            row["time_ratio_hip8_over_hip"] = round(row["hip8"]["us_median"] / row["hip"]["us_median"], 3)
            row["bytes_ratio_hip8_over_hip"] = round(nbytes8 / nbytes, 3)
            row["beyond_the_spread_hip8"] = (row["hip8"]["us_max"] < row["hip"]["us_min"]
                                             or row["hip"]["us_max"] < row["hip8"]["us_min"])
            for other in ("foreach", "fused"):
                row[f"time_ratio_hip_over_{other}"] = round(row["hip"]["us_median"] / row[other]["us_median"], 3)
                row[f"beyond_the_spread_{other}"] = (row["hip"]["us_max"] < row[other]["us_min"]
                                                     or row[other]["us_max"] < row["hip"]["us_min"])
            rows[f"{dtn}_{mib}MiB"] = row
            del ways
            torch.cuda.empty_cache()
    doc = {
        "what": "ops.adamw_step (clip coefficient, AdamW, cast into param_shard: one kernel) next to ops.clip_scale + "
                "torch.optim.AdamW(foreach=True / fused=True).step() + param_shard.copy_(master), in the same run on the "
                "same shapes: device-event microseconds per call (median, min, max over interleaved rounds), the hip "
                "kernel's bytes over its median, and the ratios of the medians. One GPU; the whole ZeRO step across "
                "GPUs is not measured",
        "hip8": "ops.adamw_step(state_format='mxfp8_e4m3') in the same rounds: its own bytes (grad, master read and "
                "written, two state wires read and written, param_shard), TB/s, and the ratio of its median to hip's",
        "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "rows": rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: [v["hip_tb_per_s"], v["time_ratio_hip_over_foreach"], v["time_ratio_hip_over_fused"],
                          v["beyond_the_spread_foreach"], v["beyond_the_spread_fused"], v["hip8_tb_per_s"],
                          v["time_ratio_hip8_over_hip"], v["beyond_the_spread_hip8"]] for k, v in rows.items()}))


if __name__ == "__main__":
    main()
