#!/usr/bin/env python3
"""The gradient-clipping kernels next to the torch ops they replace, in one run and on the same tensors (interleaved
rounds, medians; nothing here is a pass / fail gate).

One process, GPU 0. At 64 MiB and 1 GiB, for f32 and bf16:
  * sumsq:  ops.sumsq([x]) next to torch.linalg.vector_norm(x) (which leaves the norm in x's dtype, not an f64 sum
            of squares with a fixed order: the closest thing torch offers, not the same contract);
  * clip:   (bf16 only) ops.clip_scale(x, total, c, out=f32 buffer) next to x.to(torch.float32) followed by mul_ with
            a 0-d device tensor, what the step would do with torch ops once the coefficient is on the device.
The two ways alternate inside every round. Times are device events around back-to-back calls after a warm-up call;
per case the file holds the median, minimum and maximum over the rounds in microseconds, the bytes the kernel has to
move over its median (TB/s), the ratio of the medians, and whether the difference is beyond the run's own spread
(one way's slowest round below the other's fastest).

    python scripts/clip_bench.py [--rounds 7] [--out profiles/zero/clip_kernels.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_rot_bench import timeit  # noqa: E402


def cases_for(mib, dtn, ops, torch, dev):
    """{case: ({way: fn}, bytes the hip kernel moves)}; the buffers live in the closures."""
    dt, esize = {"f32": (torch.float32, 4), "bf16": (torch.bfloat16, 2)}[dtn]
    n = (mib << 20) // esize
    x = torch.randn(n, device=dev).to(dt)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    cases = {"sumsq": ({"hip": lambda: ops.sumsq([x], total), "torch": lambda: torch.linalg.vector_norm(x)}, n * esize)}
    if dtn == "bf16":
        out = torch.empty(n, dtype=torch.float32, device=dev)
        ops.sumsq([x], total)
        coef = torch.tensor(0.5, device=dev)
        cases["clip"] = ({"hip": lambda: ops.clip_scale(x, total, 1.0, out=out),
                          "torch": lambda: x.to(torch.float32).mul_(coef)}, n * (esize + 4))
    return cases


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024], help="MiB")
    ap.add_argument("--out", default=os.path.join("profiles", "zero", "clip_kernels.json"))
    a = ap.parse_args()

    import torch

    from pytorch_distributed_collective_communication_amd import ops

    assert torch.cuda.is_available(), "clip_bench.py measures on a GPU; there is no fallback"
    dev = torch.device("cuda", 0)
    rows = {}
    for mib in a.sizes:
        for dtn in ("f32", "bf16"):
            for case, (ways, nbytes) in cases_for(mib, dtn, ops, torch, dev).items():
                raw = {k: [] for k in ways}
                iters = 50 if mib <= 64 else 10
                for _ in range(a.rounds):
                    for key, fn in ways.items():  # the ways alternate inside every round
                        raw[key].append(timeit(fn, iters) * 1e6)
                row = {k: {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2),
                           "us_max": round(max(v), 2), "us_rounds": [round(u, 2) for u in v]} for k, v in raw.items()}
                row["bytes"] = nbytes
                row["hip_tb_per_s"] = round(nbytes / row["hip"]["us_median"] / 1e6, 3)
                row["time_ratio_hip_over_torch"] = round(row["hip"]["us_median"] / row["torch"]["us_median"], 3)
                row["beyond_the_spread"] = (row["hip"]["us_max"] < row["torch"]["us_min"]
                                            or row["torch"]["us_max"] < row["hip"]["us_min"])
                rows[f"{case}_{dtn}_{mib}MiB"] = row
            torch.cuda.empty_cache()
    doc = {
        "what": "ops.sumsq next to torch.linalg.vector_norm, and ops.clip_scale (bf16 -> f32) next to .to(float32) + mul_ "
                "by a device scalar, in the same run on the same tensors: device-event microseconds per call (median, "
                "min, max over interleaved rounds), the hip kernel's bytes over its median, and the ratio of the medians",
        "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "rows": rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: [v["hip_tb_per_s"], v["time_ratio_hip_over_torch"], v["beyond_the_spread"]]
                      for k, v in rows.items()}))


if __name__ == "__main__":
    main()
