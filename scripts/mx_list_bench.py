#!/usr/bin/env python3
"""The tensor-list kernels next to the packed path they replace, in one run and on the same tensors (interleaved
rounds, medians; nothing here is a pass / fail gate).

One process, GPU 0. For the FP8 and FP4 wires, f32 and bf16, and three lists of tensors:
  * equal8:      256 MiB in 8 equal tensors;
  * transformer: 4 layers of a transformer-like mix: four d x d and two d x 4d matrices with their 1-D biases and
                 two norms per layer (d = 1024);
  * tiny4096:    4096 tensors of 4 KiB;
three ways to take the list to a wire and back:
  * list:   mx_quantize_list + mx_dequantize_list, the tensors read and written where they are;
  * packed: K2 ops.pack into a flat bucket, mx_quantize, mx_dequantize, K2 ops.unpack (what GradBucketer does
            around the collective today; for f32 about 26 bytes per element against the list's 10);
  * flat:   (equal8 only) mx_quantize + mx_dequantize of one tensor of the same size, the kernels' own speed.
The ways alternate inside every round. Times are device events around back-to-back calls after a warm-up call; per
case the file holds the median, minimum and maximum over the rounds in microseconds, the ratio of the list's
median to the others', and whether the list is faster than the packed path beyond the run's own spread (its
slowest round below the packed path's fastest).

The collectives themselves are not measured here: nothing cross-GPU has been measured for any wire.

    python scripts/mx_list_bench.py [--rounds 7] [--out profiles/mx/mx_list_kernels.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_rot_bench import timeit  # noqa: E402

WIRES = {"fp8": "mxfp8_e4m3", "fp4": "mxfp4_e2m1"}


def shapes(esize):
    d = 1024
    layer = [d * d, d] * 4 + [d * 4 * d, 4 * d, 4 * d * d, d] + [d, d, d, d]
    return {"equal8": [(256 << 20) // esize // 8] * 8, "transformer": layer * 4, "tiny4096": [4096 // esize] * 4096}


def ways_for(numels, dt, wire, ops, torch, dev, flat_too):
    """{way: fn}; the buffers live in the closures."""
    xs = [torch.randn(n, device=dev).to(dt) for n in numels]
    total = sum(numels)
    wl = torch.empty(ops.mx_wire_bytes(ops.mx_list_numel(numels), 1, wire=wire), dtype=torch.uint8, device=dev)
    wp = torch.empty(ops.mx_wire_bytes(total, 1, wire=wire), dtype=torch.uint8, device=dev)
    bucket = torch.empty(total, dtype=dt, device=dev)

    def as_list():
        ops.mx_quantize_list(xs, 1, out=wl, wire=wire)
        ops.mx_dequantize_list(wl, xs, 1, wire=wire)

    def packed():
        ops.pack(xs, out=bucket.view(torch.uint8))
        ops.mx_quantize(bucket, 1, out=wp, wire=wire)
        ops.mx_dequantize(wp, total, dt, 1, out=bucket, wire=wire)
        ops.unpack(bucket.view(torch.uint8), xs)

    def flat():
        ops.mx_quantize(bucket, 1, out=wp, wire=wire)
        ops.mx_dequantize(wp, total, dt, 1, out=bucket, wire=wire)

    return {"list": as_list, "packed": packed, **({"flat": flat} if flat_too else {})}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "mx", "mx_list_kernels.json"))
    a = ap.parse_args()

    import torch

    from pytorch_distributed_collective_communication_amd import ops

    assert torch.cuda.is_available(), "mx_list_bench.py measures on a GPU; there is no fallback"
    dev = torch.device("cuda", 0)
    rows = {}
    for dtn, dt, esize in (("f32", torch.float32, 4), ("bf16", torch.bfloat16, 2)):
        for shape, numels in shapes(esize).items():
            for wkey, wire in WIRES.items():
                ways = ways_for(numels, dt, wire, ops, torch, dev, shape == "equal8")
                raw = {k: [] for k in ways}
                for _ in range(a.rounds):
                    for key, fn in ways.items():  # the ways alternate inside every round
                        raw[key].append(timeit(fn, 20) * 1e6)
                row = {k: {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2),
                           "us_max": round(max(v), 2), "us_rounds": [round(u, 2) for u in v]} for k, v in raw.items()}
                row["tensors"], row["elements"] = len(numels), sum(numels)
                for other in ways:
                    if other != "list":
                        row[f"time_ratio_list_over_{other}"] = round(row["list"]["us_median"] / row[other]["us_median"], 3)
                row["list_faster_than_packed_beyond_the_spread"] = row["list"]["us_max"] < row["packed"]["us_min"]
                if "flat" in row:
                    row["list_within_the_spread_of_flat"] = row["list"]["us_min"] <= row["flat"]["us_max"]
                rows[f"{shape}_{dtn}_{wkey}"] = row
                del ways
                torch.cuda.empty_cache()
    doc = {
        "what": "mx_quantize_list + mx_dequantize_list (list) next to pack + mx_quantize + mx_dequantize + unpack (packed) "
                "and, for the 8 equal tensors, mx_quantize + mx_dequantize of one tensor of the same size (flat), in the "
                "same run on the same tensors: device-event microseconds per round trip (median, min, max over interleaved "
                "rounds) and the ratios of the medians",
        "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "rows": rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: [v["time_ratio_list_over_packed"], v["list_faster_than_packed_beyond_the_spread"],
                          v.get("time_ratio_list_over_flat")] for k, v in rows.items()}))


if __name__ == "__main__":
    main()
