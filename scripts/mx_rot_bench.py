#!/usr/bin/env python3
"""The Hadamard-rotated wire kernels next to their plain twins, in one run and on the same tensors (interleaved
rounds, medians; nothing here is a pass / fail gate).

One process, GPU 0. For every wire format, tensor size (--mib, MiB of the tensor itself) and dtype (f32, bf16):
  * mx_quantize plain, with a residual (error feedback) and stochastic; mx_dequantize (1 chunk);
  * mx_fold of 2 and 8 chunk wires into the tensor;
each with ``rotation="hadamard"`` and without, the two alternating inside every round. A rotated kernel moves the
bytes of its twin and adds five add / subtract stages and two (bf16) or three (f32) lane exchanges per element
group, so the expectation is a ratio near 1. Times are device events around back-to-back calls after a warm-up
call; per case the file holds the median, minimum and maximum over the rounds in microseconds, the GB/s of the
median over the bytes the kernel must read and write, the ratio of the rotated median to the plain one, and whether
the rotated kernel is slower than its twin beyond the run's own spread (its fastest round above the twin's slowest).

The collectives themselves are not measured here: nothing cross-GPU has been measured for any wire.

    python scripts/mx_rot_bench.py [--rounds 7] [--mib 64 1024] [--out profiles/mx/mx_rot_kernels.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIRES = {"fp8": "mxfp8_e4m3", "fp6": "mxfp6_e2m3", "fp4": "mxfp4_e2m1"}
TWINS = {"plain": {}, "rot": dict(rotation="hadamard", rotation_seed=20261021)}


def timeit(fn, iters):
    import torch

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters / 1e3


def cases_for(mib, dtn, ops, torch, dev):
    """{case: {twin key: (fn, bytes)}} for one tensor size and dtype; the buffers live in the closures."""
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtn]
    esize = 4 if dtn == "f32" else 2
    n = (mib << 20) // esize
    x = torch.randn(n, device=dev).to(dt)
    back = torch.empty(n, dtype=dt, device=dev)
    res = torch.zeros(n, dtype=torch.float32, device=dev)
    out = {}

    def add(name, key, fn, nbytes):
        out.setdefault(f"{name}_{dtn}_{mib}MiB", {})[key] = (fn, nbytes)

    for wkey, wire in WIRES.items():
        w1 = torch.empty(ops.mx_wire_bytes(n, 1, wire=wire), dtype=torch.uint8, device=dev)
        chunk = ops.mx_shard_wire_bytes(n, 1, wire=wire)
        win = torch.empty(chunk * 8, dtype=torch.uint8, device=dev)
        for r in range(8):
            ops.mx_quantize(x * float(r + 1), 1, out=win[chunk * r:chunk * (r + 1)], wire=wire)
        for key, rot in TWINS.items():
            add(f"mx_quantize_{wkey}", key, lambda w1=w1, wire=wire, rot=rot: ops.mx_quantize(x, 1, out=w1, wire=wire, **rot),
                esize * n + w1.numel())
            add(f"mx_quantize_ef_{wkey}", key, lambda w1=w1, wire=wire, rot=rot:
                ops.mx_quantize(x, 1, out=w1, wire=wire, residual=res, **rot), esize * n + 8 * n + w1.numel())
            add(f"mx_quantize_sr_{wkey}", key, lambda w1=w1, wire=wire, rot=rot:
                ops.mx_quantize(x, 1, out=w1, wire=wire, rounding="stochastic", seed=1234, **rot), esize * n + w1.numel())
            add(f"mx_dequantize_{wkey}", key, lambda w1=w1, wire=wire, rot=rot:
                ops.mx_dequantize(w1, n, dt, 1, out=back, wire=wire, **rot), esize * n + w1.numel())
            for nsrc in (2, 8):
                src = win[:chunk * nsrc]
                add(f"mx_fold_{nsrc}_{wkey}", key, lambda src=src, nsrc=nsrc, wire=wire, rot=rot:
                    ops.mx_fold(src, nsrc, n, dt, "sum", out=back, wire=wire, **rot), src.numel() + esize * n)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--mib", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--out", default=os.path.join("profiles", "mx", "mx_rot_kernels.json"))
    a = ap.parse_args()

    import torch

    from pytorch_distributed_collective_communication_amd import ops

    assert torch.cuda.is_available(), "mx_rot_bench.py measures on a GPU; there is no fallback"
    dev = torch.device("cuda", 0)
    raw, nbytes = {}, {}
    for mib in a.mib:
        iters = max(8, min(200, 16384 // mib))
        for dtn in ("f32", "bf16"):
            cases = cases_for(mib, dtn, ops, torch, dev)
            for _ in range(a.rounds):
                for name, pair in cases.items():
                    for key in TWINS:  # the twins alternate inside every round
                        fn, nb = pair[key]
                        raw.setdefault(name, {}).setdefault(key, []).append(timeit(fn, iters))
                        nbytes.setdefault(name, {})[key] = nb
            del cases
            torch.cuda.empty_cache()

    rows = {}
    for name in sorted(raw):
        row = {}
        for key in TWINS:
            us = [t * 1e6 for t in raw[name][key]]
            row[key] = {"us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2),
                        "us_max": round(max(us), 2), "bytes": nbytes[name][key],
                        "gbps_median": round(nbytes[name][key] / statistics.median(raw[name][key]) / 1e9, 1),
                        "us_rounds": [round(u, 2) for u in us]}
        row["time_ratio_rot_over_plain"] = round(row["rot"]["us_median"] / row["plain"]["us_median"], 3)
        row["rot_slower_beyond_the_spread"] = row["rot"]["us_min"] > row["plain"]["us_max"]
        rows[name] = row
    doc = {
        "what": "the Hadamard-rotated kernels next to their plain twins in the same run on the same tensors: "
                "device-event microseconds per call (median, min, max over interleaved rounds), GB/s of the median over "
                "the bytes the kernel must read and write, and the ratio of the medians",
        "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "rows": rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: [v["time_ratio_rot_over_plain"], v["rot_slower_beyond_the_spread"]] for k, v in rows.items()}))


if __name__ == "__main__":
    main()
