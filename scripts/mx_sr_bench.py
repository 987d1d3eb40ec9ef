#!/usr/bin/env python3
"""The stochastic-rounding kernels against the nearest ones and against what they are the alternative to,
the error-feedback kernels, in one run and on the same tensors (interleaved rounds, medians).

One process, GPU 0. For every tensor size (--mib, MiB of the tensor itself), dtype (f32, bf16) and
wire (mxfp8_e4m3, mxfp4_e2m1), three quantizers into the same wire buffer:
  * stochastic: ops.mx_quantize(x, out=w, rounding="stochastic", seed=...) -- the bytes of the plain kernel
                plus, per element, one counter-based word and the integer rounding of mx_sr.h;
  * nearest:    ops.mx_quantize(x, out=w) -- the floor;
  * feedback:   ops.mx_quantize(x, out=w, residual=r) -- the stateful alternative.
and for the f32 sizes ops.mx_reduce of 2 and 8 chunk wires, stochastic against nearest.

Byte arithmetic per f32 element (wire of 33/32 B; 17/32 for FP4): stochastic and nearest 5, feedback 13.
The criterion is that the stochastic quantize is no slower than the error-feedback quantize on the same
tensor, medians of this same run, the variants alternating inside every round; the script exits non-zero
otherwise. The ratio to the nearest quantize is reported, not judged. Times are device events around
back-to-back calls after a warm-up call; per variant the file holds the median, minimum and maximum over
the rounds in microseconds and the GB/s of the median over the bytes it must read and write -- where the
stochastic kernel's GB/s falls below the nearest kernel's it is bound by its integer work, not by memory.

The collectives themselves are not measured here: nothing cross-GPU has been measured for stochastic
rounding.

    python scripts/mx_sr_bench.py [--rounds 7] [--mib 64 1024] [--out profiles/mx/mx_sr_kernels.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIRES = {"fp8": "mxfp8_e4m3", "fp4": "mxfp4_e2m1"}


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
    """{case: {variant: (fn, bytes)}} for one tensor size and dtype; the buffers live in the closures."""
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dtn]
    esize = 4 if dtn == "f32" else 2
    n = (mib << 20) // esize
    x = torch.randn(n, device=dev).to(dt)
    r = torch.zeros(n, device=dev)    # the error-feedback kernel's residual
    out = {}

    def add(name, variant, fn, nbytes):
        out.setdefault(name, {})[variant] = (fn, nbytes)

    for key, wire in WIRES.items():
        wb = ops.mx_wire_bytes(n, 1, wire=wire)
        w1 = torch.empty(wb, dtype=torch.uint8, device=dev)
        name = f"mx_quantize_{key}_{dtn}_{mib}MiB"
        add(name, "stochastic", lambda w1=w1, wire=wire: ops.mx_quantize(x, 1, out=w1, wire=wire, rounding="stochastic",
                                                                         seed=1234, stream=1), esize * n + wb)
        add(name, "nearest", lambda w1=w1, wire=wire: ops.mx_quantize(x, 1, out=w1, wire=wire), esize * n + wb)
        add(name, "feedback", lambda w1=w1, wire=wire: ops.mx_quantize(x, 1, out=w1, wire=wire, residual=r),
            (esize + 8) * n + wb)
        if dtn != "f32":
            continue  # (mx_reduce never sees the tensor's dtype)
        chunk = ops.mx_shard_wire_bytes(n, 1, wire=wire)
        win = torch.empty(chunk * 8, dtype=torch.uint8, device=dev)
        for k in range(8):
            ops.mx_quantize(x * float(k + 1), 1, out=win[chunk * k:chunk * (k + 1)], wire=wire)
        mid = torch.empty(chunk, dtype=torch.uint8, device=dev)
        for nsrc in (2, 8):
            src = win[:chunk * nsrc]
            name = f"mx_reduce_{nsrc}_{key}_{mib}MiB"
            add(name, "stochastic", lambda src=src, nsrc=nsrc, mid=mid, wire=wire:
                ops.mx_reduce(src, nsrc, "sum", out=mid, wire=wire, rounding="stochastic", seed=1234, stream=1),
                src.numel() + chunk)
            add(name, "nearest", lambda src=src, nsrc=nsrc, mid=mid, wire=wire:
                ops.mx_reduce(src, nsrc, "sum", out=mid, wire=wire), src.numel() + chunk)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--mib", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--out", default=os.path.join("profiles", "mx", "mx_sr_kernels.json"))
    a = ap.parse_args()

    import torch

    from pytorch_distributed_collective_communication_amd import ops

    assert torch.cuda.is_available(), "mx_sr_bench.py measures on a GPU; there is no fallback"
    dev = torch.device("cuda", 0)
    raw, nbytes = {}, {}
    for mib in a.mib:
        iters = max(8, min(200, 16384 // mib))
        for dtn in ("f32", "bf16"):
            cases = cases_for(mib, dtn, ops, torch, dev)
            for _ in range(a.rounds):
                for name, variants in cases.items():
                    for key, (fn, nb) in variants.items():  # the variants alternate inside every round
                        raw.setdefault(name, {}).setdefault(key, []).append(timeit(fn, iters))
                        nbytes.setdefault(name, {})[key] = nb
            del cases
            torch.cuda.empty_cache()

    rows = {}
    for name in sorted(raw):
        row = {}
        for key, ts in raw[name].items():
            us = [t * 1e6 for t in ts]
            row[key] = {"us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2),
                        "us_max": round(max(us), 2), "bytes": nbytes[name][key],
                        "gbps_median": round(nbytes[name][key] / statistics.median(ts) / 1e9, 1),
                        "us_rounds": [round(u, 2) for u in us]}
        row["time_ratio_stochastic_over_nearest"] = round(row["stochastic"]["us_median"] / row["nearest"]["us_median"], 3)
        if "feedback" in row:
            row["time_ratio_stochastic_over_feedback"] = round(row["stochastic"]["us_median"]
                                                               / row["feedback"]["us_median"], 3)
            row["bytes_ratio_stochastic_over_feedback"] = round(row["stochastic"]["bytes"] / row["feedback"]["bytes"], 3)
            row["stochastic_no_slower_than_feedback"] = row["stochastic"]["us_median"] <= row["feedback"]["us_median"]
            row["stochastic_faster_beyond_the_spread"] = row["stochastic"]["us_max"] < row["feedback"]["us_min"]
        rows[name] = row
    doc = {
        "what": "the stochastic-rounding kernels (mx_quantize / mx_reduce with rounding='stochastic') against the "
                "nearest kernels and, for quantize, against the error-feedback kernel they are the alternative to, in "
                "the same run on the same tensors: device-event microseconds per call (median, min, max over "
                "interleaved rounds), GB/s of the median over the bytes each must read and write, and the ratios of "
                "the medians; the criterion is stochastic_no_slower_than_feedback in every quantize row",
        "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "rows": rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: [v["time_ratio_stochastic_over_nearest"], v.get("time_ratio_stochastic_over_feedback"),
                          v.get("stochastic_no_slower_than_feedback")] for k, v in rows.items()}))
    slower = [k for k, v in rows.items() if v.get("stochastic_no_slower_than_feedback") is False]
    if slower:
        sys.exit("the stochastic quantize is slower than the error-feedback quantize in: " + ", ".join(slower))


if __name__ == "__main__":
    main()
