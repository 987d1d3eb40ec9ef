#!/usr/bin/env python3
"""The error-feedback kernels against what they replace, in one run and on the same tensors
(interleaved rounds, medians; nothing here is a pass / fail gate).

One process, GPU 0. For every tensor size (--mib, MiB of the tensor itself), dtype (f32, bf16) and
wire (mxfp8_e4m3, mxfp4_e2m1), three ways to the same wire and the same residual:
  * fused:    ops.mx_quantize(x, out=w, residual=r) -- one kernel;
  * unfused:  the composition it replaces, four passes with every buffer preallocated:
              torch.add(x, r, out=v); ops.mx_quantize(v, out=w); ops.mx_dequantize(w, out=d);
              torch.sub(v, d, out=r)   (no reset of non-finite residuals, which the fused kernel does)
  * plain:    ops.mx_quantize(x, out=w) -- no feedback at all, the floor.
and for the f32 sizes ops.mx_reduce of 2 and 8 chunk wires with and without the owner residual.

Byte arithmetic per f32 element (wire of 33/32 B; 17/32 for FP4): fused 4 + 4 + 4 + 1 = 13, unfused
12 + 5 + 5 + 12 = 34, plain 5. The criterion is that the fused kernel beats the unfused composition as
measured in this same run, the variants alternating inside every round. Times are device events around
back-to-back calls after a warm-up call; per variant the file holds the median, minimum and maximum over
the rounds in microseconds and the GB/s of the median over the bytes it must read and write; per case
the ratios of the medians and whether the fused kernel is faster beyond the spread (its slowest round
below the composition's fastest).

The collectives themselves are not measured here: nothing cross-GPU has been measured for error feedback.

    python scripts/mx_ef_bench.py [--rounds 7] [--mib 64 1024] [--out profiles/mx/mx_ef_kernels.json]
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
    r = torch.zeros(n, device=dev)    # the fused kernel's residual
    r2 = torch.zeros(n, device=dev)   # the composition's
    v = torch.empty(n, device=dev)
    d = torch.empty(n, device=dev)
    out = {}

    def add(name, variant, fn, nbytes):
        out.setdefault(name, {})[variant] = (fn, nbytes)

    for key, wire in WIRES.items():
        wb = ops.mx_wire_bytes(n, 1, wire=wire)
        w1 = torch.empty(wb, dtype=torch.uint8, device=dev)
        name = f"mx_quantize_{key}_{dtn}_{mib}MiB"

        def unfused(w1=w1, wire=wire):
            torch.add(x, r2, out=v)
            ops.mx_quantize(v, 1, out=w1, wire=wire)
            ops.mx_dequantize(w1, n, torch.float32, 1, out=d, wire=wire)
            torch.sub(v, d, out=r2)

        add(name, "fused", lambda w1=w1, wire=wire: ops.mx_quantize(x, 1, out=w1, wire=wire, residual=r),
            (esize + 8) * n + wb)
        add(name, "unfused", unfused, (esize + 8) * n + (4 * n + wb) + (wb + 4 * n) + 12 * n)
        add(name, "plain", lambda w1=w1, wire=wire: ops.mx_quantize(x, 1, out=w1, wire=wire), esize * n + wb)
        if dtn != "f32":
            continue  # (mx_reduce never sees the tensor's dtype)
        chunk = ops.mx_shard_wire_bytes(n, 1, wire=wire)
        win = torch.empty(chunk * 8, dtype=torch.uint8, device=dev)
        for k in range(8):
            ops.mx_quantize(x * float(k + 1), 1, out=win[chunk * k:chunk * (k + 1)], wire=wire)
        mid = torch.empty(chunk, dtype=torch.uint8, device=dev)
        own = torch.zeros(ops.mx_owner_residual_numel(n, 1, wire=wire), device=dev)
        for nsrc in (2, 8):
            src = win[:chunk * nsrc]
            name = f"mx_reduce_{nsrc}_{key}_{mib}MiB"
            add(name, "fused", lambda src=src, nsrc=nsrc, mid=mid, wire=wire, own=own:
                ops.mx_reduce(src, nsrc, "sum", out=mid, wire=wire, residual=own), src.numel() + chunk + 8 * own.numel())
            add(name, "plain", lambda src=src, nsrc=nsrc, mid=mid, wire=wire:
                ops.mx_reduce(src, nsrc, "sum", out=mid, wire=wire), src.numel() + chunk)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--mib", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--out", default=os.path.join("profiles", "mx", "mx_ef_kernels.json"))
    a = ap.parse_args()

    import torch

    from pytorch_distributed_collective_communication_amd import ops

    assert torch.cuda.is_available(), "mx_ef_bench.py measures on a GPU; there is no fallback"
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
        row["time_ratio_fused_over_plain"] = round(row["fused"]["us_median"] / row["plain"]["us_median"], 3)
        row["bytes_ratio_fused_over_plain"] = round(row["fused"]["bytes"] / row["plain"]["bytes"], 3)
        if "unfused" in row:
            row["time_ratio_unfused_over_fused"] = round(row["unfused"]["us_median"] / row["fused"]["us_median"], 3)
            row["bytes_ratio_unfused_over_fused"] = round(row["unfused"]["bytes"] / row["fused"]["bytes"], 3)
            row["fused_faster_beyond_the_spread"] = row["fused"]["us_max"] < row["unfused"]["us_min"]
        rows[name] = row
    doc = {
        "what": "the fused error-feedback kernels (mx_quantize / mx_reduce with residual=) against the plain kernels "
                "and, for quantize, against the four-pass composition they replace (add, mx_quantize, mx_dequantize, "
                "subtract), in the same run on the same tensors: device-event microseconds per call (median, min, max "
                "over interleaved rounds), GB/s of the median over the bytes each must read and write, and the ratios "
                "of the medians next to the ratios of those bytes",
        "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "rows": rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: [v.get("time_ratio_unfused_over_fused"), v["time_ratio_fused_over_plain"],
                          v.get("fused_faster_beyond_the_spread")] for k, v in rows.items()}))


if __name__ == "__main__":
    main()
