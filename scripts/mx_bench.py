#!/usr/bin/env python3
"""The mxfp8_e4m3 wire kernels against torch's own FP8 casts (interleaved rounds, medians; nothing
here is a pass / fail gate).

One process, GPU 0, f32 tensors of --kernel-mib MiB each:
  * mx_quantize against `out.copy_(x)` into a float8_e4m3fn tensor -- the same traffic class (reads
    4n, writes n; the kernel writes 33n/32 and does one 8-lane max per block);
  * mx_dequantize against the copy back (float8 -> f32);
  * mx_reduce of 2 and 8 chunk wires (no torch counterpart: GB/s only).
GB/s = bytes the operation must read + write / time (device events around back-to-back calls).

The collective itself (all_reduce_compressed against dist.all_reduce) is not measured here yet:
see BASELINE.md "mxfp8_e4m3 wire".

    python scripts/mx_bench.py [--rounds 5] [--out profiles/mx/mx_kernels.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def kernels(rounds, mibs):
    import torch

    from pytorch_distributed_collective_communication_amd import ops

    dev = torch.device("cuda", 0)
    raw = {}
    for mib in mibs:
        n = (mib << 20) // 4
        iters = max(4, min(40, 4096 // mib))
        x = torch.randn(n, device=dev)
        f8 = torch.empty(n, dtype=torch.float8_e4m3fn, device=dev)
        back = torch.empty(n, device=dev)
        wire = torch.empty(ops.mx_wire_bytes(n, 1), dtype=torch.uint8, device=dev)
        cases = {
            "torch_cast_f32_to_f8": (lambda: f8.copy_(x), 5 * n),
            "mx_quantize_f32": (lambda: ops.mx_quantize(x, 1, out=wire), 4 * n + wire.numel()),
            "torch_cast_f8_to_f32": (lambda: back.copy_(f8), 5 * n),
            "mx_dequantize_f32": (lambda: ops.mx_dequantize(wire, n, torch.float32, 1, out=back), 4 * n + wire.numel()),
        }
        for nsrc in (2, 8):
            win = torch.empty(ops.mx_wire_bytes(n, nsrc), dtype=torch.uint8, device=dev)
            ops.mx_quantize(x, nsrc, out=win)
            wout = torch.empty(win.numel() // nsrc, dtype=torch.uint8, device=dev)
            cases[f"mx_reduce_{nsrc}"] = (lambda win=win, wout=wout, nsrc=nsrc: ops.mx_reduce(win, nsrc, "sum", out=wout),
                                          win.numel() + wout.numel())
        for _ in range(rounds):
            for name, (fn, nbytes) in cases.items():
                raw.setdefault(f"{name}_{mib}MiB", []).append(round(nbytes / timeit(fn, iters) / 1e9, 1))
        del x, f8, back, wire, cases
        torch.cuda.empty_cache()
    return raw


def medians(raw):
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in sorted(raw.items())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-mib", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--out", default=os.path.join("profiles", "mx", "mx_kernels.json"))
    a = ap.parse_args()
    kraw = kernels(a.rounds, a.kernel_mib)
    krows = medians(kraw)
    for mib in a.kernel_mib:
        for mine, theirs in (("mx_quantize_f32", "torch_cast_f32_to_f8"), ("mx_dequantize_f32", "torch_cast_f8_to_f32")):
            krows[f"{mine}_{mib}MiB"]["rate_over_torch_cast"] = round(
                krows[f"{mine}_{mib}MiB"]["median"] / krows[f"{theirs}_{mib}MiB"]["median"], 3)
    doc = {
        "what": "kernel GB/s (bytes read + written over device-event time) of the mxfp8_e4m3 kernels against "
                "torch's FP8 casts of the same tensor; interleaved rounds",
        "rounds": a.rounds, "kernels_gbps": krows, "kernels_gbps_rounds": kraw,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"kernels_gbps": krows}))


if __name__ == "__main__":
    main()
