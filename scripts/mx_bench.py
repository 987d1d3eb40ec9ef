#!/usr/bin/env python3
"""The mxfp8_e4m3 wire kernels against torch's own FP8 casts (interleaved rounds, medians; nothing
here is a pass / fail gate).

One process, GPU 0, f32 tensors of --kernel-mib MiB each:
  * mx_quantize against `out.copy_(x)` into a float8_e4m3fn tensor -- the same traffic class (reads
    4n, writes n; the kernel writes 33n/32 and does one 8-lane max per block);
  * mx_dequantize against the copy back (float8 -> f32);
  * mx_reduce of 2 and 8 chunk wires (no torch counterpart: GB/s only).
GB/s = bytes the operation must read + write / time (device events around back-to-back calls).

  * (--what fold) mx_fold of 2 and 8 chunk wires into f32 and bf16 against the pair it replaces on
    an owner, mx_reduce then mx_dequantize, in the same run and on the same wires: microseconds of
    both, their min-max over the rounds, and the fold's GB/s over nsrc * 33 cb + numel * element
    size bytes; and mx_quantize_shards against mx_quantize at 8 chunks, where the two layouts are
    the same bytes. The fold moves strictly fewer bytes than the pair; the margin of "no slower" is
    the spread of the rounds, nothing tighter.

The collectives themselves (all_reduce_compressed against dist.all_reduce, reduce_scatter_compressed
against dist.reduce_scatter_tensor) are not measured here: see BASELINE.md "mxfp8_e4m3 wire".

    python scripts/mx_bench.py [--rounds 5] [--what kernels fold] [--out profiles/mx/mx_kernels.json]
                               [--fold-out profiles/mx/mx_fold.json]
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


def fold(rounds, mibs):
    """{case: [seconds per call, one per round]} and {case: bytes}: mx_fold against mx_reduce + mx_dequantize on
    the same wires, mx_quantize_shards against mx_quantize; the cases of one size alternate within a round."""
    import torch

    from pytorch_distributed_collective_communication_amd import ops

    dev = torch.device("cuda", 0)
    raw, nbytes = {}, {}
    for mib in mibs:
        n = (mib << 20) // 4
        iters = max(4, min(40, 4096 // mib))
        cb = ops.mx_shard_blocks(n)
        x = torch.randn(n, device=dev)
        cases = {}
        wins = {}
        for nsrc in (2, 8):
            win = torch.empty(33 * cb * nsrc, dtype=torch.uint8, device=dev)
            for r in range(nsrc):
                ops.mx_quantize(x * float(r + 1), 1, out=win[33 * cb * r:33 * cb * (r + 1)])
            wins[nsrc] = win
            mid = torch.empty(33 * cb, dtype=torch.uint8, device=dev)
            for dtn, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                o = torch.empty(n, dtype=dt, device=dev)
                key = f"{nsrc}_{dtn}_{mib}MiB"
                cases[f"mx_fold_{key}"] = lambda win=win, nsrc=nsrc, dt=dt, o=o: ops.mx_fold(win, nsrc, n, dt, "sum", out=o)

                def pair(win=win, nsrc=nsrc, dt=dt, o=o, mid=mid):
                    ops.mx_reduce(win, nsrc, "sum", out=mid)
                    ops.mx_dequantize(mid, n, dt, 1, out=o)

                cases[f"mx_reduce_then_dequantize_{key}"] = pair
                nbytes[f"mx_fold_{key}"] = nbytes[f"mx_reduce_then_dequantize_{key}"] = (
                    win.numel() + n * o.element_size())
        # 8 chunks of whole 4096-block tiles: the dealt wire and the shard wire are the same bytes
        assert 32 * ops.mx_chunk_blocks(n, 8) * 8 == n and ops.mx_shard_wire_bytes(n // 8, 8) == ops.mx_wire_bytes(n, 8)
        w8 = torch.empty(ops.mx_wire_bytes(n, 8), dtype=torch.uint8, device=dev)
        ws8 = torch.empty_like(w8)
        cases[f"mx_quantize_f32_w8_{mib}MiB"] = lambda: ops.mx_quantize(x, 8, out=w8)
        cases[f"mx_quantize_shards_f32_w8_{mib}MiB"] = lambda: ops.mx_quantize_shards(x, 8, out=ws8)
        nbytes[f"mx_quantize_f32_w8_{mib}MiB"] = nbytes[f"mx_quantize_shards_f32_w8_{mib}MiB"] = 4 * n + w8.numel()
        for _ in range(rounds):
            for name, fn in cases.items():
                raw.setdefault(name, []).append(timeit(fn, iters))
        assert torch.equal(w8, ws8)
        del x, cases, wins, w8, ws8
        torch.cuda.empty_cache()
    return raw, nbytes


def fold_doc(raw, nbytes, rounds):
    """Per case: microseconds (median, min, max over the rounds) and GB/s of the median; per pair of cases:
    the ratio of the medians and whether the new one is slower beyond the spread (min of the new above max of the old)."""
    rows = {}
    for k, v in sorted(raw.items()):
        us = [t * 1e6 for t in v]
        rows[k] = {"us_median": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                   "gbps_median": round(nbytes[k] / statistics.median(v) / 1e9, 1), "bytes": nbytes[k]}
    verdicts = {}
    for k in rows:
        if k.startswith("mx_fold_"):
            old = "mx_reduce_then_dequantize_" + k[len("mx_fold_"):]
        elif k.startswith("mx_quantize_shards_"):
            old = "mx_quantize_" + k[len("mx_quantize_shards_"):]
        else:
            continue
        verdicts[k] = {"against": old, "time_ratio_new_over_old": round(rows[k]["us_median"] / rows[old]["us_median"], 3),
                       "slower_beyond_the_spread": rows[k]["us_min"] > rows[old]["us_max"]}
    return {
        "what": "mx_fold against mx_reduce + mx_dequantize on the same wires, and mx_quantize_shards against mx_quantize "
                "at 8 chunks (same bytes): device-event microseconds per call, interleaved rounds; GB/s over the bytes "
                "the new operation must read and write (nsrc * 33 cb + numel * element size for the fold)",
        "rounds": rounds, "rows": rows, "comparisons": verdicts,
        "rounds_us": {k: [round(t * 1e6, 2) for t in v] for k, v in sorted(raw.items())},
    }


def medians(raw):
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in sorted(raw.items())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-mib", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--out", default=os.path.join("profiles", "mx", "mx_kernels.json"))
    ap.add_argument("--what", nargs="+", choices=("kernels", "fold"), default=["kernels", "fold"])
    ap.add_argument("--fold-out", default=os.path.join("profiles", "mx", "mx_fold.json"))
    a = ap.parse_args()
    if "fold" in a.what:
        fdoc = fold_doc(*fold(a.rounds, a.kernel_mib), a.rounds)
        os.makedirs(os.path.dirname(os.path.abspath(a.fold_out)), exist_ok=True)
        with open(a.fold_out, "w") as f:
            json.dump(fdoc, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps({"fold": fdoc["comparisons"]}))
    if "kernels" not in a.what:
        return
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
