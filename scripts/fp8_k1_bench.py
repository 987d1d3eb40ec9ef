#!/usr/bin/env python3
"""FP8 K1 against int8 K1 on the same bytes (interleaved rounds in one process, medians).

An FP8 reduce moves exactly the traffic of the int8 one, and the int8 kernel is the one the library
had before FP8: anything the FP8 medians lose beyond the int8 rounds' own min-max spread is the cost of
the conversions. SUM of 2 and 8 sources of `--mib` MiB each, impls lds_ntl and stream_ntl, dtypes int8 /
float8_e4m3fn / float8_e5m2 over the SAME buffers (bytes 0x00-0x37: small positive values in every
format). Then one small-message figure: a 64 KiB all_reduce at W = 2 (ranks sharing one GPU, LL
protocol), per-call time of back-to-back calls, the three dtypes interleaved.

    python scripts/fp8_k1_bench.py [--rounds 6] [--mib 256] [--out profiles/fp8/k1_fp8_vs_i8.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DTYPES = ("int8", "float8_e4m3fn", "float8_e5m2")


def timeit(fn, iters=8):
    import torch

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters / 1e3


def k1(rounds, mib):
    import torch

    from pytorch_distributed_collective_communication_amd import ops

    dev = torch.device("cuda", 0)
    n = mib << 20
    raw = {}
    for nsrc in (2, 8):
        g = torch.Generator(device=dev).manual_seed(5)
        bufs = [torch.randint(0, 0x38, (n,), dtype=torch.uint8, device=dev, generator=g) for _ in range(nsrc)]
        dst = torch.empty(n, dtype=torch.uint8, device=dev)
        for _ in range(rounds):
            for impl in ("lds_ntl", "stream_ntl"):
                for dtn in DTYPES:
                    dt = getattr(torch, dtn)
                    srcs, out = [b.view(dt) for b in bufs], dst.view(dt)
                    t = timeit(lambda: ops.reduce_nway(srcs, out=out, op="sum", impl=impl))
                    raw.setdefault(f"n{nsrc}_{impl}_{dtn}", []).append(round((nsrc + 1) * n / t / 1e9, 1))
        del bufs, dst
        torch.cuda.empty_cache()
    return raw


def ll_work(rank, size, nbytes, rounds):
    import torch
    import torch.distributed as dist

    from pytorch_distributed_collective_communication_amd.parallel import backend as be

    dev = torch.device("cuda", torch.cuda.current_device())
    b = be.native_backend(None, "cuda")
    xs = {dtn: torch.full((nbytes,), 1, dtype=torch.uint8, device=dev).view(getattr(torch, dtn)) for dtn in DTYPES}
    raw, algo = {}, {}
    for dtn, x in xs.items():
        for _ in range(20):
            dist.all_reduce(x.clone())
        algo[dtn] = b.last_algo()
    for _ in range(rounds):
        for dtn, x in xs.items():
            y = x.clone()
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(50):
                dist.all_reduce(y)  # (SUM; the kernels' time does not depend on the values)
            torch.cuda.synchronize()
            t = torch.tensor([(time.perf_counter() - t0) / 50], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            raw.setdefault(dtn, []).append(round(t.item() * 1e6, 2))
    return {"rounds_us": raw, "algo": algo}


def summarize(raw, higher_is_better):
    """Medians, the int8 rounds' min-max spread, and each FP8 median's gap to the int8 median."""
    out = {}
    for key in sorted({k.rsplit("_int8", 1)[0] for k in raw if k.endswith("_int8")}):
        i8 = raw[f"{key}_int8"]
        row = {"int8_median": statistics.median(i8), "int8_spread": round(max(i8) - min(i8), 2)}
        for dtn in DTYPES[1:]:
            m = statistics.median(raw[f"{key}_{dtn}"])
            gap = row["int8_median"] - m if higher_is_better else m - row["int8_median"]
            row[f"{dtn}_median"] = m
            row[f"{dtn}_behind_int8"] = round(gap, 2)
            row[f"{dtn}_within_spread"] = gap <= row["int8_spread"]
        out[key] = row
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--mib", type=int, default=256, help="MiB per K1 source")
    ap.add_argument("--ll-bytes", type=int, default=64 << 10)
    ap.add_argument("--out", default=os.path.join("profiles", "fp8", "k1_fp8_vs_i8.json"))
    a = ap.parse_args()
    from pytorch_distributed_collective_communication_amd.parallel.spawn import launch

    # the children first: this process has not touched the GPU yet
    res = launch(ll_work, 2, args=(a.ll_bytes, a.rounds), bind_device=True, timeout_s=120,
                 env={"PDCC_SPAWN_DEVICE": "0", "PDCC_ALGO": "ipc"}, join_timeout_s=600)
    ll_raw = {f"allreduce_w2_{a.ll_bytes}B_{dtn}": v for dtn, v in res[0]["rounds_us"].items()}
    k1_raw = k1(a.rounds, a.mib)
    doc = {
        "what": "K1 SUM GB/s (bytes read + written) per round, and the per-call us of back-to-back "
                "all_reduce calls at W = 2 on one GPU; FP8 against int8 on the same bytes",
        "rounds": a.rounds, "mib_per_source": a.mib,
        "k1_gbps_rounds": k1_raw, "k1_summary": summarize(k1_raw, True),
        "allreduce_us_rounds": ll_raw, "allreduce_algo": res[0]["algo"], "allreduce_summary": summarize(ll_raw, False),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"k1": doc["k1_summary"], "allreduce": doc["allreduce_summary"]}))


if __name__ == "__main__":
    main()
