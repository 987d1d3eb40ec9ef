"""The IPC collectives' launch plan, without a GPU.

``kern::ipc_plan`` (csrc/kernels/ipc_plan.h) holds everything ``ipc_launch`` decides before it
launches: which calls are rejected, the grid (part of the protocol: every rank must compute the same
one from the call's arguments), the kernel family, the canonical dtype / op; ``ipc_staging_bytes``
sizes the staging over the same protocol table. ``tests/native/ipc_plan_dump.cpp`` prints those
decisions for ~3.8 thousand calls (every protocol x world x mode x size, explicit grids and caps,
roots, every dtype / op pair, unsupported worlds); the golden file holds the decisions recorded from
the launch code as it was before the table existed (BASELINE.md says how). The program is built with
ASan + UBSan, so the table lookups are checked for bounds on the way.
"""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
BUILD = os.path.join(ROOT, "build", "san")
SRC = os.path.join(ROOT, "tests", "native", "ipc_plan_dump.cpp")
HDRS = [os.path.join(CSRC, "kernels", h) for h in ("ipc_plan.h", "kernel_api.h")]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _build() -> str:
    exe = os.path.join(BUILD, "ipc_plan_dump")
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(p) for p in [SRC] + HDRS):
        return exe
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
           "-D__HIP_PLATFORM_AMD__=1", f"-I{CSRC}", f"-I{os.path.join(ROCM, 'include')}", SRC, "-o", exe + ".tmp"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-6000:]
    os.replace(exe + ".tmp", exe)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plan_and_staging_match_the_recorded_launch_decisions():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    with open(os.path.join(ROOT, "tests", "golden", "ipc_plan.json")) as f:
        gold = json.load(f)
    calls, got = zip(*(line.split(" -> ") for line in r.stdout.splitlines()))
    # the same calls in the same order as recorded, then every call's decision, row for row
    assert len(calls) == gold["calls"] > 3500
    assert hashlib.sha256("\n".join(calls).encode()).hexdigest() == gold["calls_sha256"]
    want = [gold["decisions"][k] for k in gold["rows"]]
    bad = [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not bad, f"{len(bad)} rows differ; first: {calls[bad[0][0]]}\n  want {bad[0][1]}\n  got  {bad[0][2]}"
    assert len(got) == len(want)
