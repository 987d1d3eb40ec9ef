"""FP8 (float8_e4m3fn / float8_e5m2) reductions without a GPU.

* the host-side kernel API for the two dtypes (tests/native/fp8_plan_check.cpp, ASan + UBSan): element
  size, supported ops, and the IPC launch plan of an FP8 reduction against the int8 one of the same
  bytes;
* CPU tensors through the shm transport at world 2 and 4: all_reduce (five ops), reduce,
  reduce_scatter_tensor against the fp32 CPU fold rounded once by torch's CPU cast -- exact values,
  NaN and overflow positions included (tests/_workers_fp8.py).
"""
import os
import shutil
import subprocess

import pytest

from pytorch_distributed_collective_communication_amd.parallel.spawn import launch
from tests import _workers_fp8 as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
BUILD = os.path.join(ROOT, "build", "san")
SRC = os.path.join(ROOT, "tests", "native", "fp8_plan_check.cpp")
HDRS = [os.path.join(CSRC, "kernels", h) for h in ("ipc_plan.h", "kernel_api.h")]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _build() -> str:
    exe = os.path.join(BUILD, "fp8_plan_check")
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
def test_fp8_dtypes_in_the_kernel_api_and_the_launch_plan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1000, r.stdout[-2000:]


def test_cpu_cast_is_the_documented_rounding():
    # the reference of every FP8 test: nearest even, subnormals kept, no saturation
    import torch

    e4, e5 = torch.float8_e4m3fn, torch.float8_e5m2
    f = lambda v, dt: torch.tensor([v], dtype=torch.float32).to(dt).float().item()  # noqa: E731
    assert f(464.0, e4) == 448.0
    assert all(torch.tensor([v]).to(e4).float().isnan().item() for v in (465.0, 1e6, float("inf"), -float("inf")))
    assert f(2.0 ** -10, e4) == 0.0 and f(2.0 ** -9, e4) == 2.0 ** -9
    assert f(61440.0, e5) == float("inf") and f(61439.0, e5) == 57344.0
    assert f(2.0 ** -17, e5) == 0.0 and f(2.0 ** -16, e5) == 2.0 ** -16


@pytest.mark.parametrize("world", [2, 4])
def test_cpu_tensors_through_the_shm_transport(world):
    res = launch(F.cpu_reductions, world, args=("cpu",))
    for r, got in enumerate(res):
        bad = {k: v for k, v in got.items() if not v[0]}
        assert not bad, (r, bad)
        # 2 dtypes x 2 sizes x (5 all_reduce + reduce + reduce_scatter), 2 BXOR, 2 afterwards
        assert len(got) == 2 * 2 * 7 + 4, sorted(got)
