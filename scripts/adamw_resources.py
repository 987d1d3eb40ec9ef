"""Registers, scratch and LDS of the fused AdamW kernels (csrc/kernels/adamw.hip), from the compiler.

Compiles adamw.hip for gfx950 with ``-Rpass-analysis=kernel-resource-usage`` (no GPU needed) and writes one line per
instantiation of ``k_adamw`` to profiles/zero/adamw_resources.txt. Exits non-zero if one of them uses scratch memory
or LDS.

    python scripts/adamw_resources.py [--out profiles/zero/adamw_resources.txt]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mx6_resources import DT, FIELDS, ROOT  # noqa: E402

KERNEL = re.compile(r"k_adamwILNS\w+?5DTypeE(\d)ELS\w+?_(\d)ELb(\d)ELb(\d)EE")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zero", "adamw_resources.txt"))
    a = ap.parse_args()
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    csrc = os.path.join(ROOT, "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I" + csrc,
                            "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "kernels", "adamw.hip"),
                            "-o", os.path.join(tmp, "adamw.o")], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stdout + r.stderr)
    rows, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = KERNEL.search(m.group(1))
            cur = None
            if k:
                g, p, hasp, vec = k.groups()
                out = f"-> {DT.get(p, p)}" if hasp == "1" else "no param_out"
                cur = rows.setdefault(f"adamw {DT.get(g, g)} grad {out}{'' if vec == '1' else ' element-path'}", {})
            continue
        for label, key in FIELDS:
            m = re.search(re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    bad = [what for what, k in rows.items() if k.get("scratch", 0) or k.get("lds", 0)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, csrc/kernels/adamw.hip\n")
        f.write("# (scripts/adamw_resources.py; compiler output, not a measurement): every instantiation of k_adamw.\n")
        f.write("# scratch in bytes per lane; lds in bytes per block; occupancy in waves per SIMD.\n")
        f.write(f"{'kernel':<44} {'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'scratch':>8} {'lds':>5} {'occupancy':>9}\n")
        for what, k in sorted(rows.items()):
            f.write(f"{what:<44} {k.get('vgpr', -1):>5} {k.get('agpr', -1):>5} {k.get('sgpr', -1):>5} "
                    f"{k.get('scratch', -1):>8} {k.get('lds', -1):>5} {k.get('occupancy', -1):>9}\n")
        f.write(f"# {len(rows)} instantiations, {len(bad)} of them with scratch or LDS\n")
    print(f"{a.out}: {len(rows)} kernels, {len(bad)} use scratch or LDS")
    if bad or not rows:
        sys.exit("scratch or LDS in: " + ", ".join(bad) if bad else "no k_adamw instantiation found")


if __name__ == "__main__":
    main()
