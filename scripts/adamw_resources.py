"""Registers, scratch and LDS of the fused AdamW kernels (csrc/kernels/adamw.hip, adamw8.hip), from the compiler.

Compiles adamw.hip for gfx950 with ``-Rpass-analysis=kernel-resource-usage`` (no GPU needed) and writes one line per
instantiation of ``k_adamw`` to profiles/zero/adamw_resources.txt. Exits non-zero if one of them uses scratch memory
or LDS. ``--state8`` does the same for ``k_adamw8`` of adamw8.hip (the 8-bit state), writes
profiles/zero/adamw8_resources.txt, and also exits non-zero if an instantiation of ``k_adamw`` no longer has the
registers recorded in profiles/zero/adamw_resources.txt.

    python scripts/adamw_resources.py [--state8] [--out FILE]
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

# (the instantiations without a parameter wire, WF = -1; the others: scripts/adamw_wire_resources.py)
KERNEL = re.compile(r"k_adamw8?ILNS\w+?5DTypeE(\d)ELS\w+?_(\d)ELb(\d)ELb(\d)ELin1EE")


def resources(hipcc, name):
    """{instantiation: {field: value}} of csrc/kernels/`name`.hip."""
    csrc = os.path.join(ROOT, "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I" + csrc,
                            "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "kernels", name + ".hip"),
                            "-o", os.path.join(tmp, name + ".o")], capture_output=True, text=True)
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
                cur = rows.setdefault(f"{name} {DT.get(g, g)} grad {out}{'' if vec == '1' else ' element-path'}", {})
            continue
        for label, key in FIELDS:
            m = re.search(re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def table(rows):
    yield f"{'kernel':<44} {'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'scratch':>8} {'lds':>5} {'occupancy':>9}\n"
    for what, k in sorted(rows.items()):
        yield (f"{what:<44} {k.get('vgpr', -1):>5} {k.get('agpr', -1):>5} {k.get('sgpr', -1):>5} "
               f"{k.get('scratch', -1):>8} {k.get('lds', -1):>5} {k.get('occupancy', -1):>9}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--state8", action="store_true", help="adamw8.hip, and k_adamw against its recorded table")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = "adamw8" if a.state8 else "adamw"
    recorded = os.path.join(ROOT, "profiles", "zero", "adamw_resources.txt")
    a.out = a.out or os.path.join(ROOT, "profiles", "zero", name + "_resources.txt")
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    rows = resources(hipcc, name)
    bad = [what for what, k in rows.items() if k.get("scratch", 0) or k.get("lds", 0)]
    moved = []
    if a.state8:  # the f32-state kernels: the same lines as recorded
        with open(recorded) as f:
            old = {line for line in f if line.startswith("adamw ")}
        moved = sorted(set(list(table(resources(hipcc, "adamw")))[1:]) ^ old)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, csrc/kernels/{name}.hip\n")
        f.write(f"# (scripts/adamw_resources.py; compiler output, not a measurement): every instantiation of k_{name}.\n")
        f.write("# scratch in bytes per lane; lds in bytes per block; occupancy in waves per SIMD.\n")
        f.writelines(table(rows))
        f.write(f"# {len(rows)} instantiations, {len(bad)} of them with scratch or LDS\n")
        if a.state8:
            f.write(f"# k_adamw (adamw.hip) compiled next to it: {len(moved)} lines differ from adamw_resources.txt\n")
    print(f"{a.out}: {len(rows)} kernels, {len(bad)} use scratch or LDS, {len(moved)} k_adamw lines moved")
    if bad or not rows or moved:
        sys.exit("scratch or LDS in: " + ", ".join(bad) if bad else
                 "k_adamw moved:\n" + "".join(moved) if moved else f"no k_{name} instantiation found")


if __name__ == "__main__":
    main()
