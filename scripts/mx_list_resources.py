"""Registers, scratch and LDS of the tensor-list kernels (csrc/kernels/mx_wire.hip), from the compiler.

Compiles mx_wire.hip for gfx950 with ``-Rpass-analysis=kernel-resource-usage`` (no GPU needed) and writes one line
per instantiation of ``k_mx_quantize_list`` / ``k_mx_dequantize_list`` to profiles/mx/mx_list_resources.txt. Exits
non-zero if one of them uses scratch memory. Their LDS is the descriptor table.

``--against REV`` compiles the kernel sources of the git revision REV the same way and compares every instantiation
of ``k_mx_quantize`` / ``k_mx_dequantize`` / ``k_mx_reduce`` / ``k_mx_fold`` the two builds share. The file then ends
with the number of kernels whose SGPR / VGPR / AGPR / scratch / LDS numbers differ, and the script exits non-zero if
any does.

    python scripts/mx_list_resources.py [--against HEAD~1] [--out profiles/mx/mx_list_resources.txt]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mx6_resources import DT, ROOT, SAME, resources  # noqa: E402
from mx_rot_resources import D, F, FMT, table  # noqa: E402

QUANTIZE = re.compile(r"k_mx_quantize_list" + F + D + r"Lb(\d)ELb(\d)ELb(\d)EE")
DEQUANTIZE = re.compile(r"k_mx_dequantize_list" + F + D + r"Lb(\d)EE")


def describe(name):
    m = QUANTIZE.search(name)
    if m:
        f, t, ef, sr, rot = m.groups()
        kind = "ef" if ef == "1" else ("sr" if sr == "1" else "plain")
        return f"{FMT.get(f, f)} quantize list {DT.get(t, t)} {kind}{' rot' if rot == '1' else ''}"
    m = DEQUANTIZE.search(name)
    if m:
        f, t, rot = m.groups()
        return f"{FMT.get(f, f)} dequantize list {DT.get(t, t)}{' rot' if rot == '1' else ''}"
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx", "mx_list_resources.txt"))
    ap.add_argument("--against", default=None, metavar="REV", help="git revision whose kernels to compare")
    a = ap.parse_args()
    kernels = resources(os.path.join(ROOT, "csrc"))
    rows = sorted((describe(n), k) for n, k in kernels.items() if describe(n))
    bad = [what for what, k in rows if k.get("scratch", 0)]
    differ, shared = [], 0
    if a.against:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.against], capture_output=True, text=True,
                             check=True).stdout.strip()
        with tempfile.TemporaryDirectory() as tmp:
            tar = subprocess.run(["git", "-C", ROOT, "archive", a.against, "csrc/kernels"], capture_output=True, check=True)
            subprocess.run(["tar", "-x", "-C", tmp], input=tar.stdout, check=True)
            before = table(resources(os.path.join(tmp, "csrc")))
        now = table(kernels)
        for what, k in sorted(before.items()):
            shared += 1
            if what not in now or any(now[what].get(f) != k.get(f) for f in SAME):
                differ.append((what, k, now.get(what)))
    with open(a.out, "w") as f:
        f.write("# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, csrc/kernels/mx_wire.hip\n")
        f.write("# (scripts/mx_list_resources.py; compiler output, not a measurement): every instantiation of the\n")
        f.write("# tensor-list kernels. scratch in bytes per lane; lds in bytes per block (the descriptor table);\n")
        f.write("# occupancy in waves per SIMD.\n")
        f.write(f"{'kernel':<40} {'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'scratch':>8} {'lds':>5} {'occupancy':>9}\n")
        for what, k in rows:
            f.write(f"{what:<40} {k.get('vgpr', -1):>5} {k.get('agpr', -1):>5} {k.get('sgpr', -1):>5} "
                    f"{k.get('scratch', -1):>8} {k.get('lds', -1):>5} {k.get('occupancy', -1):>9}\n")
        f.write(f"# {len(rows)} list instantiations, {len(bad)} of them with scratch\n")
        if a.against:
            f.write(f"# against the kernels of commit {rev}: {shared} older instantiations compared, {len(differ)} differ in "
                    f"sgpr / vgpr / agpr / scratch / lds\n")
            for what, was, is_ in differ:
                f.write(f"#   {what}: was {was}, is {is_}\n")
    print(f"{a.out}: {len(rows)} list kernels, {len(bad)} use scratch; {shared} older kernels compared, {len(differ)} differ")
    if bad:
        sys.exit("scratch in: " + ", ".join(bad))
    if differ:
        sys.exit(f"{len(differ)} older instantiations changed")


if __name__ == "__main__":
    main()
