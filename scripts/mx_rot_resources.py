"""Registers, scratch and LDS of the Hadamard-rotated kernels (csrc/kernels/mx_wire.hip), from the compiler.

Compiles mx_wire.hip for gfx950 with ``-Rpass-analysis=kernel-resource-usage`` (no GPU needed) and writes one
line per rotated instantiation of ``k_mx_quantize`` / ``k_mx_dequantize`` / ``k_mx_fold`` next to its plain twin
to profiles/mx/mx_rot_resources.txt. Exits non-zero if a rotated instantiation uses scratch memory or LDS.

``--against REV`` compiles the kernel sources of the git revision REV the same way and compares every
instantiation the two builds share: REV's kernels have no rotation flag, so each is matched with the
instantiation of this tree whose flag is off (``k_mx_reduce`` has none in either). The file then ends with the
number of kernels whose SGPR / VGPR / AGPR / scratch / LDS numbers differ, and the script exits non-zero if
any does.

    python scripts/mx_rot_resources.py [--against HEAD~1] [--out profiles/mx/mx_rot_resources.txt]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mx6_resources import DT, ROOT, SAME, resources  # noqa: E402

FMT = {"0": "fp8", "1": "fp4", "2": "fp6"}  # kern::MxFormat
F, D = r"ILNS\w+?8MxFormatE(\d)E", r"LNS\w+?5DTypeE(\d+)E"
QUANTIZE = re.compile(r"k_mx_quantize" + F + D + r"Lb(\d)ELb(\d)ELb(\d)ELb(\d)E(?:Lb(\d)E)?E")
DEQUANTIZE = re.compile(r"k_mx_dequantize" + F + D + r"Lb(\d)ELb(\d)E(?:Lb(\d)E)?E")
REDUCE = re.compile(r"k_mx_reduce" + F + r"Li(\d+)ELb(\d)ELb(\d)ELb(\d)EE")
FOLD = re.compile(r"k_mx_fold" + F + D + r"Li(\d+)ELb(\d)E(?:Lb(\d)E)?E")


def describe(name):
    """(readable name without the rotation flag, rotated?) of an mx kernel, None for anything else."""
    m = QUANTIZE.search(name)
    if m:
        f, t, shard, vec, ef, sr, rot = m.groups()
        kind = "ef" if ef == "1" else ("sr" if sr == "1" else "plain")
        return (f"{FMT.get(f, f)} quantize {DT.get(t, t)} {'shard' if shard == '1' else 'dealt'}"
                f"{'' if vec == '1' else ' element-path'} {kind}"), rot == "1"
    m = DEQUANTIZE.search(name)
    if m:
        f, t, shard, vec, rot = m.groups()
        return (f"{FMT.get(f, f)} dequantize {DT.get(t, t)} {'shard' if shard == '1' else 'dealt'}"
                f"{'' if vec == '1' else ' element-path'}"), rot == "1"
    m = REDUCE.search(name)
    if m:
        f, n, avg, ef, sr = m.groups()
        kind = "ef" if ef == "1" else ("sr" if sr == "1" else "plain")
        return f"{FMT.get(f, f)} reduce nsrc={n} {'avg' if avg == '1' else 'sum'} {kind}", False
    m = FOLD.search(name)
    if m:
        f, t, n, avg, rot = m.groups()
        return f"{FMT.get(f, f)} fold {DT.get(t, t)} nsrc={n} {'avg' if avg == '1' else 'sum'}", rot == "1"
    return None


def table(kernels):
    """{(readable name, rotated?): numbers}"""
    out = {}
    for name, k in kernels.items():
        d = describe(name)
        if d is not None:
            assert d not in out, d
            out[d] = k
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx", "mx_rot_resources.txt"))
    ap.add_argument("--against", default=None, metavar="REV", help="git revision whose kernels to compare")
    a = ap.parse_args()
    now = table(resources(os.path.join(ROOT, "csrc")))
    rows = sorted((what, k, now.get((what, False))) for (what, rot), k in now.items() if rot)
    bad = [what for what, k, _ in rows if k.get("scratch", 0) or k.get("lds", 0)]
    differ, shared = [], 0
    if a.against:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.against], capture_output=True, text=True,
                             check=True).stdout.strip()
        with tempfile.TemporaryDirectory() as tmp:
            tar = subprocess.run(["git", "-C", ROOT, "archive", a.against, "csrc/kernels"], capture_output=True, check=True)
            subprocess.run(["tar", "-x", "-C", tmp], input=tar.stdout, check=True)
            before = table(resources(os.path.join(tmp, "csrc")))
        for (what, rot), k in sorted(before.items()):
            if rot:
                continue
            shared += 1
            is_ = now.get((what, False))
            if is_ is None or any(is_.get(f) != k.get(f) for f in SAME):
                differ.append((what, k, is_))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def cols(k):
        return (f"{k.get('vgpr', -1):>5} {k.get('agpr', -1):>5} {k.get('sgpr', -1):>5} {k.get('scratch', -1):>8} "
                f"{k.get('lds', -1):>5} {k.get('occupancy', -1):>9}")

    with open(a.out, "w") as f:
        f.write("# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, csrc/kernels/mx_wire.hip\n")
        f.write("# (scripts/mx_rot_resources.py; compiler output, not a measurement): every instantiation with the\n")
        f.write("# Hadamard rotation, and under it (=) its twin without. scratch in bytes per lane; lds in bytes per\n")
        f.write("# block; occupancy in waves per SIMD.\n")
        f.write(f"{'kernel':<48} {'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'scratch':>8} {'lds':>5} {'occupancy':>9}\n")
        for what, k, plain in rows:
            f.write(f"{what + ' rot':<48} {cols(k)}\n")
            if plain is not None:
                f.write(f"{'  = without':<48} {cols(plain)}\n")
        more = sum(1 for _, k, p in rows if p is not None and k.get("vgpr", 0) > p.get("vgpr", 0))
        drop = sum(1 for _, k, p in rows if p is not None and k.get("occupancy", 0) < p.get("occupancy", 0))
        f.write(f"# {len(rows)} rotated instantiations, {len(bad)} of them with scratch or LDS; {more} use more VGPRs "
                f"than their twin, {drop} have a lower occupancy\n")
        if a.against:
            f.write(f"# against the kernels of commit {rev}: {shared} instantiations compared with their twin whose rotation "
                    f"flag is off, {len(differ)} differ in sgpr / vgpr / agpr / scratch / lds\n")
            for what, was, is_ in differ:
                f.write(f"#   {what}: was {was}, is {is_}\n")
    print(f"{a.out}: {len(rows)} rotated kernels, {len(bad)} use scratch or LDS; {shared} older kernels compared, "
          f"{len(differ)} differ")
    if bad:
        sys.exit("scratch or LDS in: " + ", ".join(bad))
    if differ:
        sys.exit(f"{len(differ)} instantiations without the rotation changed")


if __name__ == "__main__":
    main()
