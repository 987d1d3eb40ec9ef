"""Registers, scratch and LDS of the `mxfp6_e2m3` kernels (csrc/kernels/mx_wire.hip), from the compiler.

Compiles mx_wire.hip for gfx950 with ``-Rpass-analysis=kernel-resource-usage`` (no GPU needed) and writes
one line per FP6 instantiation of ``k_mx_quantize`` / ``k_mx_dequantize`` / ``k_mx_reduce`` / ``k_mx_fold``
to profiles/mx/mx6_resources.txt. Exits non-zero if one of them uses scratch memory or LDS.

``--against REV`` compiles the kernel sources of the git revision REV the same way and compares every
instantiation the two builds share (the FP8 and FP4 ones): the file then ends with the number of kernels
whose SGPR / VGPR / AGPR / scratch / LDS numbers differ, and the script exits non-zero if any does.

    python scripts/mx6_resources.py [--against HEAD~1] [--out profiles/mx/mx6_resources.txt]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (("SGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "lds"))
SAME = ("sgpr", "vgpr", "agpr", "scratch", "lds")
FP6 = "2"  # kern::MxFormat::FP6_E2M3
DT = {"0": "f32", "1": "f16", "2": "bf16"}  # kern::DType
F, D = r"ILNS\w+?8MxFormatE(\d)E", r"LNS\w+?5DTypeE(\d+)E"
QUANTIZE = re.compile(r"k_mx_quantize" + F + D + r"Lb(\d)ELb(\d)ELb(\d)ELb(\d)EE")
DEQUANTIZE = re.compile(r"k_mx_dequantize" + F + D + r"Lb(\d)ELb(\d)EE")
REDUCE = re.compile(r"k_mx_reduce" + F + r"Li(\d+)ELb(\d)ELb(\d)ELb(\d)EE")
FOLD = re.compile(r"k_mx_fold" + F + D + r"Li(\d+)ELb(\d)EE")


def resources(csrc):
    """{mangled kernel name: {field: number}} of csrc/kernels/mx_wire.hip."""
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I" + csrc,
               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "kernels", "mx_wire.hip"),
               "-o", os.path.join(tmp, "mx_wire.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stdout + r.stderr)
    kernels, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return kernels


def describe(name):
    """(format digit, readable name) of an mx kernel, None for anything else."""
    m = QUANTIZE.search(name)
    if m:
        f, t, shard, vec, ef, sr = m.groups()
        kind = "ef" if ef == "1" else ("sr" if sr == "1" else "plain")
        return f, f"quantize {DT.get(t, t)} {'shard' if shard == '1' else 'dealt'}{'' if vec == '1' else ' element-path'} {kind}"
    m = DEQUANTIZE.search(name)
    if m:
        f, t, shard, vec = m.groups()
        return f, f"dequantize {DT.get(t, t)} {'shard' if shard == '1' else 'dealt'}{'' if vec == '1' else ' element-path'}"
    m = REDUCE.search(name)
    if m:
        f, n, avg, ef, sr = m.groups()
        kind = "ef" if ef == "1" else ("sr" if sr == "1" else "plain")
        return f, f"reduce nsrc={n} {'avg' if avg == '1' else 'sum'} {kind}"
    m = FOLD.search(name)
    if m:
        f, t, n, avg = m.groups()
        return f, f"fold {DT.get(t, t)} nsrc={n} {'avg' if avg == '1' else 'sum'}"
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx", "mx6_resources.txt"))
    ap.add_argument("--against", default=None, metavar="REV", help="git revision whose FP8 / FP4 kernels to compare")
    a = ap.parse_args()
    now = resources(os.path.join(ROOT, "csrc"))
    rows = sorted((d[1], k) for d, k in ((describe(n), k) for n, k in now.items()) if d and d[0] == FP6)
    bad = [what for what, k in rows if k.get("scratch", 0) or k.get("lds", 0)]
    differ, shared = [], 0
    if a.against:
        with tempfile.TemporaryDirectory() as tmp:
            tar = subprocess.run(["git", "-C", ROOT, "archive", a.against, "csrc/kernels"], capture_output=True, check=True)
            subprocess.run(["tar", "-x", "-C", tmp], input=tar.stdout, check=True)
            before = resources(os.path.join(tmp, "csrc"))
        for name, k in sorted(before.items()):
            d = describe(name)
            if d is None:
                continue
            shared += 1
            if name not in now or any(now[name].get(f) != k.get(f) for f in SAME):
                differ.append((f"format {d[0]} {d[1]}", k, now.get(name)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, csrc/kernels/mx_wire.hip\n")
        f.write("# (scripts/mx6_resources.py; compiler output, not a measurement): the mxfp6_e2m3 instantiations.\n")
        f.write("# scratch in bytes per lane; lds in bytes per block; occupancy in waves per SIMD.\n")
        f.write(f"{'kernel':<44} {'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'scratch':>8} {'lds':>5} {'occupancy':>9}\n")
        for what, k in rows:
            f.write(f"{what:<44} {k.get('vgpr', -1):>5} {k.get('agpr', -1):>5} {k.get('sgpr', -1):>5} "
                    f"{k.get('scratch', -1):>8} {k.get('lds', -1):>5} {k.get('occupancy', -1):>9}\n")
        f.write(f"# {len(rows)} mxfp6_e2m3 instantiations, {len(bad)} of them with scratch or LDS\n")
        if a.against:
            f.write(f"# against the kernels of {a.against}: {shared} mxfp8_e4m3 / mxfp4_e2m1 instantiations compared, "
                    f"{len(differ)} differ in sgpr / vgpr / agpr / scratch / lds\n")
            for what, was, is_ in differ:
                f.write(f"#   {what}: was {was}, is {is_}\n")
    print(f"{a.out}: {len(rows)} FP6 kernels, {len(bad)} use scratch or LDS; {shared} older kernels compared, {len(differ)} differ")
    if bad:
        sys.exit("scratch or LDS in: " + ", ".join(bad))
    if differ:
        sys.exit(f"{len(differ)} mxfp8_e4m3 / mxfp4_e2m1 instantiations changed")


if __name__ == "__main__":
    main()
