"""Registers and scratch of the stochastic-rounding kernels (csrc/kernels/mx_wire.hip), from the compiler.

Compiles mx_wire.hip for gfx950 with ``-Rpass-analysis=kernel-resource-usage`` (no GPU needed) and
writes one line per instantiation of ``k_mx_quantize`` / ``k_mx_reduce`` -- the stochastic-rounding
ones and, for comparison, the plain ones -- to profiles/mx/mx_sr_resources.txt, with the LDS bytes of
each. Exits non-zero if a stochastic-rounding instantiation uses scratch memory or LDS.

    python scripts/mx_sr_resources.py [--out profiles/mx/mx_sr_resources.txt]
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
FMT = {"0": "mxfp8_e4m3", "1": "mxfp4_e2m1"}
DT = {"0": "f32", "1": "f16", "2": "bf16"}  # kern::DType
# the template arguments, read from the mangled names
QUANTIZE = re.compile(r"k_mx_quantizeILNS\w+?8MxFormatE(\d)ELNS\w+?5DTypeE(\d+)ELb(\d)ELb(\d)ELb(\d)ELb(\d)EE")
REDUCE = re.compile(r"k_mx_reduceILNS\w+?8MxFormatE(\d)ELi(\d+)ELb(\d)ELb(\d)ELb(\d)EE")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx", "mx_sr_resources.txt"))
    a = ap.parse_args()
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I" + os.path.join(ROOT, "csrc"),
               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "csrc", "kernels", "mx_wire.hip"),
               "-o", os.path.join(tmp, "mx_wire.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stdout + r.stderr)
    kernels, cur = [], None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            kernels.append(cur)
            continue
        for label, key in FIELDS:
            m = re.search(re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    rows, bad = [], []
    for k in kernels:
        m = QUANTIZE.search(k["name"])
        if m:
            f, t, shard, vec, ef, sr = m.groups()
            what = f"quantize {FMT[f]} {DT.get(t, t)} {'shard' if shard == '1' else 'dealt'}" \
                   f"{'' if vec == '1' else ' element-path'}"
        else:
            m = REDUCE.search(k["name"])
            if not m:
                continue
            f, n, avg, ef, sr = m.groups()
            what = f"reduce {FMT[f]} nsrc={n} {'avg' if avg == '1' else 'sum'}"
        if ef == "1":  # the error-feedback instantiations: scripts/mx_ef_resources.py
            continue
        ef = sr == "1"
        rows.append((what, ef, k))
        if ef and (k.get("scratch", 0) or k.get("lds", 0)):
            bad.append(what)
    rows.sort(key=lambda r: (r[0].split()[0], r[0], r[1]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, csrc/kernels/mx_wire.hip\n")
        f.write("# (scripts/mx_sr_resources.py; compiler output, not a measurement). sr = the stochastic-rounding\n")
        f.write("# instantiation; scratch in bytes per lane; lds in bytes per block; occupancy in waves per SIMD.\n")
        f.write(f"{'kernel':<52} {'sr':>8} {'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'scratch':>8} {'lds':>5} {'occupancy':>9}\n")
        for what, ef, k in rows:
            f.write(f"{what:<52} {'yes' if ef else 'no':>8} {k.get('vgpr', -1):>5} {k.get('agpr', -1):>5} "
                    f"{k.get('sgpr', -1):>5} {k.get('scratch', -1):>8} {k.get('lds', -1):>5} {k.get('occupancy', -1):>9}\n")
        n_ef = sum(ef for _, ef, _ in rows)
        f.write(f"# {n_ef} stochastic-rounding instantiations, {len(bad)} of them with scratch or LDS\n")
    print(f"{a.out}: {len(rows)} kernels, {n_ef} stochastic, {len(bad)} of those use scratch or LDS")
    if bad:
        sys.exit("scratch or LDS in: " + ", ".join(bad))


if __name__ == "__main__":
    main()
