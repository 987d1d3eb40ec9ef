"""Registers, scratch and LDS of the fused AdamW kernels with and without the parameter wire (csrc/kernels/adamw.hip,
adamw8.hip; docs/collectives.md "Parameter wire from the step"), from the compiler.

Compiles both files for gfx950 with ``-Rpass-analysis=kernel-resource-usage`` (no GPU needed) and writes
profiles/zero/adamw_wire_resources.txt: one line per instantiation of ``k_adamw`` and ``k_adamw8``, the ones that emit
a wire named by their format, and next to every instantiation without a wire whether its line is still the one recorded
in profiles/zero/adamw_resources.txt / adamw8_resources.txt (before) or what it was there. Exits non-zero if any
instantiation uses scratch memory or LDS.

    python scripts/adamw_wire_resources.py [--out FILE]
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

KERNEL = re.compile(r"k_adamw8?ILNS\w+?5DTypeE(\d)ELS\w+?_(\d)ELb(\d)ELb(\d)ELi(n?\d)EE")
WIRES = {"0": "mxfp8_e4m3", "1": "mxfp4_e2m1", "2": "mxfp6_e2m3"}
KEYS = ("vgpr", "agpr", "sgpr", "scratch", "lds", "occupancy")


def resources(hipcc, name):
    """{instantiation: {field: value}} of csrc/kernels/`name`.hip; the labels of scripts/adamw_resources.py, with
    "+ <wire>" for the instantiations that emit one (param_out is a run-time choice there)."""
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
                g, p, hasp, vec, wf = k.groups()
                out = f"-> {DT.get(p, p)}" if hasp == "1" else "no param_out"
                what = f"{name} {DT.get(g, g)} grad {out}{'' if vec == '1' else ' element-path'}"
                cur = rows.setdefault(what + (f" + {WIRES[wf]}" if wf in WIRES else ""), {})
            continue
        for label, key in FIELDS:
            m = re.search(re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def recorded(name):
    """{instantiation: [fields]} of profiles/zero/`name`_resources.txt."""
    out = {}
    with open(os.path.join(ROOT, "profiles", "zero", name + "_resources.txt")) as f:
        for line in f:
            if line.startswith(name + " "):
                out[line[:44].rstrip()] = [int(x) for x in line[44:].split()]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zero", "adamw_wire_resources.txt"))
    a = ap.parse_args()
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    rows, before = {}, {}
    for name in ("adamw", "adamw8"):
        rows.update(resources(hipcc, name))
        before.update(recorded(name))
    bad = [what for what, k in rows.items() if k.get("scratch", 0) or k.get("lds", 0)]
    moved = 0
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, csrc/kernels/adamw.hip, adamw8.hip\n")
        f.write("# (scripts/adamw_wire_resources.py; compiler output, not a measurement): every instantiation of k_adamw and\n")
        f.write("# k_adamw8. scratch in bytes per lane; lds in bytes per block; occupancy in waves per SIMD. `before`: the line\n")
        f.write("# of adamw_resources.txt / adamw8_resources.txt for an instantiation without a wire, `=` where it is unchanged.\n")
        f.write(f"{'kernel':<58} {'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'scratch':>8} {'lds':>5} {'occupancy':>9}  before\n")
        for what, k in sorted(rows.items()):
            now = [k.get(key, -1) for key in KEYS]
            old = before.get(what)
            note = "" if old is None else ("=" if old == now else " ".join(map(str, old)))
            moved += note not in ("", "=")
            f.write(f"{what:<58} {now[0]:>5} {now[1]:>5} {now[2]:>5} {now[3]:>8} {now[4]:>5} {now[5]:>9}  {note}\n")
        wired = sum(" + " in what for what in rows)
        f.write(f"# {len(rows)} instantiations, {wired} of them emit a wire, {len(bad)} with scratch or LDS; "
                f"{moved} of the {len(rows) - wired} without a wire differ from their recorded line\n")
    print(f"{a.out}: {len(rows)} kernels, {len(bad)} use scratch or LDS, {moved} lines without a wire moved")
    if bad or not rows:
        sys.exit("scratch or LDS in: " + ", ".join(bad) if bad else "no instantiation found")


if __name__ == "__main__":
    main()
