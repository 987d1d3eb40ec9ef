"""One-off: compare every gfx950 kernel of two builds of the extension, instruction for instruction.

    python profiles/refactor_ipc_plan/compare_isa.py PARENT_SO NEW_SO > profiles/refactor_ipc_plan/isa_compare.txt

Per kernel family: how many instantiations are the same in both builds (instructions and the code-object
metadata: VGPRs, SGPRs, private and group segment bytes). A kernel that is not gets a line of its own with
both builds' counts (--all: every kernel does). Disassembly as tests/test_isa_memory_model.py does it.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.test_isa_memory_model import LLVM, _code_objects  # noqa: E402

META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def load(so):
    funcs, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, co in enumerate(_code_objects(so, tmp)):
            path = os.path.join(tmp, f"co{k}.elf")
            open(path, "wb").write(co)
            txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", path], check=True,
                                 capture_output=True, text=True).stdout
            name = None
            for line in txt.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
                if m:
                    name = m.group(1)
                    funcs[name] = []
                elif name and line.startswith("\t"):
                    funcs[name].append(line.split("//")[0].strip())
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], check=True,
                                   capture_output=True, text=True).stdout
            cur = {}
            for line in notes.splitlines():  # kernel-level keys sit at column 4, a kernel's first after "  - "
                m = re.match(r"^  (?:- |  )(\.\w+):\s+(\S+)", line)
                if not m:
                    continue
                if line.startswith("  - "):
                    cur = {}
                if m.group(1) == ".name":
                    meta[m.group(2)] = cur
                elif m.group(1) in META:
                    cur[m.group(1)] = int(m.group(2))
    return funcs, meta


def main():
    every = "--all" in sys.argv  # one line per kernel; by default only the kernels that are not the same
    (pf, pm), (nf, nm) = [load(p) for p in sys.argv[1:] if p != "--all"]
    kern = sorted(n for n in set(pf) | set(nf) if re.search(r"k_ipc_|k_ll_|k1_|k2_", n))
    fams = {}
    for n in kern:
        fam = re.search(r"(k_ipc_[a-z]+|k_ll_[a-z_]+|k1_[a-z_]+|k2_[a-z_]+)I", n).group(1)
        if n not in pf or n not in nf:
            state = "ONLY_IN_" + ("PARENT" if n in pf else "NEW")
        else:
            state = "same" if pf[n] == nf[n] and pm.get(n) == nm.get(n) else "DIFFERS"
        a, b = pm.get(n, {}), nm.get(n, {})
        f = fams.setdefault(fam, {"n": 0, "same": 0, "insns": [], "vgpr": [], "sgpr": [], "private": [], "group": []})
        f["n"] += 1
        f["same"] += state == "same"
        f["insns"].append(len(nf.get(n, [])))
        for k, key in zip(("vgpr", "sgpr", "private", "group"), META):
            f[k].append(b.get(key, -1))
        if every or state != "same":
            print(f"{state:8s} insns {len(pf.get(n, []))}->{len(nf.get(n, []))} "
                  + " ".join(f"{k[1:].split('_')[0]} {a.get(k)}->{b.get(k)}" for k in META)
                  + "  " + re.sub(r"^_ZN4pdcc3dev\\d+", "", n).split("EvNS", 1)[0])
    print("# family: instantiations, of them same as the parent (instructions and metadata); ranges over the family")
    for fam, f in sorted(fams.items()):
        rng = " ".join(f"{k} {min(f[k])}..{max(f[k])}" for k in ("insns", "vgpr", "sgpr", "private", "group"))
        print(f"{fam}: {f['n']} instantiations, {f['same']} same; {rng}")


if __name__ == "__main__":
    main()
