"""Device-code diff of two builds of libvbc's objects (gfx950, no GPU needed).

    python tools/isa_diff.py PARENT_BUILD_DIR BRANCH_BUILD_DIR

Every object with a .hip_fatbin section is disassembled as tools/isa_check.py disassemble() does it and split at the
kernel symbols.  Kernels pair by mangled name over the whole library, so a kernel that moved to another object still
pairs; a kernel is compared on its instruction text (mnemonics and operands), with encodings, addresses, symbol names
in branch targets and objdump's "..." padding marks stripped.  Prints the per-unit table, the kernel sets that differ
and the kernels that differ; exits 1 when a kernel differs or the library's kernel sets are not equal.
"""
import glob
import os
import re
import shutil
import subprocess
import sys

from isa_check import LLVM, disassemble

SYM = re.compile(r"^[0-9A-Fa-f]+ <(.+)>:$")


def kernels(obj):
    """{mangled kernel name: instruction text} of one object ({} when it holds no device code)."""
    with open(obj, "rb") as f:
        if b".hip_fatbin" not in f.read():
            return {}
    out, cur = {}, None
    for line in disassemble(obj):
        m = SYM.match(line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        t = line.split("//", 1)[0].strip()
        if cur is None or not t or t == "..." or t.startswith("Disassembly of"):
            continue
        cur.append(re.sub(r"\s+", " ", t))
    return out


def build(d):
    """{object name: kernels(object)} of the objects of a build directory that hold kernels."""
    units = {os.path.basename(o): kernels(o) for o in sorted(glob.glob(os.path.join(d, "*.o")))}
    return {u: k for u, k in units.items() if k}


def demangle(names):
    tool = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")
    if not names or not tool:
        return list(names)
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
    return r.stdout.splitlines()


def main(parent_dir, branch_dir):
    parent, branch = build(parent_dir), build(branch_dir)
    where = lambda b: {k: u for u, ks in b.items() for k in ks}  # noqa: E731
    text = lambda b: {k: t for ks in b.values() for k, t in ks.items()}  # noqa: E731
    pw, bw, pt, bt = where(parent), where(branch), text(parent), text(branch)
    differ = sorted(k for k in pt if k in bt and pt[k] != bt[k])
    print("unit  kernels(parent)  kernels(branch)  identical  differ")
    for u in sorted(set(parent) | set(branch)):
        mine = branch.get(u, {})
        same = sum(1 for k, t in mine.items() if pt.get(k) == t)
        print(f"{u}  {len(parent.get(u, {}))}  {len(mine)}  {same}  {sum(1 for k in mine if k in pt) - same}")
    same = sum(1 for k in pt if bt.get(k) == pt[k])
    print(f"TOTAL parent kernels {len(pt)}, branch kernels {len(bt)}, identical {same}, differ {len(differ)}")
    print(f"only in parent: {len(set(pt) - set(bt))}, only in branch: {len(set(bt) - set(pt))}")
    for k in demangle(sorted(set(pt) - set(bt))):
        print(f"  - {k}")
    for k in demangle(sorted(set(bt) - set(pt))):
        print(f"  + {k}")
    moved = sorted(k for k in pt if k in bw and pw[k] != bw[k])
    print(f"\nkernels that moved to another unit: {len(moved)}")
    for (src, dst), n in sorted(_count((pw[k], bw[k]) for k in moved).items()):
        print(f"  {src} -> {dst}: {n}")
    for k, name in zip(moved, demangle(moved)):
        print(f"    {pw[k]} -> {bw[k]}  {name}")
    print("\nkernels that differ: " + ("none" if not differ else ""))
    for k in demangle(differ):
        print(f"  {k}")
    return 1 if differ or set(pt) != set(bt) else 0


def _count(items):
    out = {}
    for i in items:
        out[i] = out.get(i, 0) + 1
    return out


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
