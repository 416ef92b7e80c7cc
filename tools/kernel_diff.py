"""Kernel-by-kernel comparison of two built trees: every gfx950 kernel of every racinglmpc_amd/*.so of a parent tree against the same kernel of this tree.

    python tools/kernel_diff.py PARENT_TREE NEW_TREE [-o profiles/NAME_kernel_diff.txt]

Both trees built the same way (racinglmpc_amd.build.build_all(force=True)).  Kernels are matched by library and demangled name.  Compared: the instruction text of a
kernel -- mnemonic and operands, in order; branch operands are relative offsets and take part.  Left out: addresses, encodings, the order of the symbols in a code
object and the padding between them (whatever lies behind a symbol's size).  The report gives the identical / different / new / missing counts and the name of every
kernel that is not identical.  Exit status 0 only if no kernel is different, new or missing and the identical count is the parent's total.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from racinglmpc_amd import isa_check                                          # noqa: E402

HEAD = re.compile(r"^([0-9a-fA-F]+)\s+<([^>]+)>:\s*$")
INS = re.compile(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):")
SYM = re.compile(r"^([0-9a-fA-F]+)\s+\S+\s+F\s+\.text\s+([0-9a-fA-F]+)\s+(?:\.\w+\s+)?(\S+)\s*$")


def kernels(text, symtab=None):
    """{mangled name: [instruction text, ...]} of one `llvm-objdump -d` listing.  symtab (`llvm-objdump -t` of the same image): an instruction behind its symbol's
    size is padding and left out; without it every line under a symbol counts."""
    size = {}
    for line in (symtab or "").splitlines():
        m = SYM.match(line)
        if m:
            size[m.group(3)] = (int(m.group(1), 16), int(m.group(2), 16))
    out = {}; cur = None
    for line in text.splitlines():
        m = HEAD.match(line)
        if m:
            cur = m.group(2); out[cur] = []
            continue
        m = INS.match(line)
        if m and cur is not None:
            if cur in size and not size[cur][0] <= int(m.group(2), 16) < sum(size[cur]):
                continue
            out[cur].append(" ".join(m.group(1).split()))
    return out


def compare(parent, new):
    """Two {name: instructions} maps -> (identical, different, new, missing): four sorted lists of names."""
    same = sorted(k for k in parent if k in new and parent[k] == new[k])
    diff = sorted(k for k in parent if k in new and parent[k] != new[k])
    return same, diff, sorted(k for k in new if k not in parent), sorted(k for k in parent if k not in new)


def accepted(same, diff, added, missing, parent_total):
    return not diff and not added and not missing and len(same) == parent_total > 0            # (nothing parsed is not "all identical")


def demangle(names):
    if not names:
        return []
    return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()


def library_kernels(path):
    """{demangled name: instructions} over every code object of one shared library."""
    out = {}
    for _, image in isa_check.code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(image); f.flush()
            symtab = subprocess.run([isa_check.OBJDUMP, "-t", f.name], capture_output=True, text=True, check=True).stdout
        k = kernels(isa_check.disassemble(image), symtab)
        out.update(zip(demangle(list(k)), k.values()))
    return out


def tree_kernels(tree):
    out = {}
    for so in sorted(glob.glob(os.path.join(tree, "racinglmpc_amd", "*.so"))):
        for name, ins in library_kernels(so).items():
            out["%s: %s" % (os.path.basename(so), name)] = ins
    return out


def report(parent, new):
    same, diff, added, missing = compare(parent, new)
    lines = ["total: %d kernels in the parent's build, %d in this one: %d identical, %d different, %d new, %d missing" % (len(parent), len(new), len(same), len(diff), len(added), len(missing))]
    for title, names in (("different", diff), ("new", added), ("missing", missing)):
        lines += ["%s: %s" % (title, k) for k in names]
    per_lib = {}
    for k in parent:
        per_lib.setdefault(k.split(": ")[0], [0, 0])[0] += 1
    for k in same:
        per_lib[k.split(": ")[0]][1] += 1
    lines += ["  %-28s %4d kernels, %4d identical" % (lib, n, s) for lib, (n, s) in sorted(per_lib.items())]
    return lines, accepted(same, diff, added, missing, len(parent))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent"); ap.add_argument("new"); ap.add_argument("-o", "--out")
    a = ap.parse_args()
    lines, ok = report(tree_kernels(a.parent), tree_kernels(a.new))
    lines.append("accepted" if ok else "NOT accepted: a kernel is different, new or missing, or the identical count is not the parent's total")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
