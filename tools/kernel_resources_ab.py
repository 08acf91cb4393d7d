#!/usr/bin/env python3
"""Two builds of liberl_hip.so side by side: registers, scratch, spills and occupancy of every kernel whose (demangled) name contains one
of the patterns (tools/kernel_resources.py --spills --hash on each build), with a verdict per kernel -- scratch gained, occupancy lost
(waves per SIMD that the vector registers allow: min(8, 512 / vgpr rounded up to 8)), scalar-register spills where there were none;
"same code" when the kernel's machine code did not change.  Kernels of the second build that the first does not have are listed last.
How profiles/criterion_kernel_resources.txt was made.
    python tools/kernel_resources_ab.py PARENT_LIB TREE_LIB PATTERN [PATTERN ...]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_resources.py")


def occupancy(vgpr):
    return min(8, 512 // max(8, (vgpr + 7) // 8 * 8))


def kernels(lib, patterns):
    """{kernel name as tools/kernel_resources.py prints it: (vgpr, agpr, sgpr, scratch, lds, code bytes, sgpr spills, vgpr spills, code digest)}"""
    out = {}
    for pattern in patterns:
        listing = subprocess.run([sys.executable, TOOL, pattern, lib, "--spills", "--hash"], capture_output=True, text=True, check=True).stdout
        for line in listing.splitlines()[1:]:
            fields = line.split(None, 8)
            name, digest = fields[8].rsplit("  ", 1)
            key, n = name.strip(), 1
            while key in out and out[key][8] != digest:          # the same (truncated) name in two translation units: keep both, in listing order
                n += 1
                key = f"{name.strip()} #{n}"
            out[key] = tuple(int(x) for x in fields[:8]) + (digest,)
    return out


def same_kernel(name, parent, tree, matched):
    """the tree's entry for a parent kernel: the same name -- among the copies that several translation units hold under one name, the one
    with the same machine code if there is one --, or the name with `, false` appended (a template parameter added with a default shows)"""
    base = name.split(" #")[0]
    copies = [k for k in tree if k.split(" #")[0] == base and k not in matched]
    if not copies:
        head, sep, tail = base.partition(">(")
        copies = [k for k in tree if sep and k.split(" #")[0] == head + ", false>(" + tail and k not in matched]
    if not copies:                                              # a kernel whose parameter list changed
        copies = [k for k in tree if k.split("(")[0] == base.split("(")[0] and k not in matched]
    same = [k for k in copies if tree[k][8] == parent[name][8]]
    return (same or copies or [None])[0]


def row(r):
    return f"{r[0]:4d} {r[1]:4d} {r[2]:4d} {r[3]:5d} {r[6]:5d} {r[7]:5d} {occupancy(r[0]):2d}"


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    parent, tree = kernels(sys.argv[1], sys.argv[3:]), kernels(sys.argv[2], sys.argv[3:])
    print(f"{'kernel':58}  parent: vgpr agpr sgpr scratch s_spl v_spl occ | tree: vgpr agpr sgpr scratch s_spl v_spl occ | verdict")
    violations, matched = 0, set()
    for name in sorted(parent):
        other = same_kernel(name, parent, tree, matched)
        if other is None:
            print(f"{name[:58]:58}  not in the tree")
            continue
        matched.add(other)
        p, t = parent[name], tree[other]
        broken = [word for word, hit in (("SCRATCH+", t[3] > p[3]), ("OCC-", occupancy(t[0]) < occupancy(p[0])),
                                         ("SGPR-SPILL+", p[6] == 0 and t[6] > 0)) if hit]
        notes = list(broken)
        if t[6] > p[6]:
            notes.append(f"s_spl+{t[6] - p[6]}")
        if t[7] > p[7]:
            notes.append(f"v_spl+{t[7] - p[7]}")
        if t[8] == p[8]:
            notes.append("same code")
        violations += bool(broken)
        print(f"{name[:58]:58}  {row(p)} | {row(t)} | {' '.join(notes) or 'ok'}")
    print("violations:", violations)
    print()
    print("kernels only in the tree:")
    for name in sorted(set(tree) - matched):
        print(f"{name[:58]:58}  {row(tree[name])}")


if __name__ == "__main__":
    main()
