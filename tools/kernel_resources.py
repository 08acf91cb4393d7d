#!/usr/bin/env python3
"""Registers, scratch, LDS and code bytes of the kernels in liberl_hip.so whose (demangled) name contains a pattern, read from the gfx950
code objects' metadata notes and symbol tables; with --hash also a digest of each kernel's machine code (to tell whether a kernel
came out unchanged between two builds of the library), with --spills also the compiler's counts of spilled scalar and vector registers.
    python tools/kernel_resources.py PATTERN [lib] [--hash] [--spills]"""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF, CXXFILT = "/opt/rocm/lib/llvm/bin/llvm-readelf", "c++filt"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def demangle(names):
    return subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    pattern = args[0] if args else "rollout"
    lib = args[1] if len(args) > 1 else os.path.join(ROOT, "elegantrl_amd", "lib", "liberl_hip.so")
    want_hash = "--hash" in sys.argv
    want_spills = "--spills" in sys.argv
    data = open(lib, "rb").read()




    rows = []
    pos = data.find(MAGIC)
    with tempfile.TemporaryDirectory() as tmp:
        n = 0
        while pos >= 0:
            (cnt,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
            q = pos + len(MAGIC) + 8
            for _ in range(cnt):
                off, size, tl = struct.unpack_from("<QQQ", data, q)
                triple = data[q + 24:q + 24 + tl].decode()
                q += 24 + tl
                if "gfx950" not in triple or not size:
                    continue
                f = os.path.join(tmp, f"co{n}.elf")
                n += 1
                blob = data[pos + off:pos + off + size]
                open(f, "wb").write(blob)
                notes = subprocess.run([READELF, "--notes", f], capture_output=True, text=True).stdout
                meta = {}
                for block in notes.split("  - .agpr_count:")[1:]:
                    block = ".agpr_count:" + block
                    kv = dict(re.findall(r"\.(\w+):\s+'?([^\s']+)'?", block))
                    if "name" in kv:
                        meta[kv["name"]] = kv
                text_addr = text_off = None
                for ln in subprocess.run([READELF, "-SW", f], capture_output=True, text=True).stdout.splitlines():
                    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", ln)
                    if m:
                        text_addr, text_off = int(m.group(1), 16), int(m.group(2), 16)
                for ln in subprocess.run([READELF, "-sW", f], capture_output=True, text=True).stdout.splitlines():
                    p = ln.split()
                    if len(p) >= 8 and p[3] == "FUNC" and p[7] in meta:
                        kv, addr, sz = meta[p[7]], int(p[1], 16), int(p[2])
                        digest = ""
                        if want_hash and text_addr is not None:
                            start = text_off + addr - text_addr
                            digest = hashlib.sha1(blob[start:start + sz]).hexdigest()[:12]
                        rows.append((p[7], int(kv.get("vgpr_count", -1)), int(kv.get("agpr_count", -1)), int(kv.get("sgpr_count", -1)),
                                     int(kv.get("private_segment_fixed_size", -1)), int(kv.get("group_segment_fixed_size", -1)), sz, digest,
                                     int(kv.get("sgpr_spill_count", -1)), int(kv.get("vgpr_spill_count", -1))))
            pos = data.find(MAGIC, pos + len(MAGIC))
    names = demangle([r[0] for r in rows])
    spill_head = f"{'s_spl':>6}{'v_spl':>6}" if want_spills else ""
    print(f"{'vgpr':>5}{'agpr':>5}{'sgpr':>5}{'scratch':>8}{'lds':>7}{'code':>8}{spill_head}  kernel")
    for r, name in sorted(set(zip(rows, names)), key=lambda x: x[1]):
        name = name.replace("(anonymous namespace)::", "")
        if pattern in name:
            spills = f"{r[8]:6d}{r[9]:6d}" if want_spills else ""
            print(f"{r[1]:5d}{r[2]:5d}{r[3]:5d}{r[4]:8d}{r[5]:7d}{r[6]:8d}{spills}  {name[:110]}" + (f"  {r[7]}" if r[7] else ""))


if __name__ == "__main__":
    main()
