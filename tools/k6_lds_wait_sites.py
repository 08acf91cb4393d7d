#!/usr/bin/env python3
"""Where the minibatch kernel drains the LDS counter behind reads it does not need yet.

Compiles a translation unit of elegantrl_amd/csrc to gfx950 assembly with the Makefile's flags (or reads a finished .s file) and,
for every kernel and network path, lists every `s_waitcnt lgkmcnt(0)` that stands DIRECTLY behind a batch of LDS reads (a run of
ds_read* / ds_bpermute* instructions with nothing between it and the wait).  A wave issues in order and the LDS returns in order:
such a wait sits through the whole round trip of the batch just issued.  It is NEEDED when a destination register of that batch is
read before the next MFMA group ends (the next six MFMAs -- one k-step of a split product -- and every instruction up to them; the
scan stops early at a barrier, a branch or a label) or when a workgroup barrier follows before any MFMA (the batch must have landed
before other waves overwrite its source), else UNNEEDED: an older request was the one awaited, `lgkmcnt(<batch size>)`
or issuing the batch behind the wait would have done.  For ds_bpermute batches the tool also says whether the instruction right
behind the wait is the first reader (`immediate`: the hop is consumed where it is issued).

Only waits and LDS reads are looked at; nothing else about the code is judged.

    python tools/k6_lds_wait_sites.py ppo_step_s3_pre.hip [--sites] [--kernel SUBSTR] [--extra=-DERL_SLAB_ST=1]
    python tools/k6_lds_wait_sites.py --asm file.s
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elegantrl_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form"]     # csrc/Makefile, the s3 units
GROUP = 6                                                   # MFMAs of a k-step of a split product

KERNEL_RE = re.compile(r"^(_Z\w*ppo_step_\w*kernel\w*):")
REG_RE = re.compile(r"\b([va])(\d+)\b|\b([va])\[(\d+):(\d+)\]")
NO_DEST = ("ds_write", "ds_store", "global_store", "buffer_store", "flat_store", "scratch_store", "global_load_lds", "s_", "v_cmp", "v_nop",
           "global_atomic", "buffer_atomic")


def compile_unit(unit, extra):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    subprocess.check_call([HIPCC, *FLAGS, *extra, "--cuda-device-only", "-S", "-o", out, unit], cwd=CSRC, stderr=subprocess.DEVNULL)
    return out


def regs(text):
    s = set()
    for m in REG_RE.finditer(text):
        if m.group(1):
            s.add((m.group(1), int(m.group(2))))
        else:
            s.update((m.group(3), i) for i in range(int(m.group(4)), int(m.group(5)) + 1))
    return s


def split_ops(ins):
    """(mnemonic, destination registers, source registers) of one instruction line"""
    body = ins.split(";")[0].strip()
    parts = body.split(None, 1)
    mn = parts[0]
    ops = parts[1].split(",") if len(parts) > 1 else []
    if not ops or mn.startswith(NO_DEST):
        return mn, set(), regs(body)
    return mn, regs(ops[0]), regs(",".join(ops[1:]))


def is_lds_read(mn):
    return mn.startswith(("ds_read", "ds_load", "ds_bpermute", "ds_permute"))


def is_mfma(mn):
    return mn.startswith(("v_mfma", "v_smfma"))


def kernels(path):
    """{kernel name: [(line number, instruction text or 'LABEL')]}"""
    out, cur = {}, None
    with open(path) as f:
        for no, line in enumerate(f, 1):
            m = KERNEL_RE.match(line)
            if m:
                cur = out.setdefault(m.group(1), [])
                continue
            if cur is None:
                continue
            t = line.strip()
            if t.startswith(".Lfunc_end"):
                cur = None
            elif t.startswith(".LBB") and t.split(";")[0].strip().endswith(":"):
                cur.append((no, "LABEL"))
            elif t and not t.startswith((".", ";")):
                cur.append((no, t))
    return out


def paths_of(ins):
    """The kernel body is `actor ? block<true> : block<false>`: two copies of the same phases, each with the same number of barriers.
    The second path starts behind the last unconditional branch in front of its first barrier.  The actor's path is the one with the
    4x4x1 MFMAs of its output layer."""
    bars = [i for i, (_, t) in enumerate(ins) if t.startswith("s_barrier")]
    if len(bars) < 2 or len(bars) % 2:
        return [("whole kernel", 0, len(ins))]
    lo, hi = bars[len(bars) // 2 - 1], bars[len(bars) // 2]
    cut = max((i for i in range(lo, hi) if ins[i][1].startswith("s_branch")), default=lo) + 1
    names = []
    for a, b in ((0, cut), (cut, len(ins))):
        names.append("actor" if any(t.startswith("v_mfma_f32_4x4x1") for _, t in ins[a:b]) else "critic")
    if names[0] == names[1]:
        names = ["first path", "second path"]
    return [(names[0], 0, cut), (names[1], cut, len(ins))]


def sites_of(ins, a, b):
    """every full LDS wait directly behind a batch of LDS reads in ins[a:b]"""
    found = []
    for i in range(a, b):
        t = ins[i][1]
        if not (t.startswith("s_waitcnt") and "lgkmcnt(0)" in t):
            continue
        j = i - 1
        dests, kinds = set(), []
        while j >= a and ins[j][1] != "LABEL" and is_lds_read(split_ops(ins[j][1])[0]):
            mn, d, _ = split_ops(ins[j][1])
            dests |= d
            kinds.append(mn)
            j -= 1
        if not kinds:
            continue
        kind = ("ds_bpermute" if any(k.startswith(("ds_bpermute", "ds_permute")) for k in kinds)
                else "ds_read_b64_tr_b16" if any("_tr_" in k for k in kinds) else "ds_read_b128" if any(k.endswith("b128") for k in kinds) else "other")
        needed, first, seen = False, None, 0
        for k in range(i + 1, b):
            tt = ins[k][1]
            if tt.startswith("s_barrier") and seen == 0:
                needed, first = True, k - i             # the wait guards the barrier: other waves overwrite what the batch reads
                break
            if tt == "LABEL" or tt.startswith(("s_barrier", "s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
                break
            mn, _, src = split_ops(tt)
            if src & dests:
                needed = True
                first = k - i
                break
            if is_mfma(mn):
                seen += 1
                if seen == GROUP:
                    break
        found.append(dict(line=ins[i][0], kind=kind, batch=len(kinds), needed=needed, immediate=first == 1, mfmas_before_use=seen if needed else None))
    return found


def report(path, want=None, list_sites=False, out=sys.stdout):
    """prints the report; returns {kernel: {path: [site, ...]}}"""
    res = {}
    for name, ins in kernels(path).items():
        if want and want not in name:
            continue
        res[name] = {}
        nwait = sum(1 for _, t in ins if t.startswith("s_waitcnt") and "lgkmcnt" in t)
        nfull = sum(1 for _, t in ins if t.startswith("s_waitcnt") and "lgkmcnt(0)" in t)
        print(f"{name}: {nwait} waits on the LDS / scalar-memory counter, {nfull} of them lgkmcnt(0)", file=out)
        for pname, a, b in paths_of(ins):
            ss = sites_of(ins, a, b)
            res[name][pname] = ss
            print(f"  {pname}: {len(ss)} full waits directly behind a batch of LDS reads", file=out)
            for kind in ("ds_read_b128", "ds_read_b64_tr_b16", "ds_bpermute", "other"):
                k = [s for s in ss if s["kind"] == kind]
                if k:
                    extra = f", {sum(1 for s in k if s['immediate'])} consumed by the very next instruction" if kind == "ds_bpermute" else ""
                    print(f"    {kind:20s} {len(k):3d} sites: {sum(1 for s in k if not s['needed']):3d} unneeded, {sum(1 for s in k if s['needed']):3d} needed{extra}",
                          file=out)
            if list_sites:
                for s in ss:
                    print(f"      line {s['line']:6d} {s['kind']:20s} batch {s['batch']:2d} {'needed' if s['needed'] else 'UNNEEDED'}"
                          + (f" (first read behind {s['mfmas_before_use']} MFMAs)" if s["needed"] else ""), file=out)
    return res


def unneeded(res, kernel_substr, kind):
    return sum(1 for name, ps in res.items() if kernel_substr in name for ss in ps.values() for s in ss if s["kind"] == kind and not s["needed"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("unit", nargs="?", default="ppo_step_s3_pre.hip", help="translation unit under elegantrl_amd/csrc")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--kernel", help="only kernels whose mangled name contains this")
    ap.add_argument("--sites", action="store_true", help="list every site")
    ap.add_argument("--extra", action="append", default=[], help="further compiler flag (repeatable)")
    opt = ap.parse_args()
    path = opt.asm or compile_unit(opt.unit, opt.extra)
    print(f"# {opt.asm or opt.unit}  flags: {' '.join(FLAGS + opt.extra)}")
    report(path, opt.kernel, opt.sites)
    if not opt.asm:
        os.unlink(path)


if __name__ == "__main__":
    main()
