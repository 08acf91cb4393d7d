#!/usr/bin/env python3
"""Static instruction counts per profiled phase of ppo_step_s3_kernel, the actor's code path beside the critic's.

tools/isa_phase_cost.py stops at the first s_endpgm and knows one path; this kernel has an early exit and two straight-line paths (the
critic's first, then the actor's).  Here every s_memtime stamp of a -DERL_PROFILE [-DERL_PROFILE_FINE] build is named by the slot its
store goes to (g.prof[(net * 8 + wave) * 32 + slot]: byte offset 8 * slot, + 2048 for the critic), the instructions between two
consecutive stamps of one path are counted by class, and the two paths are printed side by side with their difference.

Usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -mllvm -amdgpu-mfma-vgpr-form -DERL_PROFILE -DERL_PROFILE_FINE \
             --cuda-device-only -S elegantrl_amd/csrc/ppo_step_s3_pre.hip -o pre.s
       isa_phase_diff.py pre.s ppo_step_s3_kernelILi2ELi4ELi4ELb1ELb1E"""
import re
import sys

SLOTS = {0: "entry", 16: "id arrived", 17: "row loads issued", 18: "W2 pieces / rows issued", 19: "rows in lanes", 1: "end of prologue",
         2: "barrier0 passed", 20: "own row normalised", 3: "end of L1 fwd", 21: "L2 tile 1", 22: "L2 tile 2", 23: "L2 tile 3",
         24: "L2 MFMA loop over", 4: "end of L2 fwd", 5: "end of out layer", 6: "end of objective", 29: "dZ2 formed", 25: "bwd tile 1",
         26: "bwd tile 2", 27: "bwd tile 3", 28: "bwd MFMA loop over", 7: "end of backward", 8: "barrier1 passed", 9: "dZ1/dY staged + barrier2",
         10: "A operand of dW1 + barrier2b", 11: "end of dW1", 12: "barrier3 + dW2 operand + barrier4", 13: "end of dW2", 14: "end of dW3",
         15: "logs written"}
CLASSES = ["bf16", "f32x32", "f32x16", "f32x4", "valu", "trans", "acc", "nop", "lds_r", "lds_w", "vmem", "salu", "wait"]
TRANS = ("v_exp_f32", "v_rcp_f32", "v_log_f32", "v_sqrt_f32", "v_rsq_f32")


def classify(op):
    if op.startswith("v_mfma_f32_32x32x16_bf16"): return "bf16"
    if op.startswith("v_mfma_f32_32x32"): return "f32x32"
    if op.startswith("v_mfma_f32_16x16"): return "f32x16"
    if op.startswith("v_mfma_f32_4x4"): return "f32x4"
    if op.startswith("v_accvgpr"): return "acc"
    if op.startswith(TRANS): return "trans"
    if op.startswith("v_"): return "valu"
    if op.startswith("s_nop"): return "nop"
    if op.startswith("s_waitcnt"): return "wait"
    if op.startswith("ds_read") or op.startswith("ds_bpermute"): return "lds_r"
    if op.startswith("ds_"): return "lds_w"
    if op.startswith(("global_", "buffer_", "scratch_")): return "vmem"
    if op.startswith("s_"): return "salu"
    return None


def main():
    path, name = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and name in l and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    segs = {0: [], 1: []}                                    # net -> [(slot, counts of the code in front of the stamp)]
    cur, pending = dict.fromkeys(CLASSES, 0), None
    for l in lines[start + 1:end]:
        t = l.strip()
        if not t or t[0] in ";.":
            continue
        op = t.split()[0]
        if op == "s_memtime":
            if pending is not None:                          # a stamp of another kind (the span stamps' own s_memtime): not a phase boundary
                cur = {k: cur[k] + pending[k] for k in CLASSES}
            pending, cur = cur, dict.fromkeys(CLASSES, 0)
            continue
        m = re.match(r"global_store_dwordx2 v\d+, v\[\d+:\d+\], s\[\d+:\d+\] offset:(\d+)$", t)
        if pending is not None and m and int(m.group(1)) % 8 == 0 and int(m.group(1)) < 4096:
            off = int(m.group(1))
            segs[off // 2048].append((off % 2048 // 8, pending))
            pending = None
            continue
        c = classify(op)
        if c:
            cur[c] += 1
    meta = {}
    for l in lines[end:end + 400]:
        m = re.match(r"\s*; (\w+)\s*(?::|=)\s*(\d+)", l)
        if m and m.group(1) in ("codeLenInByte", "TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize") and m.group(1) not in meta:
            meta[m.group(1)] = int(m.group(2))
    print("kernel metadata: " + ", ".join(f"{k} {v}" for k, v in meta.items()))
    actor = {s: c for s, c in segs[0]}
    order = [s for s, _ in segs[0]]
    critic = {s: c for s, c in segs[1]}
    print(f"{'code in front of stamp':34s} " + " ".join(f"{c:>11s}" for c in CLASSES) + "   (actor/critic, then actor - critic for the classes that differ)")
    tot = {n: dict.fromkeys(CLASSES, 0) for n in (0, 1)}
    for s in order[1:]:
        a, c = actor[s], critic.get(s)
        if c is None:
            continue
        for k in CLASSES:
            tot[0][k] += a[k]; tot[1][k] += c[k]                                # noqa: E702
        diff = ", ".join(f"{k} {a[k] - c[k]:+d}" for k in CLASSES if a[k] != c[k])
        print(f"{SLOTS.get(s, str(s)):34s} " + " ".join(f"{a[k]:5d}/{c[k]:<5d}" for k in CLASSES) + "   " + diff)
    print(f"{'whole path':34s} " + " ".join(f"{tot[0][k]:5d}/{tot[1][k]:<5d}" for k in CLASSES) + "   " +
          ", ".join(f"{k} {tot[0][k] - tot[1][k]:+d}" for k in CLASSES if tot[0][k] != tot[1][k]))


if __name__ == "__main__":
    main()
