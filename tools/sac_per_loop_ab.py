#!/usr/bin/env python3
"""AgentSAC.update_net with prioritised replay both ways, in ONE process on ONE card: args.per_loop_in_c off (AgentSAC._per_step per step:
th.rand, erl_per_sample_f32, erl_replay_sample_rows_f32, the step, fmod / div, erl_per_update_f32 -- the route before the loop existed,
untouched) against on (erl_sac_update_per_loop_f32: the whole loop from one C call).  Config 3's network and batch ([256, 256], 4 critics,
B = 256, 64 sequences, 64 updates per update_net) on a ring of 2^14 rows per sequence, three quarters filled.

Method: the same agent and buffer serve both routes (the switch is an attribute); a few warm-up calls of each, then REGIONS regions per
route, alternating off / on, each region CALLS update_net calls bracketed by device synchronisations on the host clock (update_net ends in
its own synchronising read of the objectives).  Reported: microseconds per update -- median, min, max, inter-quartile range over the
regions -- and whether the switch-on median lies below the switch-off median by more than the switch-off regions' own min .. max spread.

    python tools/sac_per_loop_ab.py > profiles/sac_per_loop_ab.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (smi_snapshot)
from elegantrl_amd.agents import AgentSAC  # noqa: E402
from elegantrl_amd.envs import SynVecEnv  # noqa: E402
from elegantrl_amd.train import Config, ReplayBuffer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--regions", type=int, default=9)
ap.add_argument("--calls", type=int, default=30, help="update_net calls per region")
ap.add_argument("--warmup", type=int, default=3, help="update_net calls per route before the first region")
ap.add_argument("--num-seqs", type=int, default=64, help="a divisor of 256")
opt = ap.parse_args()

assert th.cuda.is_available(), "needs cuda:0: a time is a time on the GPU"
dev = th.device("cuda:0")
N, S, A, B, UPD, NET, MAX_SIZE = opt.num_seqs, 11, 3, 256, 64, [256, 256], 1 << 14
assert B % N == 0
args = Config(AgentSAC, SynVecEnv, {"env_name": "SynVecEnv", "num_envs": N, "max_step": 1000, "state_dim": S, "action_dim": A, "if_discrete": False})
args.net_dims, args.batch_size, args.if_use_per, args.per_alpha, args.per_beta, args.quiet = NET, B, True, 0.6, 0.4, True
th.manual_seed(0)
agent = AgentSAC(NET, S, A, gpu_id=0, args=args)
buf = ReplayBuffer(max_size=MAX_SIZE, state_dim=S, action_dim=A, gpu_id=0, num_seqs=N, if_use_per=True, args=args)
g = th.Generator(device=dev).manual_seed(1)
for _ in range(3):                                  # three quarters of the ring, random transitions
    add = MAX_SIZE // 4
    buf.update((th.randn((add, N, S), device=dev, generator=g), th.randn((add, N, A), device=dev, generator=g).tanh(),
                th.randn((add, N), device=dev, generator=g), th.rand((add, N), device=dev, generator=g) < 0.99,
                th.rand((add, N), device=dev, generator=g) < 0.99))
agent.repeat_times = UPD * B / buf.cur_size
assert int(buf.cur_size * agent.repeat_times / B) == UPD


def region(on: bool, calls: int) -> float:
    agent.per_loop_in_c = on
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        agent.update_net(buf)
    th.cuda.synchronize()
    return (time.perf_counter() - t0) / (calls * UPD) * 1e6


paths = {}
for on in (False, True):
    region(on, opt.warmup)
    paths[on] = agent.per_path
assert "one C call" in paths[True] and "per step" in paths[False], paths
us = {False: [], True: []}
for r in range(opt.regions):
    for on in (False, True):
        us[on].append(region(on, opt.calls))


def stats(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), min(v), max(v), q[2] - q[0]


off, on = stats(us[False]), stats(us[True])
print("# AgentSAC.update_net with prioritised replay, args.per_loop_in_c off against on (tools/sac_per_loop_ab.py): one process, one MI355X, the same")
print(f"# agent and buffer; net {NET}, 4 critics, B = {B}, {N} sequences, ring 2^14 rows per sequence holding {buf.cur_size}, per_alpha 0.6, per_beta 0.4,")
print(f"# {UPD} updates per update_net; {opt.warmup} warm-up calls per route, then {opt.regions} regions per route, alternating, {opt.calls} calls"
      f" ({opt.calls * UPD} updates) per region, host clock")
print("# between device synchronisations; microseconds per update.")
for name, s, v in (("off", off, us[False]), ("on ", on, us[True])):
    print(f"per_loop_in_c {name}  median {s[0]:8.2f}  min {s[1]:8.2f}  max {s[2]:8.2f}  iqr {s[3]:6.2f}  n {len(v)}   regions: " + " ".join(f"{x:.1f}" for x in v))
spread = off[2] - off[1]
print(f"off median - on median {off[0] - on[0]:.2f} us per update ({off[0] / on[0]:.3f} x); the off regions' min .. max spread {spread:.2f}; "
      f"win beyond the spread: {off[0] - on[0] > spread}")
print(f"# routes: off = {paths[False]}")
print(f"#         on  = {paths[True]}")
smi = bench.smi_snapshot()
print("# box: " + json.dumps({"time": time.strftime("%Y-%m-%d %H:%M:%S"), "device": th.cuda.get_device_name(0), "torch": th.__version__,
                              "hip": th.version.hip, "smi": smi}))
