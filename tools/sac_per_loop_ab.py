#!/usr/bin/env python3
"""update_net with prioritised replay three ways, in ONE process on ONE card, for AgentSAC or AgentModSAC (--agent):

    per-step   AgentSAC._per_step per step: th.rand, erl_per_sample_f32, erl_replay_sample_rows_f32, the step, fmod / div, erl_per_update_f32
               (AgentSAC: args.per_loop_in_c off; AgentModSAC: args.mod_per_loop_in_c off, today's default)
    loop       the whole loop from one C call, every step starting with a stand-alone erl_per_sample_rows_f32 launch
               (AgentSAC: erl_sac_update_per_loop_f32, today's default; AgentModSAC: erl_sac_update_mod_per_loop_f32)
    loop+draw  the same call with the draw + gather inside every step's first launch (args.per_draw_in_step:
               erl_sac_update_per_draw_loop_f32; AgentModSAC: erl_sac_update_mod_per_loop_f32 with draw_in_step = 1)

Config 3's network and batch ([256, 256], B = 256, 64 sequences, 64 updates per update_net; AgentSAC 4 critics, AgentModSAC its 8 on the
fused step) on a ring of 2^14 rows per sequence, three quarters filled.

Method: the same agent and buffer serve the three routes (the switches are attributes); a few warm-up calls of each, then REGIONS regions
per route, alternating per-step / loop / loop+draw, each region CALLS update_net calls bracketed by device synchronisations on the host
clock (update_net ends in its own synchronising read of the objectives).  Reported: microseconds per update -- median, min, max,
inter-quartile range over the regions -- and, for each pair (candidate, the route it would replace), whether the candidate's median lies
below the other's by more than the candidate's own min .. max spread (the rule for a default: DESIGN.md section 9).

    (python tools/sac_per_loop_ab.py --agent sac; python tools/sac_per_loop_ab.py --agent modsac) > profiles/sac_per_loop_ab.txt
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
from elegantrl_amd.agents import AgentModSAC, AgentSAC  # noqa: E402
from elegantrl_amd.envs import SynVecEnv  # noqa: E402
from elegantrl_amd.train import Config, ReplayBuffer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--agent", choices=["sac", "modsac"], default="sac")
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--calls", type=int, default=3, help="update_net calls per region")
ap.add_argument("--warmup", type=int, default=3, help="update_net calls per route before the first region")
ap.add_argument("--num-seqs", type=int, default=64, help="a divisor of 256")
opt = ap.parse_args()

assert th.cuda.is_available(), "needs cuda:0: a time is a time on the GPU"
dev = th.device("cuda:0")
N, S, A, B, UPD, NET, MAX_SIZE = opt.num_seqs, 11, 3, 256, 64, [256, 256], 1 << 14
assert B % N == 0
agent_class = AgentModSAC if opt.agent == "modsac" else AgentSAC
args = Config(agent_class, SynVecEnv, {"env_name": "SynVecEnv", "num_envs": N, "max_step": 1000, "state_dim": S, "action_dim": A, "if_discrete": False})
args.net_dims, args.batch_size, args.if_use_per, args.per_alpha, args.per_beta, args.quiet = NET, B, True, 0.6, 0.4, True
args.fused_step = True                                  # (AgentModSAC: its prioritised loop has no layered form)
th.manual_seed(0)
agent = agent_class(NET, S, A, gpu_id=0, args=args)
buf = ReplayBuffer(max_size=MAX_SIZE, state_dim=S, action_dim=A, gpu_id=0, num_seqs=N, if_use_per=True, args=args)
g = th.Generator(device=dev).manual_seed(1)
for _ in range(3):                                  # three quarters of the ring, random transitions
    add = MAX_SIZE // 4
    buf.update((th.randn((add, N, S), device=dev, generator=g), th.randn((add, N, A), device=dev, generator=g).tanh(),
                th.randn((add, N), device=dev, generator=g), th.rand((add, N), device=dev, generator=g) < 0.99,
                th.rand((add, N), device=dev, generator=g) < 0.99))
agent.repeat_times = UPD * B / buf.cur_size
assert int(buf.cur_size * agent.repeat_times / B) == UPD

ROUTES = ("per-step", "loop", "loop+draw")
LOOP_SWITCH = "mod_per_loop_in_c" if opt.agent == "modsac" else "per_loop_in_c"


def region(route: str, calls: int) -> float:
    setattr(agent, LOOP_SWITCH, route != "per-step")
    agent.per_draw_in_step = route == "loop+draw"
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        agent.update_net(buf)
    th.cuda.synchronize()
    return (time.perf_counter() - t0) / (calls * UPD) * 1e6


paths = {}
for route in ROUTES:
    region(route, opt.warmup)
    paths[route] = agent.per_path
assert "per step" in paths["per-step"] and "one C call" in paths["loop"] and "inside the step's first launch" not in paths["loop"], paths
assert "one C call" in paths["loop+draw"] and "draw + gather inside the step's first launch" in paths["loop+draw"], paths
us = {route: [] for route in ROUTES}
for r in range(opt.regions):
    for route in ROUTES:
        us[route].append(region(route, opt.calls))


def stats(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), min(v), max(v), q[2] - q[0]


st = {route: stats(us[route]) for route in ROUTES}
print(f"# {agent_class.__name__}.update_net with prioritised replay, three routes (tools/sac_per_loop_ab.py --agent {opt.agent}): one process, one MI355X,")
print(f"# the same agent and buffer; net {NET}, {agent.num_ensembles} critics, B = {B}, {N} sequences, ring 2^14 rows per sequence holding {buf.cur_size},")
print(f"# per_alpha 0.6, per_beta 0.4, {UPD} updates per update_net; {opt.warmup} warm-up calls per route, then {opt.regions} regions per route, alternating,")
print(f"# {opt.calls} calls ({opt.calls * UPD} updates) per region, host clock between device synchronisations; microseconds per update.")
for route in ROUTES:
    s, v = st[route], us[route]
    print(f"{route:<10} median {s[0]:8.2f}  min {s[1]:8.2f}  max {s[2]:8.2f}  iqr {s[3]:6.2f}  n {len(v)}   regions: " + " ".join(f"{x:.1f}" for x in v))
for cand, base in (("loop", "per-step"), ("loop+draw", "loop"), ("loop+draw", "per-step")):
    c, b = st[cand], st[base]
    spread = c[2] - c[1]
    print(f"{base} median - {cand} median {b[0] - c[0]:8.2f} us per update ({b[0] / c[0]:.3f} x); {cand}'s own min .. max spread {spread:.2f}; "
          f"win beyond the spread: {b[0] - c[0] > spread}")
for route in ROUTES:
    print(f"# route {route:<10} = {paths[route]}")
smi = bench.smi_snapshot()
print("# box: " + json.dumps({"time": time.strftime("%Y-%m-%d %H:%M:%S"), "device": th.cuda.get_device_name(0), "torch": th.__version__,
                              "hip": th.version.hip, "smi": smi}))
