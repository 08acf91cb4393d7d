#!/usr/bin/env python3
"""AgentModSAC.update_net two ways on ONE replay ring (csrc/sac_fused.hip with ActorFixSAC as a run-time variant, csrc/sac.hip).

    (layered)  the per-step Python loop: buffer.sample + erl_sac_update_opt_f32 (one MFMA GEMM launch per dense layer, forward and
               backward, times the critics), the two-time-scale rule in Python                 -- args.fused_step = False
    (fused)    one erl_sac_update_mod_ring_loop_f32 call: per step the fused tile kernels with the sample inside the first launch,
               the rule in C                                                                     -- args.fused_step = True
    (fused, per step)  the fused step, one erl_sac_update_mod_ring_f32 call per step (args.update_loop_in_c = False): what the
               one-call loop adds on top of the kernels; informational

Shapes: config 3's (state_dim 11, 3 actions, net [256, 256], 8 critics, batch 256), the same with net [128, 64], and state_dim 56,
8 actions with net [256, 256]; a ring of 64 envs x 256 rows and repeat_times chosen so that update_net runs --steps (64) steps per call.
Method: one agent per route and shape in one process, the same ring contents and the same seed for all; a few warm-up calls of each, then
REGIONS regions per route, the routes alternating, each region CALLS update_net calls on the host clock between device synchronisations
(update_net ends in its own host read of the logged objectives).  Reported: milliseconds per update_net -- median, min, max,
inter-quartile range over the regions -- and whether the fused median lies below the layered one by more than the layered route's own
spread (max - min), the project's rule for turning a route on by default.
    python tools/modsac_update_ab.py > profiles/modsac_update_ab.txt"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ERL_QUIET", "1")

import torch as th  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=64)
ap.add_argument("--rows", type=int, default=256)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--criterion", choices=["mse", "smooth_l1", "huber"], default="mse", help="args.criterion of both arms (reduction='none', torch's default threshold)")
opt = ap.parse_args()
N, ROWS, B = opt.envs, opt.rows, opt.batch
if not th.cuda.is_available():
    sys.exit("modsac_update_ab: needs a GPU (there is no CPU path to time)")

from elegantrl_amd.agents import AgentModSAC  # noqa: E402
from elegantrl_amd.train import Config, ReplayBuffer  # noqa: E402

DEV = th.device("cuda:0")
SHAPES = [("config 3: net [256, 256]", 11, 3, [256, 256]), ("config 3's env, net [128, 64]", 11, 3, [128, 64]),
          ("state_dim 56, 8 actions, net [256, 256]", 56, 8, [256, 256])]
ROUTES = {"layered": dict(fused_step=False), "fused": dict(fused_step=True), "fused, per step": dict(fused_step=True, update_loop_in_c=False)}


def build(S, A, net, items, **switches):
    args = Config(AgentModSAC, None, {"env_name": "ab", "num_envs": N, "max_step": 1000, "state_dim": S, "action_dim": A, "if_discrete": False})
    args.net_dims, args.batch_size, args.random_seed, args.num_ensembles = list(net), B, 0, 8
    args.criterion = {"mse": th.nn.MSELoss, "smooth_l1": th.nn.SmoothL1Loss, "huber": th.nn.HuberLoss}[opt.criterion](reduction="none")
    for k, v in switches.items():
        setattr(args, k, v)
    th.manual_seed(0)
    agent = AgentModSAC(args.net_dims, S, A, gpu_id=0, args=args)
    buf = ReplayBuffer(max_size=2 * ROWS, state_dim=S, action_dim=A, gpu_id=0, num_seqs=N, args=args)
    buf.update(items)
    agent.repeat_times = opt.steps * B / buf.cur_size            # update_times = int(cur_size * repeat_times / batch_size)
    assert int(buf.cur_size * agent.repeat_times / B) == opt.steps
    return agent, buf


def ring_items(S, A, gen):
    return (th.randn((ROWS, N, S), device=DEV, generator=gen), th.randn((ROWS, N, A), device=DEV, generator=gen).tanh(),
            th.randn((ROWS, N), device=DEV, generator=gen), th.rand((ROWS, N), device=DEV, generator=gen) > 0.02,
            th.rand((ROWS, N), device=DEV, generator=gen) > 0.01)


def stats(v):
    v = sorted(v)
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [v[0], v[len(v) // 2], v[-1]]
    return dict(median=statistics.median(v), min=v[0], max=v[-1], iqr=q[2] - q[0], n=len(v))


def timed(fn, calls):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    th.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def alternate(routes, warmup, regions, calls):
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in routes}
    for r in range(regions):
        for k, fn in routes.items():
            th.manual_seed(100 + r)                              # the same sample ids for every route of a region
            ms[k].append(timed(fn, calls))
    return {k: stats(v) for k, v in ms.items()}


def line(name, s):
    print(f"    {name:<34s} median {s['median']:9.3f}  min {s['min']:9.3f}  max {s['max']:9.3f}  iqr {s['iqr']:7.3f}  n {s['n']}")


prop = th.cuda.get_device_properties(0)
try:
    clock = f"{th.cuda.clock_rate(0)} MHz (torch.cuda.clock_rate at start)"
except Exception as e:          # the management library is optional
    clock = f"not available ({type(e).__name__})"
print(f"# tools/modsac_update_ab.py on one {prop.name} ({prop.multi_processor_count} CUs); shader clock: {clock}")
print(f"# AgentModSAC.update_net on one ring of {N} envs x {ROWS} rows, 8 critics, batch_size {B}: {opt.steps} steps per call (the actor skips about every third);")
print(f"# {opt.warmup} warm-up calls per route, then {opt.regions} regions per route, alternating, {opt.calls} calls per region on the host clock")
print("# between device synchronisations; milliseconds per update_net.")

all_beyond = True
for name, S, A, net in SHAPES:
    items = ring_items(S, A, th.Generator(device=DEV).manual_seed(1))
    pairs = {k: build(S, A, net, items, **sw) for k, sw in ROUTES.items()}
    r = alternate({k: (lambda ag=ag, bf=bf: ag.update_net(bf)) for k, (ag, bf) in pairs.items()}, opt.warmup, opt.regions, opt.calls)
    print(f"{name}  (S {S}, A {A})")
    for k, (ag, _) in pairs.items():
        print(f"    [{k}] step: {ag.kernel_path.split(':')[0].split('(')[0].strip()}; update_net: {ag.update_path.split('(')[0].strip()}")
    assert pairs["layered"][0].update_path.startswith("per step") and pairs["fused"][0].update_path.startswith("one C call")
    line("layered step, per-step loop", r["layered"])
    line("fused step, one-call loop", r["fused"])
    line("fused step, per-step calls", r["fused, per step"])
    below = r["fused"]["median"] < r["layered"]["median"]
    beyond = r["layered"]["median"] - r["fused"]["median"] > r["layered"]["max"] - r["layered"]["min"]
    all_beyond = all_beyond and beyond
    print(f"    ratio of medians layered / fused {r['layered']['median'] / r['fused']['median']:.2f}; fused median below the layered median: {below}; "
          f"beyond the layered route's spread: {beyond}")
print(f"fused median below the layered median by more than the layered route's spread at every shape: {all_beyond}")
