#!/usr/bin/env python3
"""explore_env and one policy evaluation on the device-resident PointChasingVecEnv, each two ways: the per-step loop (the agent's action
launch + erl_pointchasing_step_f32 per step; args.fused_rollout = False) against one launch (erl_rollout_pointchasing_f32 /
erl_sac_rollout_pointchasing_f32), and the Evaluator's loop against agent.evaluate_env (two launches).  tools/discrete_rollout_ab.py's protocol.

AgentPPO net (128, 128) and AgentSAC net [256, 256]; N = 4096 envs, H = 64 steps, dim = 2; the evaluation at max_step 1024.  Method: one
agent + env per route in one process; a few warm-up calls of each, then REGIONS regions per route, the routes alternating, each region
CALLS calls on the host clock between device synchronisations.  Reported: milliseconds per call -- median, min, max, inter-quartile range
over the regions -- and whether the one-launch median lies below the loop's by more than the loop's own min .. max spread.
    python tools/pointchasing_rollout_ab.py > profiles/pointchasing_rollout_ab.txt"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ERL_QUIET", "1")

import torch as th  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--dim", type=int, default=2)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--eval-max-step", type=int, default=1024)
ap.add_argument("--eval-regions", type=int, default=7)
opt = ap.parse_args()
if not th.cuda.is_available():
    sys.exit("pointchasing_rollout_ab: needs a GPU (there is no CPU path to time)")

from elegantrl_amd.agents import AgentPPO, AgentSAC  # noqa: E402
from elegantrl_amd.envs import PointChasingVecEnv  # noqa: E402
from elegantrl_amd.train import Config  # noqa: E402
from elegantrl_amd.train.evaluator import get_cumulative_rewards_and_step_from_vec_env  # noqa: E402

N, H, DIM = opt.envs, opt.horizon, opt.dim
S, A = 4 * DIM, DIM
NETS = {AgentPPO: [128, 128], AgentSAC: [256, 256]}


def build(cls, fused, max_step):
    args = Config(cls, PointChasingVecEnv, {"env_name": "PointChasingVecEnv", "num_envs": N, "max_step": max_step, "state_dim": S,
                                            "action_dim": A, "if_discrete": False})
    args.net_dims, args.fused_rollout, args.random_seed = NETS[cls], fused, 0
    th.manual_seed(0)
    agent = cls(args.net_dims, S, A, gpu_id=0, args=args)
    env = PointChasingVecEnv(dim=DIM, num_envs=N, max_step=max_step, gpu_id=0, seed=1)
    agent.last_state = env.reset()[0]
    return agent, env


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
    for _ in range(regions):
        for k, fn in routes.items():
            ms[k].append(timed(fn, calls))
    return {k: stats(v) for k, v in ms.items()}


def line(name, s):
    print(f"    {name:<44s} median {s['median']:9.3f}  min {s['min']:9.3f}  max {s['max']:9.3f}  iqr {s['iqr']:7.3f}  n {s['n']}")


def verdict(loop, one):
    clear = loop["median"] - one["median"] > loop["max"] - loop["min"]
    print(f"    one launch / loop = {one['median'] / loop['median']:.3f}; below the loop by more than the loop's min .. max spread: {clear}")


prop = th.cuda.get_device_properties(0)
try:
    clock = f"{th.cuda.clock_rate(0)} MHz (torch.cuda.clock_rate at start)"
except Exception as e:          # the management library is optional
    clock = f"not available ({type(e).__name__})"
print(f"# tools/pointchasing_rollout_ab.py on one {prop.name} ({prop.multi_processor_count} CUs); shader clock: {clock}")
print(f"# PointChasingVecEnv dim {DIM}, {N} envs x {H} steps; {opt.warmup} warm-up calls per route, then {opt.regions} regions per route,")
print(f"# alternating, {opt.calls} calls per region on the host clock between device synchronisations; milliseconds per call.")

for cls in (AgentPPO, AgentSAC):
    pairs = {"loop": build(cls, False, 1024), "one": build(cls, True, 1024)}
    launches = []
    name = "fused_rollout" if cls is AgentPPO else "fused_rollout_offpolicy"
    inner = getattr(pairs["one"][1], name)
    setattr(pairs["one"][1], name, lambda *a, _inner=inner, **k: (launches.append(1), _inner(*a, **k))[1])
    routes = {k: (lambda ag=ag, env=env: ag.explore_env(env, H)) for k, (ag, env) in pairs.items()}
    r = alternate(routes, opt.warmup, opt.regions, opt.calls)
    assert len(launches) == opt.warmup + opt.regions * opt.calls, "the one-launch route did not run"
    print(f"{cls.__name__}.explore_env, net {NETS[cls]}")
    line("per-step loop (args.fused_rollout = False)", r["loop"])
    line("one launch", r["one"])
    verdict(r["loop"], r["one"])

    agent, env = build(cls, True, opt.eval_max_step)
    routes = {"loop": lambda: get_cumulative_rewards_and_step_from_vec_env(env, agent.act), "one": lambda: agent.evaluate_env(env)}
    assert agent.evaluate_env(env) is not None, "the fused evaluation did not run"
    r = alternate(routes, 1, opt.eval_regions, 1)
    print(f"{cls.__name__}, one evaluation x {opt.eval_max_step} steps (env.reset() + the steps + the episode table on the host)")
    line("Evaluator's loop", r["loop"])
    line("agent.evaluate_env (two launches)", r["one"])
    verdict(r["loop"], r["one"])
