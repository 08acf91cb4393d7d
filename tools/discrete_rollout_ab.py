#!/usr/bin/env python3
"""AgentDiscretePPO.explore_env on CartPole three ways (or, with --env acrobot / --env mountaincar, on that env two ways), and one policy
evaluation two ways
(csrc/rollout_discrete.hip).

    (a) CartPoleVecEnv (torch ops) + the per-step loop            -- the only route before the device-resident env
    (b) CartPoleGpuVecEnv (erl_cartpole_step_f32) + the per-step loop (args.fused_rollout = False)
    (c) CartPoleGpuVecEnv + the one-launch rollout (erl_rollout_discrete_cartpole_f32)
--env acrobot has no torch-ops env: (b) AcrobotGpuVecEnv (erl_acrobot_step_f32) + the per-step loop against (c) AcrobotGpuVecEnv + the
one-launch rollout (erl_rollout_discrete_acrobot_f32).  --env mountaincar likewise: MountainCarGpuVecEnv (erl_mountaincar_step_f32,
erl_rollout_discrete_mountaincar_f32); its evaluation runs at max_step 500 like the others', not at the env's own 200.

N = 4096 envs, H = 64 steps, net (64, 32).  Method: one agent + env per route in one process; a few warm-up calls of each, then
REGIONS regions per route, the routes alternating, each region CALLS explore_env calls on the host clock between device
synchronisations.  Reported: milliseconds per explore_env -- median, min, max, inter-quartile range over the regions -- and whether (c)'s
median lies below (a)'s and (b)'s by more than their own min .. max spread.  The evaluation (max_step 500: env.reset() + 500 steps of the
greedy policy + the episode table on the host) is timed the same way through the Evaluator's loop and through agent.evaluate_env.
    python tools/discrete_rollout_ab.py > profiles/discrete_rollout_ab.txt
    python tools/discrete_rollout_ab.py --env acrobot >> profiles/discrete_rollout_ab.txt
    python tools/discrete_rollout_ab.py --env mountaincar >> profiles/discrete_rollout_ab.txt"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ERL_QUIET", "1")

import torch as th  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--env", choices=("cartpole", "acrobot", "mountaincar"), default="cartpole")
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--net", type=int, nargs=2, default=(64, 32))
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--eval-max-step", type=int, default=500)
ap.add_argument("--eval-regions", type=int, default=5)
opt = ap.parse_args()
if not th.cuda.is_available():
    sys.exit("discrete_rollout_ab: needs a GPU (there is no CPU path to time)")

from elegantrl_amd.agents import AgentDiscretePPO  # noqa: E402
from elegantrl_amd.envs import AcrobotGpuVecEnv, CartPoleGpuVecEnv, CartPoleVecEnv, MountainCarGpuVecEnv  # noqa: E402
from elegantrl_amd.train import Config  # noqa: E402
from elegantrl_amd.train.evaluator import get_cumulative_rewards_and_step_from_vec_env  # noqa: E402

N, H, NET = opt.envs, opt.horizon, list(opt.net)
# env name, state_dim, action_dim, the torch-ops env (or None) and the device-resident env
NAME, S, A, TORCH_ENV, GPU_ENV = {"cartpole": ("CartPole-v1", 4, 2, CartPoleVecEnv, CartPoleGpuVecEnv),
                                  "acrobot": ("Acrobot-v1", 6, 3, None, AcrobotGpuVecEnv),
                                  "mountaincar": ("MountainCar-v0", 2, 3, None, MountainCarGpuVecEnv)}[opt.env]


def build(env_cls, fused, max_step):
    args = Config(AgentDiscretePPO, env_cls, {"env_name": NAME, "num_envs": N, "max_step": max_step, "state_dim": S,
                                              "action_dim": A, "if_discrete": True})
    args.net_dims, args.fused_rollout, args.random_seed = NET, fused, 0
    th.manual_seed(0)
    agent = AgentDiscretePPO(args.net_dims, S, A, gpu_id=0, args=args)
    env = env_cls(N, max_step=max_step, gpu_id=0, seed=1)
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


def line(name, s, extra=""):
    print(f"    {name:<34s} median {s['median']:9.3f}  min {s['min']:9.3f}  max {s['max']:9.3f}  iqr {s['iqr']:7.3f}  n {s['n']}{extra}")


prop = th.cuda.get_device_properties(0)
try:
    clock = f"{th.cuda.clock_rate(0)} MHz (torch.cuda.clock_rate at start)"
except Exception as e:          # the management library is optional
    clock = f"not available ({type(e).__name__})"
print(f"# tools/discrete_rollout_ab.py on one {prop.name} ({prop.multi_processor_count} CUs); shader clock: {clock}")
print(f"# AgentDiscretePPO.explore_env, {NAME}, {N} envs x {H} steps, net {NET}; {opt.warmup} warm-up calls per route, then {opt.regions} regions")
print(f"# per route, alternating, {opt.calls} calls per region on the host clock between device synchronisations; milliseconds per call.")

pairs = {"b": build(GPU_ENV, False, 500), "c": build(GPU_ENV, True, 500)}
if TORCH_ENV is not None:
    pairs = {"a": build(TORCH_ENV, True, 500), **pairs}
routes = {k: (lambda ag=ag, env=env: ag.explore_env(env, H)) for k, (ag, env) in pairs.items()}
r = alternate(routes, opt.warmup, opt.regions, opt.calls)
assert all(pairs[k][0].rollout_path == ("one-launch" if k == "c" else "loop") for k in pairs)
print("rollout")
if "a" in r:
    line(f"(a) {TORCH_ENV.__name__} + loop", r["a"])
line(f"(b) {GPU_ENV.__name__} + loop", r["b"])
line(f"(c) {GPU_ENV.__name__}, one launch", r["c"])
win_b = r["b"]["median"] - r["c"]["median"] > r["b"]["max"] - r["b"]["min"]
if "a" in r:
    win_a = r["a"]["median"] - r["c"]["median"] > r["a"]["max"] - r["a"]["min"]
    print(f"    ratio of medians a / c {r['a']['median'] / r['c']['median']:.2f}, b / c {r['b']['median'] / r['c']['median']:.2f}; "
          f"(c) below (a) beyond (a)'s spread: {win_a}; below (b) beyond (b)'s spread: {win_b}")
else:
    print(f"    ratio of medians b / c {r['b']['median'] / r['c']['median']:.2f}; (c) below (b) beyond (b)'s spread: {win_b}")

MS = opt.eval_max_step
agent, env = build(GPU_ENV, True, MS)
rows = {}


def ev_loop():
    with th.no_grad():
        rows["loop"] = get_cumulative_rewards_and_step_from_vec_env(env, agent.act)


def ev_fused():
    rows["fused"] = agent.evaluate_env(env)
    assert rows["fused"] is not None


e = alternate({"loop": ev_loop, "fused": ev_fused}, 1, opt.eval_regions, 1)
print(f"evaluation  one evaluation of {N} envs x {MS} steps (env.reset(), the greedy policy, the episode table on the host)")
for k, name in (("loop", "Evaluator loop"), ("fused", "agent.evaluate_env (two launches)")):
    line(name, e[k], f"  episodes {rows[k].shape[0]}  mean return {float(rows[k][:, 0].mean()):.3f}")
win = e["loop"]["median"] - e["fused"]["median"] > e["loop"]["max"] - e["loop"]["min"]
print(f"    ratio of medians {e['loop']['median'] / e['fused']['median']:.2f}; fused below the loop beyond the loop's spread: {win}")
