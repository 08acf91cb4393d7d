#!/usr/bin/env python3
"""AgentTD3.explore_env and one evaluation, each the ways the agent can run them (csrc/sac_fused.hip sac_rollout_synenv_kernel<.., DET> and
det_actor_tile_kernel; csrc/sac.hip erl_td3_rollout_* / erl_td3_eval_* / erl_td3_explore_action_tile_f32).  AgentDDPG runs the same
launches (`--agent ddpg`).

    (loop, layered action)  the per-step loop on erl_td3_explore_action_f32 (one GEMM launch per dense layer + the action kernel) and
                            one env launch per step                                   -- args.fused_td3_rollout = False (the default)
    (loop, tile action)     the per-step loop on erl_td3_explore_action_tile_f32 (one launch) and one env launch per step
                                                                                      -- fused_td3_rollout = True, fused_rollout = False
    (one launch)            erl_td3_rollout_*_f32                                     -- fused_td3_rollout = True, fused_rollout = True
    (evaluation)            the Evaluator's loop (the torch module + env.step per step, episodes cut on the host) against
                            agent.evaluate_env (erl_td3_eval_*_f32 + the compaction launch)

Cases (--case, default all), net [256, 256]: `syn64` SynVecEnv S 56 / A 8, 64 envs x 256 steps; `syn4096` the same at 4096 envs x 64
steps; `pendulum` PendulumVecEnv, 4096 envs x 200 steps; `point` PointChasingVecEnv dim 2, 4096 envs x 64 steps; `eval-pendulum` /
`eval-syn` / `eval-point` one evaluation of 4096 envs at max_step 200 / 1000 / 1024; `gap` no timing: the bound of
tests/test_td3_rollout_gpu.py's evaluation test -- the Evaluator's loop with the fp32 Actor module against the same loop with the module
in fp64 (actions cast to fp32 for the env), Pendulum 256 envs x 200 steps, net (128, 64), weight seeds 0..4.
Method: one agent + env per route in ONE process, the same seeds for all; a few warm-up calls of each, then REGIONS (7) regions per
route, the routes alternating, each region CALLS (3) calls on the host clock between device synchronisations.  Reported: milliseconds
per call -- median, min, max -- and whether the one-launch median lies below both loops' medians by more than each loop's own spread
(max - min), the project's rule for turning a route on by default.  Run each case as a command of its own under a time limit:
    for c in syn64 syn4096 pendulum point eval-pendulum eval-syn eval-point gap; do timeout -k 10 300 python tools/td3_rollout_ab.py --case $c || break; done"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import tempfile
import time
from copy import deepcopy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ERL_QUIET", "1")

import torch as th  # noqa: E402

CASES = ("syn64", "syn4096", "pendulum", "point", "eval-pendulum", "eval-syn", "eval-point", "gap")
ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=CASES + ("all",), default="all")
ap.add_argument("--agent", choices=("td3", "ddpg"), default="td3")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--calls", type=int, default=3)
opt = ap.parse_args()
if not th.cuda.is_available():
    sys.exit("td3_rollout_ab: needs a GPU (there is no CPU path to time)")

from elegantrl_amd.agents import AgentDDPG, AgentTD3  # noqa: E402
from elegantrl_amd.envs import PendulumVecEnv, PointChasingVecEnv, SynVecEnv  # noqa: E402
from elegantrl_amd.train import Config  # noqa: E402
from elegantrl_amd.train.evaluator import Evaluator, get_cumulative_rewards_and_step_from_vec_env  # noqa: E402

DEV = th.device("cuda:0")
AGENT = AgentTD3 if opt.agent == "td3" else AgentDDPG


def build(kind, N, S, A, net, max_step, seed=0, **switches):
    args = Config(AGENT, None, {"env_name": kind, "num_envs": N, "max_step": max_step, "state_dim": S, "action_dim": A, "if_discrete": False})
    args.net_dims, args.random_seed, args.reward_scale, args.eval_times = list(net), 0, 1.0, 1
    for k, v in switches.items():
        setattr(args, k, v)
    th.manual_seed(seed)
    agent = AGENT(args.net_dims, S, A, gpu_id=0, args=args)
    env = (PendulumVecEnv(N, max_step=max_step, gpu_id=0, seed=5) if kind == "pendulum" else
           PointChasingVecEnv(A, N, max_step=max_step, gpu_id=0, seed=5) if kind == "point" else
           SynVecEnv(N, S, A, max_step=max_step, gpu_id=0, seed=5))
    agent.last_state = env.reset()[0]
    return agent, env, args


def stats(v):
    v = sorted(v)
    return dict(median=statistics.median(v), min=v[0], max=v[-1], n=len(v))


def timed(fn, calls):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    th.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def alternate(routes):
    for fn in routes.values():
        for _ in range(opt.warmup):
            fn()
    ms = {k: [] for k in routes}
    for _ in range(opt.regions):
        for k, fn in routes.items():
            ms[k].append(timed(fn, opt.calls))
    return {k: stats(v) for k, v in ms.items()}


def line(name, s):
    print(f"    {name:<44s} median {s['median']:9.3f}  min {s['min']:9.3f}  max {s['max']:9.3f}  n {s['n']}", flush=True)


ROLLOUT_ROUTES = {"loop, layered action": dict(fused_td3_rollout=False, fused_rollout=True),
                  "loop, tile action": dict(fused_td3_rollout=True, fused_rollout=False),
                  "one launch": dict(fused_td3_rollout=True, fused_rollout=True)}


def rollout_case(title, kind, N, S, A, net, max_step, H):
    pairs = {k: build(kind, N, S, A, net, max_step, **sw)[:2] for k, sw in ROLLOUT_ROUTES.items()}
    r = alternate({k: (lambda ag=ag, env=env: ag.explore_env(env, H)) for k, (ag, env) in pairs.items()})
    print(f"{title}: {AGENT.__name__}.explore_env, {N} envs x {H} steps, net {list(net)}, S {S}, A {A}")
    for k, (ag, _) in pairs.items():
        print(f"    [{k}] {ag.rollout_path}")
    assert pairs["one launch"][0].rollout_path.startswith("one launch (erl_td3_rollout_")
    assert pairs["loop, layered action"][0].rollout_path.startswith("per-step loop (erl_td3_explore_action_f32")
    assert pairs["loop, tile action"][0].rollout_path.startswith("per-step loop (tile action erl_td3_explore_action_tile_f32")
    for k in ROLLOUT_ROUTES:
        line(k, r[k])
    one = r["one launch"]["median"]
    beyond = all(r[k]["median"] - one > r[k]["max"] - r[k]["min"] for k in ("loop, layered action", "loop, tile action"))
    print(f"    ratio of medians: layered loop / one launch {r['loop, layered action']['median'] / one:.1f}, tile loop / one launch "
          f"{r['loop, tile action']['median'] / one:.1f}; one launch below both loops by more than each loop's spread: {beyond}", flush=True)
    return beyond


def eval_case(title, kind, N, S, A, net, max_step):
    out = {}
    for k, on in (("Evaluator's loop", False), ("evaluate_env (two launches)", True)):
        agent, env, args = build(kind, N, S, A, net, max_step, fused_td3_rollout=on, fused_rollout=True)
        args.cwd, args.eval_times = tempfile.mkdtemp(prefix="td3_rollout_ab_"), 1
        with contextlib.redirect_stdout(io.StringIO()):          # (the Evaluator's table header)
            ev = Evaluator(args.cwd, env, args, agent=agent)
        out[k] = (ev, agent)
    with contextlib.redirect_stdout(io.StringIO()):              # (it says its path once)
        r = alternate({k: (lambda ev=ev, ag=ag: ev.get_cumulative_rewards_and_step(ag.act)) for k, (ev, ag) in out.items()})
    print(f"{title}: one evaluation of {AGENT.__name__}, {N} envs, max_step {max_step}, net {list(net)}, S {S}, A {A}")
    for k, (ev, _) in out.items():
        print(f"    [{k}] {ev.eval_path.split(' (')[0]}")
    assert out["Evaluator's loop"][0].eval_path.startswith("loop evaluation") and "fused evaluation" in out["evaluate_env (two launches)"][0].eval_path
    for k in out:
        line(k, r[k])
    lo, on = r["Evaluator's loop"], r["evaluate_env (two launches)"]
    beyond = lo["median"] - on["median"] > lo["max"] - lo["min"]
    print(f"    ratio of medians loop / two launches {lo['median'] / on['median']:.1f}; below the loop by more than the loop's spread: {beyond}", flush=True)
    return beyond


class _Fp64Actor(th.nn.Module):
    """the module in fp64, its action cast to fp32 for the env"""

    def __init__(self, act):
        super().__init__()
        self.m = deepcopy(act).double()

    def forward(self, state):
        return self.m(state.double()).float()


def gap_case():
    print(f"gap: the Evaluator's loop with the fp32 Actor module of {AGENT.__name__} against the same loop with the module in fp64 (actions cast to")
    print("     fp32 for the env); Pendulum, 256 envs x 200 steps, net (128, 64), weight seeds 0..4; per seed: largest per-episode |return gap| / "
          "|gap of the mean return|")
    worst_ep = worst_mean = 0.0
    for seed in range(5):
        agent, env, _ = build("pendulum", 256, 3, 1, (128, 64), 200, seed=seed)
        a = get_cumulative_rewards_and_step_from_vec_env(env, agent.act)
        b = get_cumulative_rewards_and_step_from_vec_env(env, _Fp64Actor(agent.act))
        assert a.shape == b.shape == (256, 2) and bool((a[:, 1] == 200).all()) and bool((b[:, 1] == 200).all())
        ep, mean = float((a[:, 0] - b[:, 0]).abs().max()), abs(float(a[:, 0].mean()) - float(b[:, 0].mean()))
        worst_ep, worst_mean = max(worst_ep, ep), max(worst_mean, mean)
        print(f"    seed {seed}: {ep!r} / {mean!r}   (mean return {float(a[:, 0].mean()):.3f})", flush=True)
    print(f"    largest: {worst_ep!r} / {worst_mean!r}; allowed in the test: three times that = {3 * worst_ep!r} / {3 * worst_mean!r}")


prop = th.cuda.get_device_properties(0)
print(f"# tools/td3_rollout_ab.py --case {opt.case} --agent {opt.agent} on one {prop.name} ({prop.multi_processor_count} CUs); {opt.warmup} warm-up "
      f"calls per route, then {opt.regions} regions per route, alternating, {opt.calls} calls per region on the host clock between device "
      "synchronisations; ms per call")
want = CASES if opt.case == "all" else (opt.case,)
verdicts = []
NET = (256, 256)
if "syn64" in want:
    verdicts.append(rollout_case("syn64", "syn", 64, 56, 8, NET, 1000, 256))
if "syn4096" in want:
    verdicts.append(rollout_case("syn4096", "syn", 4096, 56, 8, NET, 1000, 64))
if "pendulum" in want:
    verdicts.append(rollout_case("pendulum", "pendulum", 4096, 3, 1, NET, 200, 200))
if "point" in want:
    verdicts.append(rollout_case("point", "point", 4096, 8, 2, NET, 1024, 64))
if "eval-pendulum" in want:
    verdicts.append(eval_case("eval-pendulum", "pendulum", 4096, 3, 1, NET, 200))
if "eval-syn" in want:
    verdicts.append(eval_case("eval-syn", "syn", 4096, 56, 8, NET, 1000))
if "eval-point" in want:
    verdicts.append(eval_case("eval-point", "point", 4096, 8, 2, NET, 1024))
if "gap" in want:
    gap_case()
if verdicts:
    print(f"one launch below the loops by more than their spread in every case of this run: {all(verdicts)}")
