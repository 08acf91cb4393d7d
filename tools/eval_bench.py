#!/usr/bin/env python3
"""One policy evaluation both ways -- the Evaluator's step loop (args.fused_eval = False) and agent.evaluate_env (two launches) -- on
config 2's env (Pendulum 4096 x 200, PPO [128, 64]), config 4's (SynVecEnv 4096, S 64, A 8, max_step 1000, PPO [128, 128]) and config 3's
actor (SAC [256, 256] on SynVecEnv 4096, S 24, A 8, max_step 1000), and a short train_agent Pendulum run with an evaluation per
iteration both ways.  Same process, same box for both paths of a case; warm-up, then repeats with a device synchronisation around each
evaluation; median and spread (min .. max, and the interquartile range) are reported.

    python tools/eval_bench.py                  every case, one child process at a time, each under its own `timeout -k 10`; stops at the
                                                first that fails; the report goes to stdout (and to --out FILE)
    python tools/eval_bench.py --case pendulum  one case in this process (pendulum | synenv | sac | train | gap)
`gap` measures what tests/test_eval_fused_gpu.py bounds: the loop against the per-step-exact kernel path under zero noise."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = {"pendulum": 240, "synenv": 420, "sac": 420, "train": 300, "gap": 240}      # seconds allowed per child


def spread(xs):
    xs = sorted(xs)
    q = statistics.quantiles(xs, n=4) if len(xs) >= 4 else [xs[0], statistics.median(xs), xs[-1]]
    return {"median_ms": round(1e3 * statistics.median(xs), 3), "min_ms": round(1e3 * xs[0], 3), "max_ms": round(1e3 * xs[-1], 3),
            "iqr_ms": round(1e3 * (q[2] - q[0]), 3), "n": len(xs)}


def build(case):
    import torch as th
    from elegantrl_amd.agents import AgentPPO, AgentSAC
    from elegantrl_amd.envs import PendulumVecEnv, SynVecEnv
    from elegantrl_amd.train import Config
    N = 4096
    if case == "pendulum":
        cls, ea, net = AgentPPO, dict(env_name="Pendulum-v1", num_envs=N, max_step=200, state_dim=3, action_dim=1, if_discrete=False), [128, 64]
        env = PendulumVecEnv(N, max_step=200, gpu_id=0, seed=1)
    elif case == "synenv":
        cls, ea, net = AgentPPO, dict(env_name="SynVecEnv", num_envs=N, max_step=1000, state_dim=64, action_dim=8, if_discrete=False), [128, 128]
        env = SynVecEnv(N, 64, 8, max_step=1000, gpu_id=0, seed=1)
    else:
        cls, ea, net = AgentSAC, dict(env_name="SynVecEnv", num_envs=N, max_step=1000, state_dim=24, action_dim=8, if_discrete=False), [256, 256]
        env = SynVecEnv(N, 24, 8, max_step=1000, gpu_id=0, seed=1)
    args = Config(cls, None, ea)
    args.net_dims, args.random_seed, args.quiet = net, 0, True
    th.manual_seed(0)
    agent = cls(net, ea["state_dim"], ea["action_dim"], gpu_id=0, args=args)
    return agent, env, args


def time_case(case, warmup, reps):
    import tempfile
    import torch as th
    from elegantrl_amd.train.evaluator import Evaluator
    agent, env, args = build(case)
    out = {"case": case, "num_envs": env.num_envs, "max_step": env.max_step, "net_dims": list(args.net_dims), "agent": type(agent).__name__}
    with tempfile.TemporaryDirectory() as cwd, th.no_grad():
        for name, fused in (("loop", False), ("fused", True)):
            args.fused_eval = fused
            ev = Evaluator(cwd, env, args, agent=agent)
            ev.eval_times = env.num_envs                   # one round
            ts, rows = [], None
            for i in range(warmup + reps):
                th.cuda.synchronize()
                t0 = time.perf_counter()
                rows = ev.get_cumulative_rewards_and_step(agent.act)
                th.cuda.synchronize()
                if i >= warmup:
                    ts.append(time.perf_counter() - t0)
            assert ("fused evaluation" in ev.eval_path) == fused, ev.eval_path
            out[name] = dict(spread(ts), episodes=int(rows.shape[0]), mean_return=round(float(rows[:, 0].mean()), 4),
                             mean_length=round(float(rows[:, 1].mean()), 2))
    lo, fu = out["loop"], out["fused"]
    out["speedup_of_medians"] = round(lo["median_ms"] / fu["median_ms"], 2)
    out["win_beyond_loop_spread"] = bool(lo["median_ms"] - fu["median_ms"] > lo["max_ms"] - lo["min_ms"])
    return out


def time_train(iters):
    import tempfile
    import torch as th
    from elegantrl_amd import train_agent
    from elegantrl_amd.agents import AgentPPO
    from elegantrl_amd.envs import PendulumVecEnv
    from elegantrl_amd.train import Config
    out = {"case": "train", "what": f"train_agent, Pendulum 4096 envs x horizon 200, net [128, 64], {iters} iterations, 40 minibatches of 16384 and one evaluation per iteration"}
    for rep in range(2):                                   # the first pair warms the process up (kernel loads, the one-off workgroup-map measurement)
        for name, fused in (("loop", False), ("fused", True)):
            with tempfile.TemporaryDirectory() as cwd:
                args = Config(AgentPPO, PendulumVecEnv, dict(env_name="Pendulum-v1", num_envs=4096, max_step=200, state_dim=3, action_dim=1,
                                                             if_discrete=False))
                args.net_dims, args.horizon_len, args.batch_size, args.repeat_times = [128, 64], 200, 16384, 40 * 16384 / 200      # 40 minibatches per iteration
                args.gamma, args.reward_scale, args.learning_rate = 0.97, 2 ** -2, 4e-4
                args.break_step, args.eval_per_step, args.eval_times = 200 * iters, 1, 4096      # (total_step counts horizon steps)
                args.cwd, args.gpu_id, args.random_seed, args.if_keep_save, args.fused_eval = cwd, 0, 0, False, fused
                th.cuda.synchronize()
                t0 = time.perf_counter()
                train_agent(args, if_single_process=True)
                th.cuda.synchronize()
                out[name + "_s"] = round(time.perf_counter() - t0, 3)
    out["speedup"] = round(out["loop_s"] / out["fused_s"], 2)
    return out


def measure_gap():
    import numpy as np
    import torch as th
    from tests.eval_helpers import make_ppo as _make_ppo, loop_vs_exact_gap, oracle_table
    from elegantrl_amd.train.evaluator import get_cumulative_rewards_and_step_from_vec_env
    out = {"case": "gap", "what": "Evaluator loop vs per-step-exact kernel rollout under zero noise, Pendulum 256 x 200, net [128, 64]", "seeds": []}
    for seed in range(5):
        ep, mean, ok = loop_vs_exact_gap(seed)
        out["seeds"].append({"seed": seed, "max_episode_return_gap": ep, "mean_return_gap": mean, "all_lengths_200": ok})
    out["largest_episode_gap"] = max(s["max_episode_return_gap"] for s in out["seeds"])
    out["largest_mean_gap"] = max(s["mean_return_gap"] for s in out["seeds"])
    # the SynVecEnv cap of the same test: row counts and lengths, loop vs exact path
    agent, env, _ = _make_ppo("syn", 1024, 64, 8, (128, 128), 8)
    loop = get_cumulative_rewards_and_step_from_vec_env(env, agent.act).numpy()
    agent.last_state = env.reset()[0]
    items = agent._explore_vec_env(env, 8, noise=th.zeros((8, 1024, 8), device="cuda:0"))
    exact = oracle_table(items[3], items[4], items[5])
    out["synenv_max_step_8"] = {"rows_loop": int(loop.shape[0]), "rows_exact": int(exact.shape[0]),
                                "identical_lengths": float((loop[:, 1] == exact[:, 1]).mean()) if loop.shape == exact.shape else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cases", default="pendulum,synenv,sac,train")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        os.environ.setdefault("ERL_QUIET", "1")
        res = measure_gap() if a.case == "gap" else time_train(a.iters) if a.case == "train" else time_case(a.case, a.warmup, a.reps)
        print("EVAL_BENCH " + json.dumps(res), flush=True)
        return 0
    lines = []
    for case in a.cases.split(","):
        cmd = ["timeout", "-k", "10", str(CASES[case]), sys.executable, os.path.abspath(__file__), "--case", case, "--warmup", str(a.warmup),
               "--reps", str(a.reps), "--iters", str(a.iters)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("EVAL_BENCH ")]
        if p.returncode != 0 or not got:                   # a failed step ends the run: nothing more is started on the GPU
            print(p.stdout[-3000:], p.stderr[-3000:], f"eval_bench: case {case} ended with status {p.returncode}; stopping", sep="\n", flush=True)
            return p.returncode or 1
        lines.append(got[-1][len("EVAL_BENCH "):])
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
