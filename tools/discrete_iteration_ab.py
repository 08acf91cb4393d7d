#!/usr/bin/env python3
"""One iteration of a discrete agent -- explore_env + update_net -- two ways, both on the one-launch rollout (args.fused_rollout = True)
and the fused update loop (csrc/rollout_discrete.hip, csrc/ppo_step_discrete.hip):

    (scan)    args.fused_gae = False: update_net runs the critic over all (H, N) states (the layered value pass) and over last_state,
              then the GAE scan with its statistics and the normalisation
    (rollout) args.fused_gae = True: the rollout launch itself leaves values, cri(last_state), raw advantages, reward sums and the
              per-tile sums; update_net folds the sums, normalises (two small launches) and ends with erl_ppo_finish_f32

Shapes: 4096 envs x 64 steps on CartPole with net (64, 32) and (128, 128), on Acrobot with net (64, 32).  batch_size 4096, repeat_times
1024 unless given: 16 minibatches per update_net.  Method: one agent and one env per route and shape in one process; a few warm-up
iterations of each, then REGIONS regions per route, the routes alternating, each region CALLS iterations on the host clock between
device synchronisations.  Reported: milliseconds per iteration -- median, min, max, inter-quartile range over the regions -- and,
per route, the split of an iteration: explore_env and update_net timed on their own in the same alternating way, the advantage stage
(scan: value pass + scan + normalisation; rollout: fold + normalisation) timed stand-alone on the iteration's buffer, and the minibatch
loop as update_net less that stage.  Last line: the rule DESIGN.md section 9 sets for a change of the default.
    python tools/discrete_iteration_ab.py > profiles/discrete_iteration_ab.txt"""
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
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--repeat", type=float, default=1024.0)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--calls", type=int, default=3)
opt = ap.parse_args()
N, H, B = opt.envs, opt.horizon, opt.batch
update_times = int(H * opt.repeat / B)              # AgentPPO.update_net's own count
if update_times < 1:
    sys.exit(f"discrete_iteration_ab: horizon {H} * repeat {opt.repeat:g} / batch {B} gives no minibatch (update_net needs at least one); "
             f"raise --repeat or lower --batch")
if not th.cuda.is_available():
    sys.exit("discrete_iteration_ab: needs a GPU (there is no CPU path to time)")

from elegantrl_amd import ops  # noqa: E402
from elegantrl_amd.agents import AgentDiscretePPO  # noqa: E402
from elegantrl_amd.envs import AcrobotGpuVecEnv, CartPoleGpuVecEnv  # noqa: E402
from elegantrl_amd.train import Config  # noqa: E402

DEV = th.device("cuda:0")
SHAPES = [("CartPole-v1, net (64, 32)", CartPoleGpuVecEnv, 4, 2, [64, 32]), ("CartPole-v1, net (128, 128)", CartPoleGpuVecEnv, 4, 2, [128, 128]),
          ("Acrobot-v1, net (64, 32)", AcrobotGpuVecEnv, 6, 3, [64, 32])]


def build(env_cls, S, A, net, fused_gae):
    args = Config(AgentDiscretePPO, env_cls, {"env_name": env_cls.env_name, "num_envs": N, "max_step": 500, "state_dim": S, "action_dim": A,
                                              "if_discrete": True})
    args.net_dims, args.fused_rollout, args.fused_update, args.fused_gae, args.random_seed = net, True, True, fused_gae, 0
    args.horizon_len, args.batch_size, args.repeat_times = H, B, opt.repeat
    th.manual_seed(0)
    agent = AgentDiscretePPO(args.net_dims, S, A, gpu_id=0, args=args)
    env = env_cls(N, max_step=500, gpu_id=0, seed=1)
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
    print(f"    {name:<44s} median {s['median']:9.3f}  min {s['min']:9.3f}  max {s['max']:9.3f}  iqr {s['iqr']:7.3f}  n {s['n']}{extra}")


class Route:
    """an agent, its env and the pieces of one iteration"""

    def __init__(self, env_cls, S, A, net, fused_gae, ids):
        self.agent, self.env = build(env_cls, S, A, net, fused_gae)
        self.ids, self.items = ids, None
        self.stats = th.zeros(8, dtype=th.float64, device=DEV)

    def explore(self):
        self.items = self.agent.explore_env(self.env, H)

    def update(self):
        self.agent.update_net(list(self.items), ids=self.ids)

    def iteration(self):
        self.explore()
        self.update()

    def explore_then_update(self, which):
        """time one half of an iteration while the other still runs (an update needs its own fresh rollout)"""
        if which == "explore":
            ms = timed(self.explore, 1)
            self.update()
        else:
            self.explore()
            ms = timed(self.update, 1)
        return ms

    def advantage_stage(self):
        """what update_net does between the rollout and the minibatch loop, on the last buffer, leaving it as it was"""
        a = self.agent
        states, _, _, rewards, undones, unmasks = self.items
        c = a._rollout_cache
        if c is not None and "adv" in c:
            ops.adv_stats_fold(c["parts"], c["n_parts"], H, N, self.stats)
            ops.adv_normalize(c["adv"], self.stats, out=th.empty_like(c["adv"]))
        else:
            values = a.get_values(states)
            adv, _ = ops.gae_scan(rewards.clone(), undones.clone(), unmasks, values, a.get_values(a.last_state), float(a.gamma),
                                  float(a.lambda_gae_adv), use_v_trace=bool(a.if_use_v_trace), mutate=True, algo=a.gae_algo, stats=self.stats)
            ops.adv_normalize(adv, self.stats, out=adv)


prop = th.cuda.get_device_properties(0)
try:
    clock = f"{th.cuda.clock_rate(0)} MHz (torch.cuda.clock_rate at start)"
except Exception as e:          # the management library is optional
    clock = f"not available ({type(e).__name__})"
print(f"# tools/discrete_iteration_ab.py on one {prop.name} ({prop.multi_processor_count} CUs); shader clock: {clock}")
print(f"# AgentDiscretePPO explore_env + update_net, {N} envs x {H} steps, batch_size {B}, repeat_times {opt.repeat:g}: {update_times} minibatches per update;")
print(f"# args.fused_rollout = True and the fused update loop on both routes; {opt.warmup} warm-up iterations per route, then {opt.regions} regions per route,")
print(f"# alternating, {opt.calls} iterations per region on the host clock between device synchronisations; milliseconds per iteration.")

flip = True
for name, env_cls, S, A, net in SHAPES:
    gen = th.Generator(device=DEV).manual_seed(1)
    ids = th.randint(H * N, (update_times, B), device=DEV, generator=gen)
    routes = {"scan": Route(env_cls, S, A, net, False, ids), "rollout": Route(env_cls, S, A, net, True, ids)}
    r = alternate({k: v.iteration for k, v in routes.items()}, opt.warmup, opt.regions, opt.calls)
    for k, v in routes.items():
        assert (v.agent.rollout_path, v.agent.advantage_path, v.agent.update_path) == ("one-launch", k, "fused"), (k, v.agent.kernel_path)
    print(f"{name}  (S {S}, A {A})")
    line("value pre-pass + scan in update_net", r["scan"])
    line("values + GAE inside the rollout launch", r["rollout"])
    below = r["rollout"]["median"] < r["scan"]["median"]
    beyond = r["scan"]["median"] - r["rollout"]["median"] > r["scan"]["max"] - r["scan"]["min"]
    flip = flip and beyond
    print(f"    ratio of medians scan / rollout {r['scan']['median'] / r['rollout']['median']:.2f}; rollout-route median below the scan route's: {below}; "
          f"by more than the scan route's min-max spread: {beyond}")
    # the split of an iteration, per route
    for k, v in routes.items():
        parts = {"explore": [], "update": [], "stage": []}
        for _ in range(opt.regions):
            parts["explore"].append(v.explore_then_update("explore"))
            parts["update"].append(v.explore_then_update("update"))
            v.explore()
            parts["stage"].append(timed(v.advantage_stage, 1))
            v.update()
        e, u, s = (stats(parts[x]) for x in ("explore", "update", "stage"))
        print(f"    split, {k} route (single calls, {opt.regions} each):")
        line("  explore_env", e)
        line("  update_net", u)
        line("  advantage stage, stand-alone" + (" (pre-pass + scan + normalise)" if k == "scan" else " (fold + normalise)"), s)
        print(f"      minibatch loop and the rest of update_net, by difference of the medians: {u['median'] - s['median']:9.3f};  "
              f"the stage's share of the iteration: {100 * s['median'] / (e['median'] + u['median']):.1f} %")
print(f"rule for turning args.fused_gae on by default for the discrete agents (rollout-route median below the scan route's by more than that "
      f"route's min-max spread at every shape): {'met' if flip else 'NOT met'}")
