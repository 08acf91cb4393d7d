#!/usr/bin/env python3
"""AgentDiscretePPO.update_net two ways on ONE rollout buffer with fixed minibatch ids (csrc/ppo_step_discrete.hip).

    (layered) the per-minibatch Python loop: erl_mlpn_ppo_step_discrete_f32 (one GEMM launch per dense layer, forward and backward,
              both networks) + erl_clip_adam_f32                                         -- args.fused_update = False
    (fused)   one erl_ppo_update_discrete_f32 call: per minibatch the fused kernel, the slab reduction and the two-launch
              clip + Adam tail                                                           -- args.fused_update = True

Shapes: CartPole's 4096 envs x 64 steps with net (64, 32); the same buffer with net (128, 128); state_dim 64, 8 actions with net
(128, 128).  batch_size 4096, repeat_times 1024 unless given: update_net runs int(horizon * repeat_times / batch_size) = 16 minibatches of
4096 samples per call (the agent's own formula; the tool exits when it gives none).  Method: one agent per route and shape in
one process, the same synthetic buffer and the same ids for both; a few warm-up calls of each, then REGIONS regions per route, the
routes alternating, each region CALLS update_net calls on the host clock between device synchronisations (update_net ends in its own
host read of the logged means).  Reported: milliseconds per update_net -- median, min, max, inter-quartile range over the regions --
and whether the fused median lies below the layered one.
    python tools/discrete_update_ab.py > profiles/discrete_update_ab.txt"""
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
ap.add_argument("--criterion", choices=["mse", "smooth_l1", "huber"], default="mse", help="args.criterion of both arms (reduction='none', torch's default threshold)")
opt = ap.parse_args()
N, H, B = opt.envs, opt.horizon, opt.batch
update_times = int(H * opt.repeat / B)              # AgentPPO.update_net's own count
if update_times < 1:
    sys.exit(f"discrete_update_ab: horizon {H} * repeat {opt.repeat:g} / batch {B} gives no minibatch (update_net needs at least one); "
             f"raise --repeat or lower --batch")
if not th.cuda.is_available():
    sys.exit("discrete_update_ab: needs a GPU (there is no CPU path to time)")

from elegantrl_amd.agents import AgentDiscretePPO  # noqa: E402
from elegantrl_amd.train import Config  # noqa: E402

DEV = th.device("cuda:0")
SHAPES = [("CartPole shape, net (64, 32)", 4, 2, [64, 32]), ("CartPole shape, net (128, 128)", 4, 2, [128, 128]),
          ("state_dim 64, 8 actions, net (128, 128)", 64, 8, [128, 128])]


def build(S, A, net, fused):
    args = Config(AgentDiscretePPO, None, {"env_name": "ab", "num_envs": N, "max_step": 500, "state_dim": S, "action_dim": A,
                                           "if_discrete": True})
    args.net_dims, args.fused_update, args.random_seed = net, fused, 0
    args.horizon_len, args.batch_size, args.repeat_times = H, B, opt.repeat
    args.criterion = {"mse": th.nn.MSELoss, "smooth_l1": th.nn.SmoothL1Loss, "huber": th.nn.HuberLoss}[opt.criterion](reduction="none")
    th.manual_seed(0)
    return AgentDiscretePPO(args.net_dims, S, A, gpu_id=0, args=args)


def buffer(S, A, gen):
    states = th.randn((H, N, S), device=DEV, generator=gen)
    actions = th.randint(0, A, (H, N), device=DEV, generator=gen, dtype=th.int32)
    logprobs = -th.log(th.tensor(float(A))) + 0.1 * th.randn((H, N), device=DEV, generator=gen)
    rewards = th.ones((H, N), device=DEV)
    undones = th.rand((H, N), device=DEV, generator=gen) > 0.02
    unmasks = th.rand((H, N), device=DEV, generator=gen) > 0.01
    last = th.randn((N, S), device=DEV, generator=gen)
    return (states, actions, logprobs, rewards, undones, unmasks), last


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
print(f"# tools/discrete_update_ab.py on one {prop.name} ({prop.multi_processor_count} CUs); shader clock: {clock}")
print(f"# AgentDiscretePPO.update_net on one buffer of {N} envs x {H} steps, batch_size {B}, repeat_times {opt.repeat:g}: {update_times} minibatches per call, fixed ids;")
print(f"# {opt.warmup} warm-up calls per route, then {opt.regions} regions per route, alternating, {opt.calls} calls per region on the host clock")
print("# between device synchronisations; milliseconds per update_net.")

all_below = True
for name, S, A, net in SHAPES:
    gen = th.Generator(device=DEV).manual_seed(1)
    items, last = buffer(S, A, gen)
    ids = th.randint(H * N, (update_times, B), device=DEV, generator=gen)
    agents = {"layered": build(S, A, net, False), "fused": build(S, A, net, True)}

    def call(agent):
        agent.last_state = last
        # update_net's GAE fixes truncated rewards / undones up in place: every call gets its own copies of the two
        buf = [items[0], items[1], items[2], items[3].clone(), items[4].clone(), items[5]]
        return agent.update_net(buf, ids=ids)

    r = alternate({k: (lambda ag=ag: call(ag)) for k, ag in agents.items()}, opt.warmup, opt.regions, opt.calls)
    assert agents["layered"].update_path == "layered" and agents["fused"].update_path == "fused"
    print(f"{name}  (S {S}, A {A})")
    line("layered minibatch loop", r["layered"])
    line("fused kernel, one-call loop", r["fused"])
    below = r["fused"]["median"] < r["layered"]["median"]
    beyond = r["layered"]["median"] - r["fused"]["median"] > r["layered"]["max"] - r["layered"]["min"]
    all_below = all_below and below
    print(f"    ratio of medians layered / fused {r['layered']['median'] / r['fused']['median']:.2f}; fused median below the layered median: {below}; "
          f"beyond the layered route's spread: {beyond}")
print(f"fused median below the layered median at every shape: {all_below}")
