#!/usr/bin/env python3
"""AgentTD3 / AgentDDPG.update_net the two ways the agents can run it on the interleaved uniform ring (csrc/td3.hip):

    (per step)     one erl_td3_update_ring_f32 call per step from the interpreter     -- args.td3_loop_in_c = False
    (one C call)   the whole loop from one erl_td3_update_ring_loop_f32 call           -- args.td3_loop_in_c = True

The two are bit-identical (tests/test_td3_gpu.py); this tool times them.  Cases (--case, default all): `td3-256` AgentTD3, net
[256, 256], S 17, A 6 (HalfCheetah-sized), 8 heads, batch 256, 64 envs x 64 rows in the ring, 16 steps per update_net; `td3-64` the
same with net [64, 32] and batch 64 (the golden's shape); `ddpg-256` AgentDDPG at the first case's shape.
Method: ONE agent and buffer per case in ONE process, `td3_loop_in_c` flipped between regions; a few warm-up calls of each route, then
REGIONS (7) regions per route, the routes alternating, each region CALLS (3) update_net calls on the host clock between device
synchronisations (update_net itself ends with one host sync).  Reported: milliseconds per update_net -- median, min .. max -- and
whether the one-call median lies below the per-step median by more than its own spread (max - min): DESIGN.md section 9's rule for
turning a route on by default.  The record goes to profiles/td3_update_ab.txt:
    timeout -k 10 300 python tools/td3_update_ab.py | tee profiles/td3_update_ab.txt"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("ERL_QUIET", "1")

import torch as th  # noqa: E402

CASES = {"td3-256": ("AgentTD3", (256, 256), 256), "td3-64": ("AgentTD3", (64, 32), 64), "ddpg-256": ("AgentDDPG", (256, 256), 256)}
ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=tuple(CASES) + ("all",), default="all")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--steps", type=int, default=16, help="update steps per update_net")
opt = ap.parse_args()
if not th.cuda.is_available():
    sys.exit("td3_update_ab: needs a GPU (there is no CPU path to time)")

import elegantrl_amd.agents as agents  # noqa: E402
from elegantrl_amd.train import Config, ReplayBuffer  # noqa: E402

DEV = th.device("cuda:0")
N, S, A, ROWS = 64, 17, 6, 64


def build(name, net, B):
    cls = getattr(agents, name)
    args = Config(cls, None, {"env_name": "ab", "num_envs": N, "max_step": 1000, "state_dim": S, "action_dim": A, "if_discrete": False})
    args.net_dims, args.batch_size, args.random_seed, args.buffer_init_size = list(net), B, 0, ROWS
    args.repeat_times = (opt.steps + 0.5) * B / ROWS
    th.manual_seed(0)
    agent = cls(args.net_dims, S, A, gpu_id=0, args=args)
    buf = ReplayBuffer(max_size=ROWS + 8, state_dim=S, action_dim=A, gpu_id=0, num_seqs=N)
    g = th.Generator().manual_seed(1)
    buf.update((th.randn(ROWS, N, S, generator=g).to(DEV), th.rand(ROWS, N, A, generator=g).mul(2).sub(1).to(DEV),
                th.randn(ROWS, N, generator=g).to(DEV), (th.rand(ROWS, N, generator=g) > 0.05).to(DEV), (th.rand(ROWS, N, generator=g) > 0.05).to(DEV)))
    assert int(buf.cur_size * agent.repeat_times / B) == opt.steps
    return agent, buf


def timed(fn, calls):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    th.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def case(title, name, net, B):
    agent, buf = build(name, net, B)
    paths = {}

    def route(loop):
        def fn():
            agent.td3_loop_in_c = loop
            agent.update_net(buf)
            paths[loop] = agent.update_path
        return fn

    routes = {"per step": route(False), "one C call": route(True)}
    for fn in routes.values():
        for _ in range(opt.warmup):
            fn()
    ms = {k: [] for k in routes}
    for _ in range(opt.regions):
        for k, fn in routes.items():
            ms[k].append(timed(fn, opt.calls))
    assert paths[False].startswith("per step: args.td3_loop_in_c is off") and paths[True].startswith("one C call")
    print(f"{title}: {name}.update_net, {opt.steps} steps, batch {B}, net {list(net)}, S {S}, A {A}, {agent.num_ensembles} heads, "
          f"update_freq {agent.update_freq}")
    st = {}
    for k, v in ms.items():
        v = sorted(v)
        st[k] = (statistics.median(v), v[0], v[-1])
        print(f"    {k:<12s} median {st[k][0]:9.3f}  min {v[0]:9.3f} .. max {v[-1]:9.3f}  n {len(v)}   ({st[k][0] / opt.steps * 1e3:.1f} us per step)", flush=True)
    one, per = st["one C call"], st["per step"]
    beyond = per[0] - one[0] > one[2] - one[1]
    print(f"    ratio of medians per step / one C call {per[0] / one[0]:.2f}; the loop's median below the per-step median by more than its own "
          f"spread: {beyond}", flush=True)
    return beyond


prop = th.cuda.get_device_properties(0)
print(f"# tools/td3_update_ab.py --case {opt.case} on one {prop.name} ({prop.multi_processor_count} CUs); {opt.warmup} warm-up calls per route, then "
      f"{opt.regions} regions per route, alternating, {opt.calls} calls per region on the host clock between device synchronisations; ms per update_net")
want = tuple(CASES) if opt.case == "all" else (opt.case,)
verdicts = [case(c, *CASES[c]) for c in want]
print(f"the one-call loop below the per-step route by more than its own spread in every case of this run: {all(verdicts)}")
