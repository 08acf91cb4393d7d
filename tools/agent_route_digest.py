#!/usr/bin/env python3
"""sha256 digests of what every rollout / update route of the agents computes from a fixed seed: the check that a change to the
Python that CHOOSES the kernels (elegantrl_amd/agents/) left every route's bits alone.  Run it on the two commits to compare, on
the same machine, and diff the outputs:

    python tools/agent_route_digest.py                   > after.txt
    python tools/agent_route_digest.py --tree ../before  > before.txt      # imports elegantrl_amd from another checkout (built)

Per route: ITERS iterations of explore_env + update_net; hashed are the rollout tensors of the last iteration (as update_net left
them), the flat weights and Adam moments, `_grads[:update_times]` and the logs every update_net returned.  The SAC routes hash
their rollout tensors and the rows of evaluate_env.  The PendulumVecEnv routes and the AgentModSAC route run max_step 4: truncation and
auto-reset fall inside the horizon.  Shapes: 48 envs x 10 steps (H * N = 480 is no multiple of 256: the plane pitch
is padded), batch 256 = two slabs, two minibatches per update; one env x 10 steps, batch 4 for the single-env rollout."""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import elegantrl_amd from")
opt = ap.parse_args()
sys.path.insert(0, os.path.abspath(opt.tree))
os.environ.setdefault("ERL_QUIET", "1")

import numpy as np  # noqa: E402
import torch as th  # noqa: E402

if not th.cuda.is_available():
    sys.exit("agent_route_digest: needs a GPU")

from elegantrl_amd.agents import AgentA2C, AgentDiscretePPO, AgentModSAC, AgentPPO, AgentSAC  # noqa: E402
from elegantrl_amd.envs import CartPoleGpuVecEnv, PendulumVecEnv, SynVecEnv  # noqa: E402
from elegantrl_amd.train import Config  # noqa: E402

ITERS, N, H, B, S, A = 3, 48, 10, 256, 17, 3


class StubEnv:
    """single numpy env: the state is a fixed function of the step count and the action, an episode ends every fourth step"""

    def __init__(self, state_dim):
        self.S, self.t = state_dim, 0

    def _state(self, a=0.0):
        return np.sin(np.arange(self.S, dtype=np.float32) * 0.7 + 0.3 * self.t + a).astype(np.float32)

    def reset(self):
        return self._state(), {}

    def step(self, action):
        self.t += 1
        a = float(np.sum(action))
        return self._state(a), float(np.cos(a + self.t)), self.t % 4 == 0, self.t % 7 == 0, {}


def sha(tensors, logs):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().contiguous().cpu()
        h.update(str((t.dtype, tuple(t.shape))).encode())
        h.update(t.view(th.uint8).numpy().tobytes() if t.numel() else b"")
    h.update(np.asarray(logs, dtype=np.float64).tobytes())
    return h.hexdigest()


def make(cls, env, S_, A_, net, n_envs, batch, repeat, discrete, **flags):
    args = Config(cls, None, {"env_name": "digest", "num_envs": n_envs, "max_step": 6, "state_dim": S_, "action_dim": A_,
                              "if_discrete": discrete})
    args.net_dims, args.random_seed, args.horizon_len, args.batch_size, args.repeat_times = list(net), 7, H, batch, repeat
    for k, v in flags.items():
        setattr(args, k, v)
    th.manual_seed(11)
    agent = cls(args.net_dims, S_, A_, gpu_id=0, args=args)
    state = env.reset()[0]
    agent.last_state = state if th.is_tensor(state) else th.as_tensor(state, dtype=th.float32, device=agent.device).reshape(1, S_)
    return agent


def on_policy(name, cls, env, S_, A_, net, n_envs=N, batch=B, repeat=52.0, discrete=False, rollout=None, **flags):
    agent = make(cls, env, S_, A_, net, n_envs, batch, repeat, discrete, **flags)
    logs = []
    for _ in range(ITERS):
        items = agent.explore_env(env, H)
        left = agent._rollout_cache or {}      # what the rollout left for update_net: nothing | the critic's values | + advantages
        logs.append(agent.update_net(list(items)))
    got = getattr(agent, "rollout_path", None) or ("one-launch" if agent._last_state_token is not None else "loop")
    assert rollout is None or got == rollout, (name, got, agent.kernel_path)
    update_times = int(H * repeat / batch)
    assert update_times >= 2
    digest = sha([*items, agent._flat, agent._exp_avg, agent._exp_avg_sq, agent._grads[:update_times]], logs)
    print(f"{digest}  {name}  [rollout: {got}; left for update_net: {'values + advantages' if 'adv' in left else 'values' if left else 'nothing'}]",
          flush=True)


def syn():
    return SynVecEnv(N, S, A, max_step=6, gpu_id=0, seed=5)


def cartpole():
    return CartPoleGpuVecEnv(N, max_step=6, gpu_id=0, seed=5)


on_policy("AgentPPO (128,128) one-launch rollout, fused_gae on", AgentPPO, syn(), S, A, (128, 128), rollout="one-launch", fused_rollout=True, fused_gae=True)
on_policy("AgentPPO (128,128) one-launch rollout, fused_gae off", AgentPPO, syn(), S, A, (128, 128), rollout="one-launch", fused_rollout=True, fused_gae=False)
on_policy("AgentPPO (128,128) raw-stepper loop", AgentPPO, syn(), S, A, (128, 128), rollout="loop", fused_rollout=False)
on_policy("AgentPPO wide (256,128)", AgentPPO, syn(), S, A, (256, 128), rollout="loop")
on_policy("AgentPPO three-layer (64,64,32) layered", AgentPPO, syn(), S, A, (64, 64, 32), rollout="loop")
for gae in (True, False):
    on_policy(f"AgentDiscretePPO (64,32) CartPole one-launch rollout, fused_gae {'on' if gae else 'off'}", AgentDiscretePPO, cartpole(), 4, 2,
              (64, 32), discrete=True, rollout="one-launch", fused_rollout=True, fused_gae=gae)
on_policy("AgentDiscretePPO (64,32) CartPole fused_update off", AgentDiscretePPO, cartpole(), 4, 2, (64, 32), discrete=True, rollout="one-launch",
          fused_rollout=True, fused_update=False)
on_policy("AgentA2C (64,32) one numpy env", AgentA2C, StubEnv(5), 5, 2, (64, 32), n_envs=1, batch=4, repeat=1.0)
on_policy("AgentDiscretePPO (64,32) one numpy env", AgentDiscretePPO, StubEnv(5), 5, 3, (64, 32), n_envs=1, batch=4, repeat=1.0, discrete=True)



def pendulum():
    return PendulumVecEnv(N, max_step=4, gpu_id=0, seed=5)


for net, name in (((128, 64), "tuned class"), ((64, 64), "general class")):
    on_policy(f"AgentPPO {net} Pendulum one-launch rollout ({name})", AgentPPO, pendulum(), 3, 1, net, rollout="one-launch", fused_rollout=True,
              fused_gae=True)
on_policy("AgentPPO (128,64) Pendulum raw-stepper loop", AgentPPO, pendulum(), 3, 1, (128, 64), rollout="loop", fused_rollout=False)
# the evaluation form of the PPO rollout on both envs
for name, env, S_, A_, net in (("SynVecEnv", syn(), S, A, (128, 128)), ("Pendulum", pendulum(), 3, 1, (128, 64))):
    agent = make(AgentPPO, env, S_, A_, net, N, B, 52.0, False, fused_rollout=True)
    agent.explore_env(env, H)
    rows = agent.evaluate_env(env)
    assert rows is not None, agent._fused_eval_reason(env)
    print(f"{sha([rows, env.state, env.step_count, env.episode], [])}  AgentPPO {net} {name} evaluate_env", flush=True)


def off_policy(name, cls, env, S_, A_, net=(64, 64)):
    """the one-launch off-policy rollout and the evaluation that goes with it (AgentModSAC: both are opt-in, fused_mod_rollout)"""
    agent = make(cls, env, S_, A_, net, N, B, 1.0, False, fused_rollout=True, fused_mod_rollout=True)
    for _ in range(ITERS):
        items = agent.explore_env(env, H)
    assert agent._last_state_token is not None, agent.kernel_path
    rows = agent.evaluate_env(env)
    assert rows is not None, agent._fused_eval_reason(env)
    print(f"{sha([*items, agent.last_state, rows], [])}  {name} one-launch rollout + evaluate_env", flush=True)


off_policy("AgentSAC (64,64)", AgentSAC, SynVecEnv(N, S, A, max_step=6, gpu_id=0, seed=5), S, A)
off_policy("AgentSAC (64,64) Pendulum", AgentSAC, pendulum(), 3, 1)
off_policy("AgentModSAC (64,64)", AgentModSAC, SynVecEnv(N, S, A, max_step=4, gpu_id=0, seed=5), S, A)
off_policy("AgentModSAC (64,64) Pendulum", AgentModSAC, pendulum(), 3, 1)
