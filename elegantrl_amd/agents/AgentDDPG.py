"""`AgentTD3` and `AgentDDPG` on the HIP path: the deterministic off-policy pair of the reference's elegantrl/agents/AgentTD3.py
(`AgentTD3` :15-70, `AgentDDPG` :73-87 with `AgentBase.update_objectives`, AgentBase.py:191-224).

Everything numerical runs in liberl_hip.so (csrc/td3.hip): the exploration action is `erl_td3_explore_action_f32`, one update step after
the sample is ONE `erl_td3_update_f32` / `erl_td3_update_ring_f32` call -- target action with its clipped-action / unclipped-noise rule,
min over the target critic's heads, critic objective, clip + Adam, soft updates, the delayed actor step against the critic just updated --
and `update_net`'s loop can be ONE `erl_td3_update_ring_loop_f32` call.  The `nn.Module`s below describe the parameter layout (their
tensors are views into the flat blocks the kernels read and write, in the order of the reference's `state_dict`) and serve the
Evaluator's `actor(state)` and the checkpoints.  No torch fallback for the update math: its restatement lives in tests/td3_ref.py.

The module is called AgentDDPG, not AgentTD3: `from elegantrl.agents import AgentTD3, AgentDDPG` is the path the reference's scripts use and
the one supported; `import elegantrl.agents.AgentTD3` stays a ModuleNotFoundError.

One stated deviation, DDPG only (D1): the reference's `AgentBase.update_objectives` broadcasts a (B, 1) q against a
(B,) unmask and a (B,) label into (B, B) mismatched pairs; here the critic objective is the per-sample one,
`criterion(q_i, label_i) * unmask_i` -- TD3's formula with one head.
"""
from __future__ import annotations

import os
from copy import deepcopy
from typing import List, Optional, Tuple

import torch as th
from torch import nn

from .. import _hip
from ..train.config import Config
from .AgentBase import _FlatAdamState, _OffPolicyFlatAgent, build_mlp, layer_init_with_orthogonal

TEN = th.Tensor


class Actor(nn.Module):
    """state -> build_mlp([S, *net_dims, A]) -> tanh; exploration adds N(0, action_std) and clips to [-1, 1] (AgentTD3.py:126-136)."""

    def __init__(self, net_dims: List[int], state_dim: int, action_dim: int):
        super().__init__()
        self.state_dim, self.action_dim = state_dim, action_dim
        self.explore_noise_std = None
        self.net = build_mlp(dims=[state_dim, *net_dims, action_dim])
        layer_init_with_orthogonal(self.net[-1], std=0.1)

    def forward(self, state: TEN) -> TEN:
        return self.net(state).tanh()

    def get_action(self, state: TEN, action_std: float, noise: Optional[TEN] = None) -> TEN:
        action_avg = self.net(state).tanh()
        eps = th.randn_like(action_avg) if noise is None else noise
        return (action_avg + action_std * eps).clip(-1.0, 1.0)          # Normal(avg, std).sample().clip(-1, 1)


class CriticTwin(nn.Module):
    """ONE build_mlp([S + A, *net_dims, num_ensembles]): the trunk is shared, the last layer holds the heads (AgentTD3.py:146-150)."""

    def __init__(self, net_dims: List[int], state_dim: int, action_dim: int, num_ensembles: int = 2):
        super().__init__()
        self.state_dim, self.action_dim = state_dim, action_dim
        self.net = build_mlp(dims=[state_dim + action_dim, *net_dims, num_ensembles])
        layer_init_with_orthogonal(self.net[-1], std=0.5)

    def get_q_values(self, state: TEN, action: TEN) -> TEN:
        return self.net(th.cat((state, action), dim=1))

    def forward(self, state: TEN, action: TEN) -> TEN:
        return self.get_q_values(state, action).mean(dim=-1, keepdim=True)


class Critic(CriticTwin):
    """the same with one output (AgentTD3.py:139-143)"""

    def __init__(self, net_dims: List[int], state_dim: int, action_dim: int):
        super().__init__(net_dims, state_dim, action_dim, num_ensembles=1)


class AgentTD3(_OffPolicyFlatAgent):
    """Twin Delayed DDPG (AgentTD3.py:15-70): `num_ensembles` (8) heads on one critic trunk, target-policy smoothing with
    `policy_noise_std` (0.10), the actor and its target updated every `update_freq`-th (2) step, exploration noise `explore_noise_std`
    (0.05).  `update_path` / `rollout_path` name the route the last `update_net` / rollout took and, for a fallback, why."""
    # update_net's loop as ONE C call (erl_td3_update_ring_loop_f32), bit-identical to one erl_td3_update_ring_f32 call per step: the
    # default follows the A/B record (tools/td3_update_ab.py -> profiles/td3_update_ab.txt);
    # args.td3_loop_in_c / ERL_TD3_LOOP_IN_C override it
    _loop_in_c_default = "0"
    _ring_loop_path = "one C call (erl_td3_update_ring_loop_f32: sample, step and the actor's delay rule per step inside the call)"
    _per_why = "prioritised replay (a prioritised one-call loop is out of scope): sample_for_per, erl_td3_update_f32, tree update per step"

    def __init__(self, net_dims: List[int], state_dim: int, action_dim: int, gpu_id: int = 0, args: Config = None):
        args = Config() if args is None else args
        super().__init__(net_dims, state_dim, action_dim, gpu_id, args)
        if self.if_discrete:
            raise NotImplementedError(f"{type(self).__name__} is a continuous-action agent")
        if self.lambda_fit_cum_r != 0:
            raise NotImplementedError(f"{type(self).__name__}: lambda_fit_cum_r = {self.lambda_fit_cum_r} is not implemented by the HIP step "
                                      "(csrc/td3.hip holds no cumulative-reward term); leave args.lambda_fit_cum_r at 0")
        from .. import ops
        self._read_args(args)
        self.td3_loop_in_c = bool(getattr(args, "td3_loop_in_c", os.environ.get("ERL_TD3_LOOP_IN_C", self._loop_in_c_default) != "0"))
        self._spec = ops.Td3Spec(state_dim, action_dim, net_dims, self.num_ensembles)
        dev, f32 = self.device, th.float32
        sp = self._spec
        self._actor_flat = th.zeros(sp.actor_count, dtype=f32, device=dev)
        self._critic_flat = th.zeros(sp.critic_count, dtype=f32, device=dev)
        act = Actor(net_dims, state_dim, action_dim).to(dev)
        cri = self._make_critic(net_dims, state_dim, action_dim).to(dev)
        self._bind("_act", act, sp.actor_slices(), self._actor_flat)
        self._bind("cri", cri, sp.critic_slices(), self._critic_flat)
        self._actor_target_flat = self._actor_flat.clone()
        self._critic_target_flat = self._critic_flat.clone()
        self._bind("act_target", deepcopy(act), sp.actor_slices(), self._actor_target_flat)
        self._bind("cri_target", deepcopy(cri), sp.critic_slices(), self._critic_target_flat)
        self.act_optimizer = _FlatAdamState(sp.actor_count, self.learning_rate, dev)
        self.cri_optimizer = _FlatAdamState(sp.critic_count, self.learning_rate, dev)
        self._actor_step = 0                       # the actor optimiser's own Adam step (it steps only when the actor is updated)
        L = len(net_dims)
        self.kernel_path = (f"layered TD3 step (csrc/td3.hip: one MFMA GEMM launch per dense layer, {10 * L + 20} launches with the actor's "
                            f"update, {5 * L + 11} without)")
        if not getattr(args, "quiet", False) and os.environ.get("ERL_QUIET", "0") == "0":
            print(f"| {type(self).__name__}: {self.kernel_path}", flush=True)

    # ---- what differs between the two agents ------------------------------------------------------------
    def _read_args(self, args):
        self.update_freq = int(getattr(args, "update_freq", 2))
        self.num_ensembles = int(getattr(args, "num_ensembles", 8))
        self.policy_noise_std = float(getattr(args, "policy_noise_std", 0.10))
        self.explore_noise_std = float(getattr(args, "explore_noise_std", 0.05))
        if self.update_freq < 1:
            raise ValueError(f"args.update_freq = {self.update_freq} must be >= 1")

    def _make_critic(self, net_dims, state_dim, action_dim):
        return CriticTwin(net_dims, state_dim, action_dim, num_ensembles=self.num_ensembles)

    def _actor_gate(self, buffer) -> bool:
        """may the actor be updated at all during this update_net? (AgentDDPG: AgentBase.py:216)"""
        return True

    def _update_actor(self, buffer, update_t: int) -> bool:
        return self._actor_gate(buffer) and update_t % self.update_freq == 0              # AgentTD3.py:63

    # ---- checkpoints (the reference's file set: act, act_target, act_optimizer, cri, cri_target, cri_optimizer) ---------------------
    def _checkpoint_extras(self, if_save: bool):
        if not if_save:
            self._actor_step = int(self.act_optimizer.step_count)

    def _set_step_counts(self):
        """the optimisers' `step_count` (th.optim.Adam's own count, what a checkpoint stores)"""
        self.cri_optimizer.step_count = self._step
        self.act_optimizer.step_count = self._actor_step

    # ---- rollout ------------------------------------------------------------------------------------------
    @_hip.on_device
    def explore_action(self, state: TEN, noise: Optional[TEN] = None, out: Optional[TEN] = None, out_state: Optional[TEN] = None) -> TEN:
        """Actor.get_action(state, explore_noise_std) in one launch (erl_td3_explore_action_f32); `noise` (n, action_dim) injects the
        draw, else Philox keyed by (rng_seed, rng_counter, row, component).  `out` (n, action_dim) / `out_state` (n, state_dim),
        contiguous: the kernel writes the action / a copy of `state` there (the rollout passes its buffer rows: no copies)"""
        from .. import ops
        self._sync_modules()
        action = ops.td3_explore_action(self._spec, self._actor_flat, state.contiguous(), self.explore_noise_std,
                                        noise=None if noise is None else noise.contiguous(), seed=self.rng_seed, counter=self.rng_counter,
                                        out=out, out_state=out_state)
        self.rng_counter += 1
        return action

    _ROLLOUT_WHY = "one-launch rollouts are out of scope for AgentTD3 / AgentDDPG (DESIGN.md section 8)"

    @_hip.on_device
    def _explore_vec_env(self, env, horizon_len: int, noise: Optional[TEN] = None) -> Tuple[TEN, ...]:
        """AgentBase._explore_vec_env (AgentBase.py:130-170) as a per-step loop on any env of the vector protocol (`step_into` where the
        env has it): one erl_td3_explore_action_f32 launch writes the action and the state row, then the env steps"""
        self.rollout_path = f"per-step loop (erl_td3_explore_action_f32 + env.{'step_into' if hasattr(env, 'step_into') else 'step'} per step): {self._ROLLOUT_WHY}"
        return super()._explore_vec_env(env, horizon_len, noise)

    @_hip.on_device
    def _explore_one_env(self, env, horizon_len: int) -> Tuple[TEN, ...]:
        self.rollout_path = f"per-step loop (erl_td3_explore_action_f32 + env.step per step, one numpy env): {self._ROLLOUT_WHY}"
        return super()._explore_one_env(env, horizon_len)

    # ---- update -------------------------------------------------------------------------------------------
    def _nets(self) -> tuple:
        """the leading arguments of every ops.td3_update* call"""
        return (self._spec, (self._actor_flat, self._critic_flat, self._actor_target_flat, self._critic_target_flat),
                (self.act_optimizer.exp_avg, self.act_optimizer.exp_avg_sq, self.cri_optimizer.exp_avg, self.cri_optimizer.exp_avg_sq))

    def _hyper(self) -> dict:
        return dict(policy_noise_std=float(self.policy_noise_std), gamma=float(self.gamma), tau=float(self.soft_update_tau),
                    lr=float(self.learning_rate), max_norm=float(self.clip_grad_norm), criterion=self.criterion_code)

    def _count_step(self, update_actor: bool) -> dict:
        """advance the counters for one step; its keyword arguments"""
        self._step += 1
        if update_actor:
            self._actor_step += 1
        return dict(update_actor=update_actor, actor_step=self._actor_step, seed=self.rng_seed + 1, counter=self._step)

    def _update_on_batch(self, batch, objs_out: TEN, update_actor: bool, noise=None, is_weight=None, td_error_out=None, buffer=None):
        # (`buffer`: what the shared loop hands every step; nothing here reads it)
        from .. import ops
        kw = self._count_step(update_actor)
        ops.td3_update(*self._nets(), batch, self._step, **self._hyper(), objs_out=objs_out, noise=noise, is_weight=is_weight,
                       td_error_out=td_error_out, **kw)
        self._set_step_counts()

    def _update_from_ring(self, buffer, ring, ids: TEN, objs_out: TEN, update_actor: bool, noise=None):
        """ReplayBuffer.sample(ids) and the step from one C call; the buffer's stage / ids0 / ids1 end up as after `buffer.sample`"""
        from .. import ops
        arrays, sample_len, stage = ring
        kw = self._count_step(update_actor)
        ops.td3_update_from_ring(*self._nets(), arrays, ids, sample_len, stage, self._step, **self._hyper(), objs_out=objs_out, noise=noise, **kw)
        buffer.ids0, buffer.ids1 = stage.ids
        self._set_step_counts()

    def _update_ring_loop(self, buffer, ring, id_all: TEN, objs: TEN):
        """update_net's whole loop from ONE C call: step t = what _update_from_ring(id_all[t]) enqueues, the delay rule decided on the
        host side of the loop in C; afterwards the counters are what the per-step route leaves"""
        from .. import ops
        arrays, sample_len, stage = ring
        T, gate = id_all.shape[0], self._actor_gate(buffer)
        n_upd = ops.td3_update_ring_loop(*self._nets(), arrays, id_all, sample_len, stage, self._step + 1, self._actor_step, self.update_freq,
                                         gate, **self._hyper(), objs_all=objs, seed=self.rng_seed + 1, counter0=self._step + 1)
        assert n_upd == (len(range(0, T, self.update_freq)) if gate else 0), n_upd
        self._step += T
        self._actor_step += n_upd
        buffer.ids0, buffer.ids1 = stage.ids
        self._set_step_counts()

    def _step_kwargs(self, buffer, update_t: int, noise=None) -> dict:
        return dict(update_actor=self._update_actor(buffer, update_t), noise=noise)

    @_hip.on_device
    def update_objectives(self, buffer, update_t: int, ids: Optional[TEN] = None, noise: Optional[TEN] = None) -> Tuple[float, float]:
        """one step (AgentTD3.py:34-70 / AgentBase.py:191-224).  `ids` / `noise` (batch_size, action_dim) inject the random draws."""
        return super().update_objectives(buffer, update_t, ids, noise)

    def _ring_loop_reason(self, buffer, ring) -> Optional[str]:
        """on the interleaved ring the whole loop is one C call when `td3_loop_in_c` is on, else one erl_td3_update_ring_f32 call per step"""
        from ..ops import ReplayRing
        return (f"{type(buffer).__name__} offers no continuous-action ring of >= 2 rows" if not ring else
                "planar replay ring (args.replay_interleaved is off): erl_td3_update_ring_f32 per step" if not isinstance(ring[0], ReplayRing) else
                "args.td3_loop_in_c is off (ERL_TD3_LOOP_IN_C; profiles/td3_update_ab.txt): erl_td3_update_ring_f32 per step"
                if not self.td3_loop_in_c else None)


class AgentDDPG(AgentTD3):
    """DDPG (AgentTD3.py:73-87 on AgentBase.update_objectives, AgentBase.py:191-224): one critic head, no target-policy noise, exploration
    noise read from `args.explore_noise`, the actor updated on every step of an update_net whose buffer holds at least
    `buffer_init_size` rows.  The critic objective is the per-sample one (D1 in the module docstring)."""

    def _read_args(self, args):
        self.update_freq = 1
        self.num_ensembles = 1
        self.policy_noise_std = 0.0
        self.explore_noise_std = float(getattr(args, "explore_noise", 0.05))                # (AgentTD3.py:80: `explore_noise`, not `_std`)

    def _make_critic(self, net_dims, state_dim, action_dim):
        return Critic(net_dims, state_dim, action_dim)

    def _actor_gate(self, buffer) -> bool:
        return bool(buffer.cur_size >= self.buffer_init_size)                               # AgentBase.py:216
