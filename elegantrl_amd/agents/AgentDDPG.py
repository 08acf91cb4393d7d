"""`AgentTD3` and `AgentDDPG` on the HIP path: the deterministic off-policy pair of the reference's elegantrl/agents/AgentTD3.py
(`AgentTD3` :15-70, `AgentDDPG` :73-87 with `AgentBase.update_objectives`, AgentBase.py:191-224).

Everything numerical runs in liberl_hip.so (csrc/td3.hip): the exploration action is `erl_td3_explore_action_f32`, one update step after
the sample is ONE `erl_td3_update_f32` / `erl_td3_update_ring_f32` call -- target action with its clipped-action / unclipped-noise rule,
min over the target critic's heads, critic objective, clip + Adam, soft updates, the delayed actor step against the critic just updated --
and `update_net`'s loop can be ONE `erl_td3_update_ring_loop_f32` call.  The `nn.Module`s below describe the parameter layout (their
tensors are views into the flat blocks the kernels read and write, in the order of the reference's `state_dict`) and serve the
Evaluator's `actor(state)` and the checkpoints.  No torch fallback for the update math: its restatement lives in tests/td3_ref.py.
Opt-in (`args.fused_td3_rollout`): the exploration action as one launch of a tile kernel (`erl_td3_explore_action_tile_f32`) and, on the
device-resident continuous envs, the whole rollout and the whole evaluation as one launch each (`erl_td3_rollout_*_f32`,
`erl_td3_eval_*_f32`: csrc/sac_fused.hip, the deterministic-actor forms of AgentSAC's persistent rollout kernel).

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
    (0.05).  `update_path` / `rollout_path` name the route the last `update_net` / rollout took and, for a fallback, why.
    With `fused_td3_rollout` on and inside erl_td3_rollout_supported's shapes, `explore_action` is the tile kernel
    (erl_td3_explore_action_tile_f32) and, on SynVecEnv / PendulumVecEnv / PointChasingVecEnv with `fused_rollout`, `explore_env` and
    `evaluate_env` are one launch each (erl_td3_rollout_*, erl_td3_eval_*: csrc/sac_fused.hip sac_rollout_synenv_kernel<.., DET>)."""
    # update_net's loop as ONE C call (erl_td3_update_ring_loop_f32), bit-identical to one erl_td3_update_ring_f32 call per step: the
    # default follows the A/B record (tools/td3_update_ab.py -> profiles/td3_update_ab.txt);
    # args.td3_loop_in_c / ERL_TD3_LOOP_IN_C override it
    _loop_in_c_default = "0"
    _ring_loop_path = "one C call (erl_td3_update_ring_loop_f32: sample, step and the actor's delay rule per step inside the call)"
    _per_why = "prioritised replay (a prioritised one-call loop is out of scope): sample_for_per, erl_td3_update_f32, tree update per step"
    # the one-launch rollout / evaluation and the tile action (erl_td3_rollout_*, erl_td3_eval_*, erl_td3_explore_action_tile_f32): opt-in
    # -- args.fused_td3_rollout = True or ERL_FUSED_TD3_ROLLOUT=1 (tools/td3_rollout_ab.py writes profiles/td3_rollout_ab.txt); off, the
    # rollout and the evaluation are the per-step loops on erl_td3_explore_action_f32.  The tile kernel sums a layer in another order
    # than the layered path, so the switch changes a run's bits within the tolerance either has against fp64.
    _fused_td3_rollout_default = "0"

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
        self.fused_td3_rollout = bool(getattr(args, "fused_td3_rollout",
                                              os.environ.get("ERL_FUSED_TD3_ROLLOUT", self._fused_td3_rollout_default) != "0"))
        # with the switch on, device-resident envs that offer it: the whole off-policy rollout as one launch (False: the per-step loop)
        self.fused_rollout = bool(getattr(args, "fused_rollout", True))
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
        if self.fused_td3_rollout:
            why = self._one_launch_agent_reason()
            self.kernel_path += ("; rollout: one launch on device-resident envs, and so the evaluation (erl_td3_rollout_*, erl_td3_eval_*), "
                                 "per-step action on the tile kernel (erl_td3_explore_action_tile_f32)" if why is None else
                                 "; rollout: per-step loop: " + why)
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
        """Actor.get_action(state, explore_noise_std) (erl_td3_explore_action_f32: the layered path; with `fused_td3_rollout` and inside
        its shapes erl_td3_explore_action_tile_f32: one launch); `noise` (n, action_dim) injects the draw, else Philox keyed by (rng_seed,
        rng_counter, row, component).  `out` (n, action_dim) / `out_state` (n, state_dim), contiguous: the kernel writes the action / a
        copy of `state` there (the rollout passes its buffer rows: no copies)"""
        from .. import ops
        self._sync_modules()
        action = ops.td3_explore_action(self._spec, self._actor_flat, state.contiguous(), self.explore_noise_std,
                                        noise=None if noise is None else noise.contiguous(), seed=self.rng_seed, counter=self.rng_counter,
                                        out=out, out_state=out_state, tile=self._tile_action_reason(state.shape[0]) is None)
        self.rng_counter += 1
        return action

    _SWITCH_OFF = "args.fused_td3_rollout is off (ERL_FUSED_TD3_ROLLOUT; profiles/td3_rollout_ab.txt)"

    def _shape_reason(self, n_rows: int, what: str) -> Optional[str]:
        """None when the deterministic-actor tile kernels cover this actor on `n_rows` rows, else why not"""
        sp = self._spec
        if _hip.lib().erl_td3_rollout_supported(sp.S, sp.A, sp._c, len(sp.hidden), int(n_rows)):
            return None
        return f"S={sp.S} A={sp.A} net_dims={list(self.net_dims)} rows={n_rows} outside {what}'s shapes"

    def _one_launch_agent_reason(self) -> Optional[str]:
        if not self.fused_td3_rollout:
            return self._SWITCH_OFF
        if not self.fused_rollout:
            return "args.fused_rollout is off (the persistent rollout and its evaluation form go together)"
        return self._shape_reason(self.num_envs, "the persistent off-policy rollout")

    def _tile_action_reason(self, n_rows: int) -> Optional[str]:
        """None when `explore_action` on `n_rows` states is erl_td3_explore_action_tile_f32 (the per-step twin of the one-launch rollouts),
        else why it is the layered erl_td3_explore_action_f32"""
        if not self.fused_td3_rollout:
            return self._SWITCH_OFF
        return self._shape_reason(n_rows, "the tile kernel")

    def _loop_path(self, n_rows: int, env_call: str, why: str) -> str:
        tile_why = self._tile_action_reason(n_rows)
        if tile_why is None:
            return f"per-step loop (tile action erl_td3_explore_action_tile_f32 + {env_call} per step): {why}"
        return f"per-step loop (erl_td3_explore_action_f32 + {env_call} per step): {why if why == tile_why else why + '; ' + tile_why}"

    @_hip.on_device
    def _explore_vec_env(self, env, horizon_len: int, noise: Optional[TEN] = None) -> Tuple[TEN, ...]:
        """AgentBase._explore_vec_env (AgentBase.py:130-170).  With `fused_td3_rollout`, on a device-resident env that offers
        `fused_rollout_offpolicy`, the whole loop is ONE launch (erl_td3_rollout_*_f32: the five tensors, the final state and the env's
        counters of the per-step loop on the tile action, bit for bit; `args.fused_rollout = False` keeps the loop).  Else a per-step loop
        on any env of the vector protocol (`step_into` where the env has it): one explore_action launch writes the action and the state
        row, then the env steps.  `rollout_path` says which route ran and, for the loop, why."""
        H, N, S, A, dev = horizon_len, self.num_envs, self.state_dim, self.action_dim, self.device
        why = self._one_launch_reason(env, "fused_rollout_offpolicy")
        if why is not None:
            self._last_state_token = None
            self.rollout_path = self._loop_path(N, f"env.{'step_into' if hasattr(env, 'step_into') else 'step'}", why)
            return super()._explore_vec_env(env, horizon_len, noise)
        self.rollout_path = f"one launch (erl_td3_rollout_*_f32 through {type(env).__name__}.fused_rollout_offpolicy)"
        self._sync_modules()
        state = self.last_state.to(dev, th.float32)
        assert state.shape == (N, S)
        self._hand_state_to_env(env, state)
        states = th.empty((H, N, S), dtype=th.float32, device=dev)
        actions = th.empty((H, N, A), dtype=th.float32, device=dev)
        rewards = th.empty((H, N), dtype=th.float32, device=dev)
        undones = th.empty((H, N), dtype=th.bool, device=dev)
        unmasks = th.empty((H, N), dtype=th.bool, device=dev)
        last_out = th.empty((N, S), dtype=th.float32, device=dev)
        env.fused_rollout_offpolicy(self, H, None if noise is None else noise.contiguous(), (states, actions, rewards, undones, unmasks), last_out)
        self.rng_counter += H
        self._record_last_state(env, last_out)
        return states, actions, rewards, undones, unmasks

    @_hip.on_device
    def _explore_one_env(self, env, horizon_len: int) -> Tuple[TEN, ...]:
        self.rollout_path = self._loop_path(1, "env.step", "one numpy env")
        return super()._explore_one_env(env, horizon_len)

    def _fused_eval_reason(self, env) -> Optional[str]:
        """None when `evaluate_env(env)` runs the fused evaluation, else why not"""
        return self._one_launch_reason(env, "fused_evaluate_offpolicy")

    @_hip.on_device
    def evaluate_env(self, env) -> Optional[TEN]:
        """AgentBase.evaluate_env on the persistent rollout's evaluation form (erl_td3_eval_*_f32): env.reset(), env.max_step steps of
        Actor.forward in one launch, the episode table from a second; None outside its shapes or with `fused_td3_rollout` off."""
        if self._fused_eval_reason(env) is not None:
            return None
        self._sync_modules()
        return self._evaluate_env_fused(env, lambda ws: env.fused_evaluate_offpolicy(self, int(env.max_step), ws))

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
