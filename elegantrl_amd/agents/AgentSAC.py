"""`AgentSAC` on the HIP path (BASELINE config 3): off-policy rollout feeding `ReplayBuffer.update` (reference
`AgentBase._explore_vec_env`, elegantrl/agents/AgentBase.py:130-170), and the update loop around `ReplayBuffer.sample`
(`AgentBase.update_net` :172-189 + `AgentSAC.update_objectives`, elegantrl/agents/AgentSAC.py:42-86).

Everything numerical runs in liberl_hip.so: ring write / sample are K8 / K9, the exploration action is
`erl_sac_explore_action_f32` and the whole update step after the sample -- tanh-Gaussian actor, critic ensemble, target
min, temperature, soft update, three clip + Adam steps -- is ONE `erl_sac_update_f32` call (csrc/sac.hip).  The
`nn.Module`s below only describe the parameter layout (their tensors are views into the flat blocks the kernels
read/write) and serve the Evaluator's `actor(state)` / checkpoints.  No torch fallback for the update math: the torch
restatement lives in oracle/sac_torch.py as test infrastructure.

Quirks of the reference are reproduced (see csrc/sac.hip): log-prob evaluated at the Gaussian MEAN (:197), tanh correction
`log(1 - tanh^2 + 1e-6)` (:198), actor trained against the TARGET ensemble mean (:83), alpha clamped after its own step.
"""
from __future__ import annotations

import math
import os
from copy import deepcopy
from typing import List, Optional, Tuple

import torch as th
from torch import nn

from .. import _hip
from ..train.config import Config
# (_FlatAdamState: checkpoints written before it moved pickle it under this module's path)
from .AgentBase import _FlatAdamState, _OffPolicyFlatAgent, build_mlp, layer_init_with_orthogonal

TEN = th.Tensor


class ActorSAC(nn.Module):
    """state -> encoder MLP (GELU after every layer) -> linear head -> (mean, log_std); action = tanh(mean + std * eps)."""

    def __init__(self, net_dims: List[int], state_dim: int, action_dim: int):
        super().__init__()
        self.state_dim, self.action_dim = state_dim, action_dim
        self.net_s = build_mlp(dims=[state_dim, *net_dims], if_raw_out=False)
        self.net_a = build_mlp(dims=[net_dims[-1], action_dim * 2])
        layer_init_with_orthogonal(self.net_a[-1], std=0.1)

    def _head(self, state: TEN) -> Tuple[TEN, TEN]:
        mean, log_std = self.net_a(self.net_s(state)).chunk(2, dim=1)
        return mean, log_std.clamp(-16, 2).exp()

    def forward(self, state: TEN) -> TEN:
        return self.net_a(self.net_s(state))[:, :self.action_dim].tanh()

    def get_action(self, state: TEN, noise: Optional[TEN] = None) -> TEN:
        mean, std = self._head(state)
        eps = th.randn_like(mean) if noise is None else noise
        return (mean + std * eps).tanh()                       # Normal(mean, std).rsample().tanh()

    def get_action_logprob(self, state: TEN, noise: Optional[TEN] = None) -> Tuple[TEN, TEN]:
        mean, std = self._head(state)
        eps = th.randn_like(mean) if noise is None else noise
        action_tanh = (mean + std * eps).tanh()
        logprob = -std.log() - math.log(math.sqrt(2 * math.pi))          # Normal.log_prob evaluated at the mean (:197)
        logprob = logprob - (-action_tanh.pow(2) + 1.000001).log()       # tanh correction (:198)
        return action_tanh, logprob.sum(1)


class ActorFixSAC(nn.Module):
    """AgentModSAC's actor (elegantrl/agents/AgentSAC.py:201-243): encoder build_mlp([S, *net_dims]) whose LAST layer is raw, two
    one-layer decoders for the mean and the log-std (clamped to [-20, 2]), the log-prob AT the sample with the tanh correction in its
    softplus form.  The training path does not call these methods (kernels on the flat block: csrc/sac.hip, ERL_SAC_ACTOR_FIX)."""

    def __init__(self, net_dims: List[int], state_dim: int, action_dim: int):
        super().__init__()
        self.state_dim, self.action_dim = state_dim, action_dim
        self.encoder_s = build_mlp(dims=[state_dim, *net_dims])
        self.decoder_a_avg = build_mlp(dims=[net_dims[-1], action_dim])
        self.decoder_a_std = build_mlp(dims=[net_dims[-1], action_dim])
        self.soft_plus = nn.Softplus()
        layer_init_with_orthogonal(self.decoder_a_avg[-1], std=0.1)
        layer_init_with_orthogonal(self.decoder_a_std[-1], std=0.1)

    def forward(self, state: TEN) -> TEN:
        return self.decoder_a_avg(self.encoder_s(state)).tanh()

    def get_action(self, state: TEN, noise: Optional[TEN] = None, **_kwargs) -> TEN:
        tmp = self.encoder_s(state)
        avg, std = self.decoder_a_avg(tmp), self.decoder_a_std(tmp).clamp(-20, 2).exp()
        eps = th.randn_like(avg) if noise is None else noise
        return (avg + std * eps).tanh()

    def get_action_logprob(self, state: TEN, noise: Optional[TEN] = None) -> Tuple[TEN, TEN]:
        tmp = self.encoder_s(state)
        log_std = self.decoder_a_std(tmp).clamp(-20, 2)
        avg = self.decoder_a_avg(tmp)
        eps = th.randn_like(avg) if noise is None else noise
        action = avg + log_std.exp() * eps
        logprob = -log_std - eps.pow(2) * 0.5 - math.log(math.sqrt(2 * math.pi))
        logprob = logprob - (math.log(2.) - action - self.soft_plus(-2. * action)) * 2.
        return action.tanh(), logprob.sum(1)


class CriticEnsemble(nn.Module):
    """shared (state, action) encoder layer + `num_ensembles` independent Q decoders; forward = ensemble mean."""

    def __init__(self, net_dims: List[int], state_dim: int, action_dim: int, num_ensembles: int = 4):
        super().__init__()
        self.state_dim, self.action_dim = state_dim, action_dim
        self.encoder_sa = build_mlp(dims=[state_dim + action_dim, net_dims[0]])
        self.decoder_qs = []
        for i in range(num_ensembles):
            dec = build_mlp(dims=[*net_dims, 1])
            layer_init_with_orthogonal(dec[-1], std=0.5)
            self.decoder_qs.append(dec)
            setattr(self, f"decoder_q{i:02}", dec)              # registers the parameters under the reference's names

    def get_q_values(self, state: TEN, action: TEN) -> TEN:
        enc = self.encoder_sa(th.cat((state, action), dim=1))
        return th.cat([dec(enc) for dec in self.decoder_qs], dim=-1)

    def forward(self, state: TEN, action: TEN) -> TEN:
        return self.get_q_values(state, action).mean(dim=-1, keepdim=True)


class AgentSAC(_OffPolicyFlatAgent):
    _actor_class = ActorSAC
    _actor_variant = _hip.SAC_ACTOR_SAC
    _default_ensembles = 4
    _ring_loop_path = "one C call (erl_sac_update_ring_loop_f32: the sample inside every step's first launch)"
    _per_why = "prioritised replay (per_path names its route)"

    def __init__(self, net_dims: List[int], state_dim: int, action_dim: int, gpu_id: int = 0, args: Config = None):
        args = Config() if args is None else args
        super().__init__(net_dims, state_dim, action_dim, gpu_id, args)
        if self.if_discrete:
            raise NotImplementedError("SAC is a continuous-action agent")
        # (without a GPU the agent can still be constructed, to read `kernel_path`; it runs on the HIP kernels only and there is no CPU
        # fallback: its first kernel call raises HipExtensionError, _hip.ptr)
        from .. import ops
        self.num_ensembles = getattr(args, "num_ensembles", self._default_ensembles)
        # update_net draws the sample ids of all its steps with one th.randint (False: one draw per step, the reference's call pattern)
        self.sample_ids_ahead = bool(getattr(args, "sample_ids_ahead", True))
        # device-resident envs that offer it: the whole off-policy rollout as one launch (False: the per-step loop)
        self.fused_rollout = bool(getattr(args, "fused_rollout", True))
        # update_net hands the replay ring + the drawn ids to the step instead of sampling first (False: sample, then step)
        self.sample_in_step = bool(getattr(args, "sample_in_step", os.environ.get("ERL_SAC_SAMPLE_IN_STEP", "1") != "0"))
        # round 6: with the sample inside the step, update_net's whole loop is ONE C call (erl_sac_update_ring_loop_f32): bit-identical to the
        # per-step calls; `args.update_loop_in_c = False` / ERL_SAC_LOOP_IN_C=0 keeps one call per step
        self.update_loop_in_c = bool(getattr(args, "update_loop_in_c", os.environ.get("ERL_SAC_LOOP_IN_C", "1") != "0"))
        # prioritised replay: update_net's whole loop is ONE C call as well (erl_sac_update_per_loop_f32: draw + gather, step, tree update per
        # step, bit-identical to the per-step calls on the same uniforms); `args.per_loop_in_c = False` / ERL_SAC_PER_LOOP_IN_C=0 keeps
        # _per_step's six host-driven calls per step
        self.per_loop_in_c = bool(getattr(args, "per_loop_in_c", os.environ.get("ERL_SAC_PER_LOOP_IN_C", "1") != "0"))
        # the prioritised loop's draw + gather inside every step's first launch (erl_sac_update_per_draw_loop_f32, AgentModSAC:
        # erl_sac_update_mod_per_loop_f32 with draw_in_step) instead of one erl_per_sample_rows_f32 launch per step: bit-identical, fused step
        # only; opt-in -- args.per_draw_in_step = True or ERL_SAC_PER_DRAW_IN_STEP=1 -- until profiles/sac_per_loop_ab.txt shows the win
        # DESIGN.md section 9 asks of a default
        self.per_draw_in_step = bool(getattr(args, "per_draw_in_step", os.environ.get("ERL_SAC_PER_DRAW_IN_STEP", "0") != "0"))
        self.fused_mod_rollout = False             # AgentModSAC's switch for the ActorFixSAC forms of the rollout launches (_variant_kernel_path)
        self._spec = ops.SacSpec(state_dim, action_dim, net_dims, self.num_ensembles, actor_variant=self._actor_variant)
        dev, f32 = self.device, th.float32
        self._actor_flat = th.zeros(self._spec.actor_count, dtype=f32, device=dev)
        self._critic_flat = th.zeros(self._spec.critic_count, dtype=f32, device=dev)
        self._target_flat = th.zeros(self._spec.critic_count, dtype=f32, device=dev)
        act = self._actor_class(net_dims, state_dim, action_dim).to(dev)
        cri = CriticEnsemble(net_dims, state_dim, action_dim, num_ensembles=self.num_ensembles).to(dev)
        cri_target = deepcopy(cri)
        self._bind("_act", act, self._spec.actor_slices(), self._actor_flat)
        self._bind("cri", cri, self._spec.critic_slices(), self._critic_flat)
        self._bind("cri_target", cri_target, self._spec.critic_slices(), self._target_flat)
        self.act_optimizer = _FlatAdamState(self._spec.actor_count, self.learning_rate, dev)
        self.cri_optimizer = _FlatAdamState(self._spec.critic_count, self.learning_rate, dev)
        self.alpha_optim = _FlatAdamState(1, self.learning_rate, dev)
        self.alpha_log = th.full((1,), -1.0, dtype=f32, device=dev)
        self.target_entropy = math.log(action_dim)               # np.log(action_dim), as the reference (:31)
        self.save_attr_names = self.save_attr_names | {"alpha_log", "alpha_optim"}
        import ctypes as _ct
        hid = (_ct.c_int * len(net_dims))(*[int(h) for h in net_dims])
        fused_ok = (not self._actor_variant and len(net_dims) == 2 and os.environ.get("ERL_SAC_FUSED", "1") != "0"
                    and bool(_hip.lib().erl_sac_rollout_synenv_supported(state_dim, action_dim, hid, len(net_dims), 16)))
        self.kernel_path = ("fused SAC step (two hidden layers <= 256 wide, S + A <= 64, A <= 8, batch <= 4096: tile kernels, sample inside the step's "
                            "first launch, one-launch rollout on device-resident envs)" if fused_ok else
                            "layered SAC step (one MFMA GEMM launch per dense layer): " +
                            ("ActorFixSAC / two-time-scale options (AgentModSAC)" if self._actor_variant else
                             f"net_dims {list(net_dims)}, state_dim {state_dim}, action_dim {action_dim} outside the fused step's shapes"))
        if self._actor_variant:
            self.kernel_path = self._variant_kernel_path(args)
        if not getattr(args, "quiet", False) and os.environ.get("ERL_QUIET", "0") == "0":
            print(f"| {type(self).__name__}: {self.kernel_path}", flush=True)

    def _optimizers(self) -> tuple:
        return self.act_optimizer, self.cri_optimizer, self.alpha_optim

    def _checkpoint_extras(self, if_save: bool):
        """beyond the reference's file set a resumed SAC run needs the temperature and its optimiser state (`alpha_log`, `alpha_optim`:
        save_attr_names)"""
        if not if_save:
            self.alpha_log = self.alpha_log.to(self.device, th.float32).contiguous()

    @_hip.on_device
    def _explore_vec_env(self, env, horizon_len: int, noise: Optional[TEN] = None) -> Tuple[TEN, ...]:
        """AgentBase._explore_vec_env (AgentBase.py:130-170); on a device-resident env that offers `fused_rollout_offpolicy` (SynVecEnv) the
        whole loop is ONE launch (erl_sac_rollout_synenv_f32: same five tensors, final state and env counters, bit for bit, as the
        per-step loop; `args.fused_rollout = False` keeps the loop).  `rollout_path` says which route ran and, for the loop, why."""
        H, N, S, A, dev = horizon_len, self.num_envs, self.state_dim, self.action_dim, self.device
        why = self._one_launch_reason(env, "fused_rollout_offpolicy")
        if why is not None:
            self._last_state_token = None
            self.rollout_path = f"per-step loop ({self._explore_action_route(N)} + env.step per step): {why}"
            return super()._explore_vec_env(env, horizon_len, noise)
        self.rollout_path = (f"one launch ({'erl_sac_rollout_mod_' if self._actor_variant else 'erl_sac_rollout_'}*_f32 through "
                             f"{type(env).__name__}.fused_rollout_offpolicy)")
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

    def _one_launch_agent_reason(self) -> Optional[str]:
        if self._actor_variant and not self.fused_mod_rollout:
            return ("ActorFixSAC (AgentModSAC) has no persistent rollout unless args.fused_mod_rollout is on (ERL_FUSED_MODSAC_ROLLOUT; "
                    "profiles/modsac_rollout_ab.txt)")
        if not self.fused_rollout:
            return "args.fused_rollout is off (the persistent rollout and its evaluation form go together)"
        sp = self._spec
        supported = _hip.lib().erl_sac_rollout_mod_supported if self._actor_variant else _hip.lib().erl_sac_rollout_synenv_supported
        if not supported(sp.S, sp.A, sp._c, len(sp.hidden), self.num_envs):
            return f"S={sp.S} A={sp.A} net_dims={list(self.net_dims)} N={self.num_envs} outside the persistent off-policy rollout's shapes"
        return None

    def _tile_action_reason(self, n_rows: int) -> Optional[str]:
        """None when `explore_action` on `n_rows` states is erl_sac_explore_action_tile_f32 (the per-step twin of the one-launch rollouts),
        else why it is erl_sac_explore_action_f32 / _opt_f32 with their own routes"""
        if not self._actor_variant:
            return "ActorSAC: erl_sac_explore_action_f32 picks the tile kernel itself"
        if not self.fused_mod_rollout:
            return "args.fused_mod_rollout is off"
        sp = self._spec
        if not _hip.lib().erl_sac_rollout_mod_supported(sp.S, sp.A, sp._c, len(sp.hidden), int(n_rows)):
            return f"S={sp.S} A={sp.A} net_dims={list(self.net_dims)} rows={n_rows} outside the tile kernel's shapes"
        return None

    def _explore_action_route(self, n_rows: int) -> str:
        if self._tile_action_reason(n_rows) is None:
            return "tile action erl_sac_explore_action_tile_f32"
        return "erl_sac_explore_action_opt_f32" if self._actor_variant else "erl_sac_explore_action_f32"

    def _fused_eval_reason(self, env) -> Optional[str]:
        """None when `evaluate_env(env)` runs the fused evaluation, else why not"""
        return self._one_launch_reason(env, "fused_evaluate_offpolicy")

    @_hip.on_device
    def evaluate_env(self, env) -> Optional[TEN]:
        """AgentBase.evaluate_env on the persistent off-policy rollout's evaluation form (erl_sac_eval_synenv_f32 / erl_sac_eval_pendulum_f32;
        AgentModSAC with `fused_mod_rollout`: erl_sac_eval_mod_*): env.reset(), env.max_step steps of the actor's `forward` in one launch,
        the episode table from a second; None outside its shapes."""
        if self._fused_eval_reason(env) is not None:
            return None
        self._sync_modules()
        return self._evaluate_env_fused(env, lambda ws: env.fused_evaluate_offpolicy(self, int(env.max_step), ws))

    @_hip.on_device
    def explore_action(self, state: TEN, noise: Optional[TEN] = None, out: Optional[TEN] = None, out_state: Optional[TEN] = None) -> TEN:
        """`out` (n, action_dim), contiguous: the kernel writes the action there (the rollout passes its buffer row: no copy);
        `out_state` (n, state_dim), contiguous: the kernel also copies `state` there (the rollout's `states[t] = state`)"""
        from .. import ops
        self._sync_modules()
        action = ops.sac_explore_action(self._spec, self._actor_flat, state.contiguous(), noise=noise, seed=self.rng_seed,
                                        counter=self.rng_counter, out=out, out_state=out_state,
                                        tile=self._tile_action_reason(state.shape[0]) is None)
        self.rng_counter += 1
        return action

    def _nets(self) -> tuple:
        """the leading arguments of every ops.sac_update* call"""
        return (self._spec, self._actor_flat, self._critic_flat, self._target_flat, self.alpha_log, self._moments())

    def _moments(self) -> tuple:
        return (self.act_optimizer.exp_avg, self.act_optimizer.exp_avg_sq, self.cri_optimizer.exp_avg, self.cri_optimizer.exp_avg_sq,
                self.alpha_optim.exp_avg, self.alpha_optim.exp_avg_sq)

    def _hyper(self) -> dict:
        return dict(gamma=float(self.gamma), target_entropy=float(self.target_entropy), tau=float(self.soft_update_tau),
                    lr=float(self.learning_rate), max_norm=float(self.clip_grad_norm), criterion=self.criterion_code)

    def _set_step_counts(self):
        """the optimisers' `step_count` after a step (th.optim.Adam's own count, what a checkpoint stores)"""
        self.act_optimizer.step_count = self.cri_optimizer.step_count = self.alpha_optim.step_count = self._step

    def _update_from_ring(self, buffer, ring, ids: TEN, objs_out: TEN, noises=None, update_t: int = 0):
        """ReplayBuffer.sample(ids) and the step from one C call; the buffer's stage / ids0 / ids1 end up as after `buffer.sample`"""
        from .. import ops
        self._step += 1
        arrays, sample_len, stage = ring
        ops.sac_update_from_ring(*self._nets(), arrays, ids, sample_len, stage, self._step, **self._hyper(), objs_out=objs_out, noises=noises,
                                 seed=self.rng_seed + 1, counter=self._step)
        buffer.ids0, buffer.ids1 = stage.ids
        self._set_step_counts()

    def _step_options(self, update_t: int) -> dict:
        """extra keyword arguments of ops.sac_update for this step (AgentModSAC: its two-time-scale rule and actor target)"""
        return {}

    def _variant_kernel_path(self, args) -> str:
        """`kernel_path` of an agent whose actor is not ActorSAC"""
        return self.kernel_path

    def _variant_per_loop_reason(self) -> Optional[str]:
        """why this agent class keeps a prioritised update_net on _per_step whatever the buffer offers (None: it does not)"""
        return None

    def _variant_ring_step_reason(self) -> Optional[str]:
        """None when this agent class's step takes the replay sample inside its first launch (the ring forms), else why not"""
        return "ActorFixSAC / two-time-scale options take the layered step, which reads a finished batch" if self._actor_variant else None

    def _ring_step_reason(self) -> Optional[str]:
        # the sample rides in the step's first launch (erl_sac_update_ring_f32) where nothing needs ids0 / ids1 before the step
        return ("args.sample_ids_ahead is off" if not self.sample_ids_ahead else
                "args.sample_in_step is off" if not self.sample_in_step else
                "lambda_fit_cum_r needs ids0 / ids1 on the host side of every step" if self.lambda_fit_cum_r else
                self._variant_ring_step_reason())

    def _ring_loop_reason(self, buffer, ring) -> Optional[str]:
        if not ring:
            return f"{type(buffer).__name__} offers no continuous-action ring of >= 2 rows for the sample inside the step"
        return None if self.update_loop_in_c else "args.update_loop_in_c is off"

    def _update_ring_loop(self, buffer, ring, id_all: TEN, objs: TEN):
        """update_net's whole loop from ONE C call (erl_sac_update_ring_loop_f32, round 6): step t = what _update_from_ring(id_all[t])
        enqueues"""
        from .. import ops
        arrays, sample_len, stage = ring
        update_times = id_all.shape[0]
        ops.sac_update_ring_loop(*self._nets(), arrays, id_all, sample_len, stage, self._step + 1, **self._hyper(), objs_all=objs,
                                 seed=self.rng_seed + 1, counter0=self._step + 1)
        self._step += update_times
        buffer.ids0, buffer.ids1 = stage.ids
        self._set_step_counts()

    def _per_draw_why(self) -> Optional[str]:
        """None when the prioritised loop's draw + gather ride in every step's first launch, else why they are a launch of their own"""
        return self._per_draw_reason() if self.per_draw_in_step else "args.per_draw_in_step is off"

    def _per_loop_path(self) -> str:
        """`per_path` of the prioritised loop as one C call"""
        draw_why = self._per_draw_why()
        if draw_why is None:
            return ("prioritised update loop in one C call (erl_sac_update_per_draw_loop_f32: draw + gather inside the step's first launch, "
                    "tree update behind every step)")
        return ("prioritised update loop in one C call (erl_sac_update_per_loop_f32: draw + gather, step, tree update per step)" +
                (f"; args.per_draw_in_step ignored: {draw_why}" if self.per_draw_in_step else ""))

    def _update_per_loop(self, buffer, per, objs: TEN, per_uniform: Optional[TEN]):
        """the prioritised loop from ONE C call (erl_sac_update_per_loop_f32): step t = what _per_step enqueues on uniforms[t].  The
        uniforms of ALL the steps in one th.rand (sample_for_per draws (num_seqs, batch_size // num_seqs) per step: same distribution,
        same generator; the trees change inside the loop, the uniforms do not depend on them)"""
        from .. import ops
        p_ring, trees, cur_size, cursor, per_alpha, per_beta, stage, per_stage = per
        update_times = objs.shape[0]
        per_uniform = self._per_uniforms(buffer, update_times, per_uniform)
        loop = ops.sac_update_per_loop if self._per_draw_why() else ops.sac_update_per_draw_loop
        loop(*self._nets(), p_ring, trees, per_uniform, cur_size, cursor, per_alpha, per_beta, stage, per_stage, self._step + 1, **self._hyper(),
             objs_all=objs, seed=self.rng_seed + 1, counter0=self._step + 1)
        self._step += update_times
        buffer.ids0, buffer.ids1 = stage.ids
        self._td_error = per_stage.td_error
        self._set_step_counts()

    def _per_uniforms(self, buffer, update_times: int, per_uniform: Optional[TEN]) -> TEN:
        """the prioritised sampler's uniforms of a whole loop, (update_times, num_seqs, batch_size // num_seqs), drawn here unless injected"""
        shape = (update_times, buffer.num_seqs, self.batch_size // buffer.num_seqs)
        if per_uniform is None:
            per_uniform = th.rand(shape, dtype=th.float32, device=self.device)
        assert per_uniform.shape == shape
        return per_uniform.contiguous()

    def _per_draw_reason(self) -> Optional[str]:
        """None when the prioritised loop's step is the fused one, whose first launch can draw and gather, else why it cannot"""
        from .. import ops
        if os.environ.get("ERL_SAC_FUSED", "1") == "0":
            return "ERL_SAC_FUSED=0: the layered step reads a finished batch (the stand-alone draw runs)"
        if not ops.sac_mod_fused_supported(self._spec, int(self.batch_size)):
            return (f"net_dims {list(self.net_dims)}, batch {int(self.batch_size)} take the layered step, which reads a finished batch (the "
                    "stand-alone draw runs)")
        return None

    def _update_on_batch(self, batch, objs_out: TEN, noises=None, is_weight=None, td_error_out=None, buffer=None, update_t: int = 0):
        from .. import ops
        self._step += 1
        cum_reward = None
        if self.lambda_fit_cum_r:          # AgentSAC.py:66-68: the sampled transitions' n-step returns (the sampler left ids0 / ids1)
            cum_reward = buffer.cum_rewards[buffer.ids0, buffer.ids1].to(th.float32).contiguous()
        ops.sac_update(*self._nets(), batch, self._step, **self._hyper(), objs_out=objs_out, noises=noises, seed=self.rng_seed + 1,
                       counter=self._step, is_weight=is_weight, td_error_out=td_error_out, cum_reward=cum_reward,
                       lambda_fit_cum_r=float(self.lambda_fit_cum_r or 0.0), **self._step_options(update_t))
        self._set_step_counts()

    def _step_kwargs(self, buffer, update_t: int, noise=None) -> dict:
        """`noise` = (eps for next_state, eps for state) injects the step's draws (AgentSAC.py:42-86)"""
        return dict(noises=noise, update_t=update_t)

    def _per_loop_reason(self, buffer) -> Optional[str]:
        """None when a prioritised update_net runs as one C call, else why it takes one _per_step per step"""
        if not self.per_loop_in_c:
            return "args.per_loop_in_c is off"
        if not self.update_loop_in_c:
            return "args.update_loop_in_c is off"
        if self.lambda_fit_cum_r:
            return "lambda_fit_cum_r needs ids0 / ids1 on the host side of every step"
        why = self._variant_per_loop_reason()
        if why is not None:
            return why
        if not getattr(buffer, "per_for_fused_loop", None):
            return f"{type(buffer).__name__} has no per_for_fused_loop"
        return None

    def _per_route(self, buffer) -> tuple:
        why = self._per_loop_reason(buffer)
        per = None if why else buffer.per_for_fused_loop(self.batch_size)
        if per:
            return self._per_loop_path(), per
        return "prioritised update loop per step (_per_step: six host-driven calls): " + (
            why or "the buffer is not an interleaved continuous-action ring of >= 2 rows, or batch_size is no multiple of num_seqs"), None

    def _before_update_net(self, buffer):
        if self.lambda_fit_cum_r:                     # AgentBase.py:176-177 (bootstraps with the current actor: see get_cumulative_rewards)
            buffer.update_cum_rewards(get_cumulative_rewards=self.get_cumulative_rewards)


class AgentModSAC(AgentSAC):
    """Modified SAC (elegantrl/agents/AgentSAC.py:89-165): ActorFixSAC, 8 critics, `target_entropy = -log(action_dim)`, an actor target
    that follows the actor by soft updates, and the "auto two-time-scale update rule": the actor is updated on a step only while
    `update_a / (update_t + 1) < 1 / (2 - reliable_lambda)`, `reliable_lambda = exp(-critic_value ** 2)` (the reference never moves
    `critic_value` off 1.0, so this is 0.61: the actor skips roughly every third step).  The step is erl_sac_update_opt_f32 (csrc/sac.hip,
    layered path; ErlSacOptions carries what differs from AgentSAC) or, with `fused_step` on and inside the fused step's shapes,
    erl_sac_update_mod_f32 (csrc/sac_fused.hip: AgentSAC's tile kernels with ActorFixSAC as a run-time variant); update_net's loop on the
    fused step is one erl_sac_update_mod_ring_loop_f32 call; with prioritised replay (`if_use_per`, the reference's own PER demo) it is
    AgentSAC._per_step per step unless `mod_per_loop_in_c` is on, then one erl_sac_update_mod_per_loop_f32 call (fused step only; with
    `per_draw_in_step` the draw and the gather ride in every step's first launch); `per_path` names the route.  With `fused_mod_rollout` on and inside the same shapes, `explore_action` is the
    tile kernel (erl_sac_explore_action_tile_f32) and, on SynVecEnv / PendulumVecEnv with `fused_rollout`, `explore_env` and `evaluate_env` are
    one launch each (erl_sac_rollout_mod_*, erl_sac_eval_mod_*: csrc/sac_fused.hip sac_rollout_synenv_kernel<.., FIX>); `rollout_path` names
    the route the last rollout took."""
    _actor_class = ActorFixSAC
    _actor_variant = _hip.SAC_ACTOR_FIX
    _default_ensembles = 8
    _ring_loop_path = "one C call (erl_sac_update_mod_ring_loop_f32: the sample inside every step's first launch, the two-time-scale rule in C)"
    # the fused step against the layered one has no A/B record yet (tools/modsac_update_ab.py writes profiles/modsac_update_ab.txt): until
    # it has, the route is opt-in -- args.fused_step = True or ERL_FUSED_MODSAC_STEP=1
    _fused_step_default = "0"
    # the one-launch rollout / evaluation and the tile action (erl_sac_rollout_mod_*, erl_sac_eval_mod_*, erl_sac_explore_action_tile_f32):
    # opt-in as well -- args.fused_mod_rollout = True or ERL_FUSED_MODSAC_ROLLOUT=1 (tools/modsac_rollout_ab.py writes
    # profiles/modsac_rollout_ab.txt); off, the rollout and the evaluation are the per-step loops on erl_sac_explore_action_opt_f32
    _fused_mod_rollout_default = "0"

    def __init__(self, net_dims: List[int], state_dim: int, action_dim: int, gpu_id: int = 0, args: Config = None):
        args = Config() if args is None else args
        super().__init__(net_dims, state_dim, action_dim, gpu_id, args)
        self.target_entropy = getattr(args, "target_entropy", -math.log(action_dim))      # (:107; AgentSAC: +log(action_dim))
        self.critic_tau = getattr(args, "critic_tau", 0.995)
        self.critic_value = 1.0                                  # for reliable_lambda (:110; never updated by the reference either)
        self.update_a = 0                                        # actor updates of the current update_net loop (:111)
        self._actor_step = 0                                     # the actor optimiser's own Adam step (it steps only when updated)
        self._actor_target_flat = self._actor_flat.clone()
        self._bind("act_target", deepcopy(self._act), self._spec.actor_slices(), self._actor_target_flat)
        self._last_actor_updated = True
        # a prioritised update_net as ONE C call (erl_sac_update_mod_per_loop_f32: the prioritised loop and the two-time-scale rule together,
        # bit-identical to _per_step on the fused step): opt-in -- args.mod_per_loop_in_c = True or ERL_SAC_MOD_PER_LOOP_IN_C=1 -- until
        # profiles/sac_per_loop_ab.txt shows the win DESIGN.md section 9 asks of a default; it needs the fused step (there is no layered form)
        self.mod_per_loop_in_c = bool(getattr(args, "mod_per_loop_in_c", os.environ.get("ERL_SAC_MOD_PER_LOOP_IN_C", "0") != "0"))

    def _fused_step_reason(self, batch_size: Optional[int] = None) -> Optional[str]:
        """None when a step on `batch_size` rows runs the fused ModSAC step (erl_sac_update_mod_*), else why it is layered.  Asked per call:
        `fused_step` can be flipped between calls (A/B runs alternate the two routes in one process)."""
        from .. import ops
        if not self.fused_step:
            return "args.fused_step is off (ERL_FUSED_MODSAC_STEP; profiles/modsac_update_ab.txt)"
        if os.environ.get("ERL_SAC_FUSED", "1") == "0":
            return "ERL_SAC_FUSED=0"
        if self.lambda_fit_cum_r:
            return "lambda_fit_cum_r: the critic's cumulative-reward term is layered only"
        B = int(self.batch_size if batch_size is None else batch_size)
        if not ops.sac_mod_fused_supported(self._spec, B):
            return (f"net_dims {list(self.net_dims)}, state_dim {self.state_dim}, action_dim {self.action_dim}, {self.num_ensembles} critics, "
                    f"batch {B} outside the fused step's shapes (two hidden layers, widths multiples of 16 up to 256, S + A <= 64, A <= 8, "
                    "<= 8 critics, batch <= 4096)")
        return None

    def _variant_kernel_path(self, args) -> str:
        # (called by the base constructor, which prints `kernel_path`)
        self.fused_step = bool(getattr(args, "fused_step", os.environ.get("ERL_FUSED_MODSAC_STEP", self._fused_step_default) != "0"))
        self.fused_mod_rollout = bool(getattr(args, "fused_mod_rollout",
                                              os.environ.get("ERL_FUSED_MODSAC_ROLLOUT", self._fused_mod_rollout_default) != "0"))
        why = self._fused_step_reason()
        if why is None:
            step = ("fused ModSAC step (erl_sac_update_mod_f32: AgentSAC's tile kernels with ActorFixSAC's raw second layer and head, skipped "
                    "actor steps end in one small launch, actor target in the actor's clip + Adam launch; update_net's loop is one C call)")
        else:
            step = "layered ModSAC step (erl_sac_update_opt_f32: one MFMA GEMM launch per dense layer): " + why
        why = self._one_launch_agent_reason()
        if why is None:
            return step + ("; rollout: one launch on device-resident envs, and so the evaluation (erl_sac_rollout_mod_*, erl_sac_eval_mod_*), "
                           "per-step action on the tile kernel (erl_sac_explore_action_tile_f32)")
        return step + "; rollout: per-step loop: " + why

    def _variant_ring_step_reason(self) -> Optional[str]:
        why = self._fused_step_reason()
        return None if why is None else "layered ModSAC step, which reads a finished batch: " + why

    def _set_step_counts(self):
        self.cri_optimizer.step_count = self.alpha_optim.step_count = self._step
        self.act_optimizer.step_count = self._actor_step         # (th.optim.Adam's own count: the actor steps only when it is updated)

    def _update_ring_loop(self, buffer, ring, id_all: TEN, objs: TEN):
        """update_net's whole loop from ONE C call (erl_sac_update_mod_ring_loop_f32): the two-time-scale rule is evaluated in C, exactly as
        _step_options does per step; afterwards the counters are what the per-step route would have left"""
        from .. import ops
        arrays, sample_len, stage = ring
        T = id_all.shape[0]
        n_upd = ops.sac_update_mod_ring_loop(*self._nets(), arrays, id_all, sample_len, stage, self._step + 1, self._actor_step,
                                             float(self.critic_value), **self._hyper(), objs_all=objs, actor_target=self._actor_target_flat,
                                             seed=self.rng_seed + 1, counter0=self._step + 1)
        self._count_loop(T, n_upd)
        buffer.ids0, buffer.ids1 = stage.ids
        self._set_step_counts()

    def _count_loop(self, T: int, n_upd: int):
        """the counters after a T-step loop in C that updated the actor n_upd times: the rule re-derived here as _step_options applies it
        per step (the last step's flag; the count must be the library's)"""
        bound, ua, do = 1 / (2 - math.exp(-self.critic_value ** 2)), 0, True
        for t in range(T):
            do = (ua / (t + 1)) < bound
            ua += do
        assert ua == n_upd, (ua, n_upd)
        self.update_a, self._last_actor_updated = n_upd, bool(do)
        self._actor_step += n_upd
        self._step += T

    def _variant_per_loop_reason(self) -> Optional[str]:
        if not self.mod_per_loop_in_c:
            return ("ActorFixSAC / two-time-scale options (AgentModSAC) are decided per step by the host unless args.mod_per_loop_in_c is on "
                    "(ERL_SAC_MOD_PER_LOOP_IN_C; profiles/sac_per_loop_ab.txt)")
        why = self._fused_step_reason()
        return None if why is None else "AgentModSAC's prioritised loop (erl_sac_update_mod_per_loop_f32) has no layered form: " + why

    def _per_loop_path(self) -> str:
        # (the step here is the fused one, _variant_per_loop_reason: per_draw_in_step is never ignored)
        return ("prioritised update loop in one C call (erl_sac_update_mod_per_loop_f32: " +
                ("draw + gather inside the step's first launch" if self.per_draw_in_step else "draw + gather, step") +
                ", tree update behind every step, the two-time-scale rule in C)")

    def _update_per_loop(self, buffer, per, objs: TEN, per_uniform: Optional[TEN]):
        """the prioritised loop from ONE C call (erl_sac_update_mod_per_loop_f32): step t = what _per_step enqueues on uniforms[t] with
        _step_options(t), the trees updated behind skipped actor steps too; afterwards the counters are what the per-step route leaves"""
        from .. import ops
        p_ring, trees, cur_size, cursor, per_alpha, per_beta, stage, per_stage = per
        T = objs.shape[0]
        per_uniform = self._per_uniforms(buffer, T, per_uniform)
        n_upd = ops.sac_update_mod_per_loop(*self._nets(), p_ring, trees, per_uniform, cur_size, cursor, per_alpha, per_beta, stage, per_stage,
                                            self._step + 1, self._actor_step, float(self.critic_value), **self._hyper(), objs_all=objs,
                                            actor_target=self._actor_target_flat, draw_in_step=self.per_draw_in_step, seed=self.rng_seed + 1,
                                            counter0=self._step + 1)
        self._count_loop(T, n_upd)
        buffer.ids0, buffer.ids1 = stage.ids
        self._td_error = per_stage.td_error
        self._set_step_counts()

    def _update_from_ring(self, buffer, ring, ids: TEN, objs_out: TEN, noises=None, update_t: int = 0):
        from .. import ops
        self._step += 1
        arrays, sample_len, stage = ring
        ops.sac_update_mod_from_ring(*self._nets(), arrays, ids, sample_len, stage, self._step, **self._hyper(), objs_out=objs_out,
                                     noises=noises, seed=self.rng_seed + 1, counter=self._step, **self._step_options(update_t))
        buffer.ids0, buffer.ids1 = stage.ids
        self._set_step_counts()

    def _step_options(self, update_t: int) -> dict:
        reliable_lambda = math.exp(-self.critic_value ** 2)
        self.update_a = 0 if update_t == 0 else self.update_a                           # (:150)
        do = (self.update_a / (update_t + 1)) < (1 / (2 - reliable_lambda))              # (:151)
        if do:
            self.update_a += 1
            self._actor_step += 1
        self._last_actor_updated = do
        return dict(update_actor=do, actor_step=max(1, self._actor_step), actor_target=self._actor_target_flat)

    def _update_on_batch(self, batch, objs_out: TEN, noises=None, is_weight=None, td_error_out=None, buffer=None, update_t: int = 0):
        if self._fused_step_reason(batch[0].shape[0]) is None:
            from .. import ops
            self._step += 1
            ops.sac_update_mod(*self._nets(), batch, self._step, **self._hyper(), objs_out=objs_out, noises=noises, seed=self.rng_seed + 1,
                               counter=self._step, is_weight=is_weight, td_error_out=td_error_out, **self._step_options(update_t))
            self._set_step_counts()
        else:
            super()._update_on_batch(batch, objs_out, noises, is_weight=is_weight, td_error_out=td_error_out, buffer=buffer, update_t=update_t)

    def _checkpoint_extras(self, if_save: bool):
        super()._checkpoint_extras(if_save)
        if if_save:      # the file keeps its layout: the actor optimiser's own count beside the update step
            self.act_optimizer.actor_step, self.act_optimizer.step_count = self._actor_step, self._step
        else:
            self._actor_step = int(getattr(self.act_optimizer, "actor_step", self._step))
