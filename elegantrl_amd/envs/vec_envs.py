"""GPU-resident vectorised environments implementing the reference's env protocol
(reset() -> (state, info); step(action) -> (state, reward, terminal, truncate, info); auto-reset;
attributes env_name, num_envs, max_step, state_dim, action_dim, if_discrete -- elegantrl/train/config.py:134-135,
elegantrl/envs/PointChasingEnv.py:84-182 as the in-tree exemplar).

They additionally expose `step_into(action, reward_row, terminal_row, truncate_row) -> state`, which lets the
rollout write step outputs straight into row t of its time-major buffers (no copies, no host sync).
The dynamics run in erl_synenv_step_f32 / erl_pendulum_step_f32 / erl_pointchasing_step_f32 (elegantrl_amd/csrc/envs.hip) and erl_cartpole_step_f32 /
erl_acrobot_step_f32 / erl_mountaincar_step_f32 (elegantrl_amd/csrc/rollout_discrete.hip).

Each family's base class owns every launch and leaves an env its constructor, `reset`, its entries' names and its live buffers:
_ContinuousGpuVecEnv (SynVecEnv, PendulumVecEnv, PointChasingVecEnv) and _DiscreteGpuVecEnv (CartPole, Acrobot, MountainCar).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch as th

from .. import _hip

TEN = th.Tensor


def _u64(x: int) -> int:
    """a Python int as the uint64 the C entries take (seeds and counters may be negative or beyond 64 bits)"""
    return x & (2 ** 64 - 1)


def _epilogue_args(epilogue):
    """the nine epilogue arguments of erl_rollout_*_f32 from (last_state_out, advantages, reward_sums, stats, workspace, gamma,
    lambda_gae, use_v_trace); all-NULL when there is none"""
    if epilogue is None:
        return None, None, None, None, None, 0, 0.0, 0.0, 0
    last, adv, ret, stats, ws, gamma, lam, vtrace = epilogue
    p, f32, f64 = _hip.ptr, th.float32, th.float64        # (None passes NULL)
    return (p(last, f32), p(adv, f32), p(ret, f32), p(stats, f64), p(ws, f64), 0 if ws is None else ws.numel() * 8, float(gamma), float(lam),
            int(bool(vtrace)))


def _discrete_epilogue_args(agent, epilogue):
    """the twelve arguments erl_rollout_discrete_*_gae_f32 takes behind the rollout entries' from `epilogue` = (values, next_value,
    advantages, reward_sums, partials, gamma, lambda_gae, use_v_trace) and the agent's critic"""
    values, next_value, adv, ret, parts, gamma, lam, vtrace = epilogue
    p, f32, c = _hip.ptr, th.float32, agent.cri
    return (p(agent._flat_c.flat, f32), p(c.state_avg.data, f32), p(c.state_std.data, f32), p(values, f32), p(next_value, f32), p(adv, f32),
            p(ret, f32), p(parts, th.float64), parts.numel() * 8, float(gamma), float(lam), int(bool(vtrace)))


class _GpuVecEnv:
    env_name = "GpuVecEnv"
    if_discrete = False

    def __init__(self, num_envs: int, state_dim: int, action_dim: int, max_step: int, gpu_id: int, seed: int):
        if not th.cuda.is_available() or gpu_id < 0:
            raise RuntimeError(f"{type(self).__name__} is GPU resident (HIP kernels); no device available for gpu_id={gpu_id}")
        self.device = th.device(f"cuda:{gpu_id}")
        self.num_envs, self.state_dim, self.action_dim, self.max_step = num_envs, state_dim, action_dim, max_step
        self.seed = int(seed)
        dev = self.device
        self.step_count = th.zeros(num_envs, dtype=th.int32, device=dev)
        self.episode = th.zeros(num_envs, dtype=th.int32, device=dev)
        self._reward = th.zeros(num_envs, dtype=th.float32, device=dev)
        self._terminal = th.zeros(num_envs, dtype=th.bool, device=dev)
        self._truncate = th.zeros(num_envs, dtype=th.bool, device=dev)
        # bumped whenever the live state changes (reset, any step): lets an agent that rolled this env out know whether its own
        # copy of the last state still IS the env's live state (AgentPPO._explore_vec_env skips the copy-back then)
        self.state_epoch = 0

    @_hip.on_device
    def step(self, action: TEN) -> Tuple[TEN, TEN, TEN, TEN, dict]:
        state = self.step_into(action.contiguous(), self._reward, self._terminal, self._truncate)
        return state.clone(), self._reward.clone(), self._terminal.clone(), self._truncate.clone(), {}

    def close(self):
        pass


def compact_episodes(workspace: TEN, num_envs: int, horizon_len: int, rows: TEN, count: TEN) -> None:
    """records + counts a `fused_evaluate*` launch left in `workspace` -> `rows` (capacity, 2) f32: (return, length) of every finished
    episode, env-major, time order inside an env; `count` (1,) int32: how many (erl_eval_episodes_compact_f32, one launch)"""
    _hip.check(_hip.lib().erl_eval_episodes_compact_f32(
        _hip.ptr(workspace, th.uint8), workspace.numel(), num_envs, horizon_len, _hip.ptr(rows, th.float32), rows.shape[0],
        _hip.ptr(count, th.int32), _hip.stream_ptr()), "erl_eval_episodes_compact_f32")


class _ContinuousGpuVecEnv(_GpuVecEnv):
    """what the device-resident continuous envs share: the per-step launch (erl_<stem>_step_f32, csrc/envs.hip) and the one-launch rollout /
    evaluation of a PPO agent (erl_rollout_<stem>_f32, erl_eval_<stem>_f32), of a SAC agent (erl_sac_rollout_[mod_]<stem>_f32,
    erl_sac_eval_[mod_]<stem>_f32) and of a TD3 / DDPG agent (erl_td3_rollout_<stem>_f32, erl_td3_eval_<stem>_f32).  An env adds its
    constructor, `reset`, the three attributes below and `_live`."""
    _stem = ""                              # "synenv" | "pendulum" | "pointchasing"
    _action_at = 0                          # how many of the live buffers the per-step entry takes in front of the action
    _takes_dims = False                     # the entries take state_dim and action_dim (else they fix them)

    def _live(self) -> Tuple[TEN, ...]:
        """the live buffers the C entries take, in their order (looked up per call: `reset` rebinds them)"""
        raise NotImplementedError

    def _dims(self, state_dim: int, action_dim: int) -> tuple:
        return (state_dim, action_dim) if self._takes_dims else ()

    def step_into(self, action: TEN, reward_row: TEN, terminal_row: TEN, truncate_row: TEN) -> TEN:
        from .. import ops
        self.state_epoch += 1
        live, k = self._live(), self._action_at
        getattr(ops, f"{self._stem}_step")(*live[:k], action, *live[k:], self.step_count, self.episode, reward_row, terminal_row, truncate_row,
                                           self.max_step, self.seed)
        return self.state

    def raw_stepper(self):
        """`step(action_ptr, reward_ptr, terminal_ptr, truncate_ptr, stream)` on raw device pointers (the rollout's per-step fast path: no
        tensor views, no argument checks); the live buffers are bound here, once (fixed addresses until the next `reset`)."""
        name = f"erl_{self._stem}_step_f32"
        fn = getattr(_hip.lib(), name)
        live = [t.data_ptr() for t in self._live()]
        head, mid = tuple(live[:self._action_at]), (*live[self._action_at:], self.step_count.data_ptr(), self.episode.data_ptr())
        tail = (self.num_envs, *self._dims(self.state_dim, self.action_dim), self.max_step, _u64(self.seed))

        def step(action_ptr, reward_ptr, terminal_ptr, truncate_ptr, stream):
            self.state_epoch += 1
            rc = fn(*head, action_ptr, *mid, reward_ptr, terminal_ptr, truncate_ptr, *tail, stream)
            if rc:
                _hip.check(rc, name)
        return step

    def _env_args(self):
        """the env block of the one-launch entries: live buffers, counters, max_step, env_seed, N"""
        return (*[_hip.ptr(t, th.float32) for t in self._live()], _hip.ptr(self.step_count, th.int32), _hip.ptr(self.episode, th.int32),
                self.max_step, _u64(self.seed), self.num_envs)

    def _ppo_args(self, agent, critic: bool):
        """a fused-path AgentPPO's networks (`critic`: both, as the rollout takes them; else the actor's three) and dims, then the env block"""
        a, c = agent._act, agent.cri
        nets = ((agent._flat_a.flat, agent._flat_c.flat, a.state_avg.data, a.state_std.data, c.state_avg.data, c.state_std.data) if critic else
                (agent._flat_a.flat, a.state_avg.data, a.state_std.data))
        dims, (h1, h2) = self._dims(self.state_dim, self.action_dim), agent.net_dims
        return (*[_hip.ptr(t, th.float32) for t in nets], *dims[:1], h1, h2, *dims[1:], *self._env_args())

    def _sac_call(self, form: str, agent, *rest) -> None:
        """erl_sac_<form>_<stem>_f32 -- for an agent whose actor is ActorFixSAC (AgentModSAC, `agent._spec.actor_variant`) the launch's
        ActorFixSAC form, erl_sac_<form>_mod_<stem>_f32; for one whose spec names the entry family "td3" (AgentTD3 / AgentDDPG:
        `spec.rollout_family`) erl_td3_<form>_<stem>_f32, whose rollout takes the agent's `explore_noise_std` in front of the stream --
        on the agent's actor, the env block and `rest`"""
        self.state_epoch += 1
        spec = agent._spec
        extra = ()
        if getattr(spec, "rollout_family", "sac") == "td3":
            entry = f"erl_td3_{form}_{self._stem}_f32"
            if form == "rollout":
                extra = (float(agent.explore_noise_std),)
        else:
            entry = f"erl_sac_{form}_{'mod_' if spec.actor_variant else ''}{self._stem}_f32"
        _hip.check(getattr(_hip.lib(), entry)(
            _hip.ptr(agent._actor_flat, th.float32), *self._dims(spec.S, spec.A), spec._c, len(spec.hidden), *self._env_args(), *rest, *extra,
            _hip.stream_ptr()), entry)

    def fused_rollout(self, agent, horizon_len: int, noise, bufs, values, next_value, epilogue=None) -> None:
        """all `horizon_len` steps of AgentPPO._explore_vec_env in ONE launch (erl_rollout_<stem>_f32); `bufs` = (states,
        actions, logprobs, rewards, undones, unmasks) time-major, written in place; the env's state / counters advance.
        `epilogue` = (last_state_out, advantages, reward_sums, stats, workspace, gamma, lambda_gae, use_v_trace) or None: the
        kernel's optional tail (include/erl_hip.h): the agent's own copy of the final state, get_advantages + its statistics."""
        self.state_epoch += 1
        p, f32 = _hip.ptr, th.float32
        states, actions, logprobs, rewards, undones, unmasks = bufs
        entry = f"erl_rollout_{self._stem}_f32"
        _hip.check(getattr(_hip.lib(), entry)(
            *self._ppo_args(agent, True), horizon_len, p(noise, f32), _u64(agent.rng_seed), _u64(agent.rng_counter), float(agent.reward_scale),
            p(states, f32), p(actions, f32), p(logprobs, f32), p(rewards, f32), _hip.flag_ptr(undones), _hip.flag_ptr(unmasks), p(values, f32),
            p(next_value, f32), *_epilogue_args(epilogue), _hip.stream_ptr()), entry)

    def fused_rollout_offpolicy(self, agent, horizon_len: int, noise, bufs, last_state_out) -> None:
        """all `horizon_len` steps of the off-policy AgentBase._explore_vec_env in ONE launch (erl_sac_rollout_<stem>_f32; AgentModSAC:
        erl_sac_rollout_mod_<stem>_f32; AgentTD3 / AgentDDPG: erl_td3_rollout_<stem>_f32 with the agent's explore_noise_std): `bufs` = (states, actions, rewards, undones, unmasks) time-major, written in place (rewards scaled,
        flags inverted); `last_state_out` (N, S) or None: the agent's own copy of the final state; the env's state / counters advance."""
        p, f32 = _hip.ptr, th.float32
        states, actions, rewards, undones, unmasks = bufs
        self._sac_call("rollout", agent, horizon_len, p(noise, f32), _u64(agent.rng_seed), _u64(agent.rng_counter), float(agent.reward_scale),
                       p(states, f32), p(actions, f32), p(rewards, f32), _hip.flag_ptr(undones), _hip.flag_ptr(unmasks), p(last_state_out, f32))

    def fused_evaluate(self, agent, horizon_len: int, workspace) -> None:
        """`horizon_len` steps of the deterministic policy tanh(mean) of a fused-path AgentPPO in ONE launch (erl_eval_<stem>_f32: the
        evaluation form of `fused_rollout`); the per-episode records and per-env counts go to `workspace` (uint8, erl_eval_workspace_bytes);
        the env's state / counters advance."""
        self.state_epoch += 1
        entry = f"erl_eval_{self._stem}_f32"
        _hip.check(getattr(_hip.lib(), entry)(
            *self._ppo_args(agent, False), horizon_len, _hip.ptr(workspace, th.uint8), workspace.numel(), _hip.stream_ptr()), entry)

    def fused_evaluate_offpolicy(self, agent, horizon_len: int, workspace) -> None:
        """... of the deterministic policy of a fused-path AgentSAC (erl_sac_eval_<stem>_f32: the evaluation form of
        `fused_rollout_offpolicy`; AgentModSAC: erl_sac_eval_mod_<stem>_f32, ActorFixSAC.forward; AgentTD3 / AgentDDPG:
        erl_td3_eval_<stem>_f32, Actor.forward)"""
        self._sac_call("eval", agent, horizon_len, _hip.ptr(workspace, th.uint8), workspace.numel())


class SynVecEnv(_ContinuousGpuVecEnv):
    """Synthetic continuous-control workload of SURVEY.md 8d: s' = s Ws + a Wa with Ws = 0.9 I + 0.05 G1,
    Wa = 0.1 G2 (G ~ N(0,1), torch.Generator().manual_seed(0)); reward = -mean(s'^2) - 0.01 mean(a^2);
    terminal = max|s'| > 10; truncate at max_step; done rows reset to N(0,1)."""
    env_name = "SynVecEnv"
    _stem, _action_at, _takes_dims = "synenv", 1, True

    def __init__(self, num_envs: int = 4096, state_dim: int = 64, action_dim: int = 8, max_step: int = 1000,
                 gpu_id: int = 0, seed: int = 0, **_):
        super().__init__(num_envs, state_dim, action_dim, max_step, gpu_id, seed)
        g = th.Generator().manual_seed(0)
        self.Ws = (0.9 * th.eye(state_dim) + 0.05 * th.randn(state_dim, state_dim, generator=g)).to(self.device).contiguous()
        self.Wa = (0.1 * th.randn(action_dim, state_dim, generator=g)).to(self.device).contiguous()
        self.state = th.zeros((num_envs, state_dim), dtype=th.float32, device=self.device)

    def _live(self):
        return (self.state, self.Ws, self.Wa)

    def reset(self) -> Tuple[TEN, dict]:
        self.state_epoch += 1
        g = th.Generator(device=self.device).manual_seed(self.seed)
        self.state = th.randn((self.num_envs, self.state_dim), device=self.device, generator=g)
        self.step_count.zero_()
        self.episode.zero_()
        return self.state.clone(), {}


class PendulumVecEnv(_ContinuousGpuVecEnv):
    """Pendulum-v1 (g=10, m=l=1, dt=0.05, 200-step truncation) behind the reference wrapper's scaling
    (elegantrl/envs/CustomGymEnv.py:42-44: torque = 2*action, reward = 0.5*gym reward).  `phys` (N, 2) = (theta, theta_dot) is the state
    of record, `state` (N, 3) the live observation; the entries fix state_dim 3 and action_dim 1."""
    env_name = "Pendulum-v1"
    _stem, _action_at = "pendulum", 2

    def __init__(self, num_envs: int = 4096, max_step: int = 200, gpu_id: int = 0, seed: int = 0, **_):
        super().__init__(num_envs, 3, 1, max_step, gpu_id, seed)
        self.phys = th.zeros((num_envs, 2), dtype=th.float32, device=self.device)
        self.state = th.zeros((num_envs, 3), dtype=th.float32, device=self.device)

    def _live(self):
        return (self.phys, self.state)

    def reset(self) -> Tuple[TEN, dict]:
        self.state_epoch += 1
        g = th.Generator(device=self.device).manual_seed(self.seed)
        u = th.rand((self.num_envs, 2), device=self.device, generator=g) * 2 - 1
        self.phys = th.stack((u[:, 0] * math.pi, u[:, 1]), dim=1).contiguous()
        self.state = th.stack((self.phys[:, 0].cos(), self.phys[:, 0].sin(), self.phys[:, 1]), dim=1).contiguous()
        self.step_count.zero_()
        self.episode.zero_()
        return self.state.clone(), {}


class PointChasingVecEnv(_ContinuousGpuVecEnv):
    """The reference's PointChasingVecEnv (elegantrl/envs/PointChasingEnv.py:84-182) on the device: a chaser p1, steered by the action
    (scaled down to unit length where longer), runs after a target p0 that drifts by `dim` uniform draws per step; reward = the distance
    closed minus 0.02 max(|action|, 1); the episode ends when the distance falls below `dim` or at `max_step`.  `state` (N, 4 dim) =
    (p0, v0, p1, v1) is the observation and the state of record, `distance` (N,) the carried |p0 - p1|; the entries take state_dim = 4 dim
    and action_dim = dim (1..4).  csrc/pointchasing_step.h states the step, operation for operation, and the three deviations from the
    reference's vec env: `distance` is recomputed after a reset (the reference leaves it stale), terminal = caught and truncate = time limit
    (the reference raises terminal for both), draws are Philox4x32-10 keyed by (seed, env, episode, step).
    The reference's KEYWORD spellings `env_num` and `sim_gpu_id` are accepted; its positional order (dim, env_num, sim_gpu_id) is not this
    constructor's (dim, num_envs, max_step, ...), so a positional third argument is a max_step here and one below 1 is refused."""
    env_name = "PointChasingVecEnv"
    _stem, _action_at, _takes_dims = "pointchasing", 1, True
    init_distance = 8.0

    def __init__(self, dim: int = 2, num_envs: int = 4096, max_step: int = 1024, gpu_id: int = 0, seed: int = 0, env_num: Optional[int] = None,
                 sim_gpu_id: Optional[int] = None, **_):
        num_envs, gpu_id = self._aliases(num_envs, gpu_id, env_num, sim_gpu_id)
        if not 1 <= int(dim) <= 4:
            raise ValueError(f"PointChasingVecEnv: dim = {dim}, the device env covers 1..4")
        if int(max_step) < 1 or int(num_envs) < 1:
            raise ValueError(f"PointChasingVecEnv: num_envs = {num_envs}, max_step = {max_step}; both must be at least 1 (the arguments are "
                             "(dim, num_envs, max_step, gpu_id, seed): pass the reference's env_num / sim_gpu_id by keyword)")
        self.dim = int(dim)
        super().__init__(num_envs, 4 * self.dim, self.dim, max_step, gpu_id, seed)
        self.state = th.zeros((num_envs, 4 * self.dim), dtype=th.float32, device=self.device)
        self.distance = th.zeros(num_envs, dtype=th.float32, device=self.device)

    @staticmethod
    def _aliases(num_envs: int, gpu_id: int, env_num, sim_gpu_id) -> Tuple[int, int]:
        """the reference's spellings (`env_num`, `sim_gpu_id`; -1 there means the CPU) win where they are given"""
        return (num_envs if env_num is None else int(env_num)), (gpu_id if sim_gpu_id is None else int(sim_gpu_id))

    def _live(self):
        return (self.state, self.distance)

    def reset(self, **_) -> Tuple[TEN, dict]:
        self.state_epoch += 1
        d = self.dim
        g = th.Generator(device=self.device).manual_seed(self.seed)
        draws = th.randn((self.num_envs, 2 * d), device=self.device, generator=g)
        zeros = th.zeros((self.num_envs, d), dtype=th.float32, device=self.device)
        p0, p1 = draws[:, :d], draws[:, d:] - self.init_distance
        self.state = th.cat((p0, zeros, p1, zeros), dim=1).contiguous()
        sq = (p0 - p1) ** 2
        total = sq[:, 0]
        for k in range(1, d):                  # (index order, as the step sums it)
            total = total + sq[:, k]
        self.distance = total.sqrt().contiguous()
        self.step_count.zero_()
        self.episode.zero_()
        return self.state.clone(), {}

    @staticmethod
    def get_action(states: TEN) -> TEN:
        """the reference's chase heuristic: head for the target (p0 - p1)"""
        rows = states.reshape((states.shape[0], 4, -1))
        return rows[:, 0] - rows[:, 2]


class _DiscreteGpuVecEnv(_GpuVecEnv):
    """what the device-resident discrete envs share: the per-step launch and the one-launch rollout / evaluation of a discrete agent
    (csrc/rollout_discrete.hip).  An env adds its constructor, `reset`, the names of its three C entries, `_live` and `_step`."""
    if_discrete = True
    _rollout_entry = _gae_entry = _eval_entry = ""

    def _live(self) -> Tuple[TEN, ...]:
        """the live buffers the C entries take, in their order (looked up per call: `reset` rebinds them)"""
        raise NotImplementedError

    def _step(self, *rows) -> None:
        """the env's `ops.*_step` on its live buffers; `rows` = what follows them, from the action on"""
        raise NotImplementedError

    @_hip.on_device
    def step_into(self, action: TEN, reward_row: TEN, terminal_row: TEN, truncate_row: TEN) -> TEN:
        self.state_epoch += 1
        action = action.to(self.device).reshape(-1)
        if action.dtype != th.int64:
            action = action.long()
        self._step(action.contiguous(), self.step_count, self.episode, reward_row, terminal_row, truncate_row, self.max_step, self.seed)
        return self.state

    def _policy_args(self, agent):
        p, f32 = _hip.ptr, th.float32
        a = agent._act
        h1, h2 = agent.net_dims
        return (p(agent._flat_a.flat, f32), p(a.state_avg.data, f32), p(a.state_std.data, f32), self.state_dim, h1, h2, agent.action_dim,
                *[p(t, f32) for t in self._live()], p(self.step_count, th.int32), p(self.episode, th.int32), self.max_step,
                self.seed & (2 ** 64 - 1), self.num_envs)

    @_hip.on_device
    def fused_rollout_discrete(self, agent, horizon_len: int, uniform, bufs, last_state_out, uniform_out=None, epilogue=None) -> None:
        """all `horizon_len` steps of AgentDiscretePPO._explore_vec_env in ONE launch (erl_rollout_discrete_<env>_f32): `bufs` = (states,
        actions int32, logprobs, rewards, undones, unmasks) time-major, written in place (rewards scaled, flags inverted); `uniform` (H, N)
        injects the U[0,1) draws or None (Philox keyed by (agent.rng_seed, agent.rng_counter + t, env)); `last_state_out` (N, state_dim)
        or None: the agent's own copy of the final state; `uniform_out` (H, N) or None: the u every cell used.  The env's live buffers
        and counters advance.
        `epilogue` = (values (H, N), next_value (N,), advantages (H, N), reward_sums (H, N), partials (3 * erl_rollout_discrete_gae_partials(N),)
        float64, gamma, lambda_gae, use_v_trace) or None: the same launch also leaves the critic's values, get_advantages (raw), the reward
        sums and the per-tile sums of the normalisation (erl_rollout_discrete_<env>_gae_f32); everything else is what it is without."""
        self.state_epoch += 1
        p, f32 = _hip.ptr, th.float32
        states, actions, logprobs, rewards, undones, unmasks = bufs
        name = self._rollout_entry if epilogue is None else self._gae_entry
        tail = () if epilogue is None else _discrete_epilogue_args(agent, epilogue)
        _hip.check(getattr(_hip.lib(), name)(
            *self._policy_args(agent), horizon_len, p(uniform, f32), agent.rng_seed & (2 ** 64 - 1), agent.rng_counter & (2 ** 64 - 1),
            float(agent.reward_scale), p(states, f32), p(actions, th.int32), p(logprobs, f32), p(rewards, f32), _hip.flag_ptr(undones),
            _hip.flag_ptr(unmasks), p(last_state_out, f32), p(uniform_out, f32), *tail, _hip.stream_ptr()), name)

    @_hip.on_device
    def fused_evaluate_discrete(self, agent, horizon_len: int, workspace) -> None:
        """`horizon_len` steps of the greedy policy argmax(logits) of a discrete agent in ONE launch (erl_eval_discrete_<env>_f32: the
        evaluation form of `fused_rollout_discrete`); records and counts go to `workspace` as SynVecEnv.fused_evaluate leaves them."""
        self.state_epoch += 1
        name = self._eval_entry
        _hip.check(getattr(_hip.lib(), name)(
            *self._policy_args(agent), horizon_len, _hip.ptr(workspace, th.uint8), workspace.numel(), _hip.stream_ptr()), name)


class CartPoleGpuVecEnv(_DiscreteGpuVecEnv):
    """CartPole-v1 for N envs on the device (erl_cartpole_step_f32): CartPoleVecEnv's dynamics -- gymnasium's physics, Euler, dt 0.02,
    force +-10, any action other than 1 pushes left, terminal when |x| > 2.4 or |theta| > 12 degrees on the new state, reward 1,
    truncation at max_step -- in one launch per step, and behind `fused_rollout_discrete` / `fused_evaluate_discrete` the whole horizon of
    a discrete agent in one launch.  A done row restarts from four U[-0.05, 0.05) Philox draws keyed by (seed, env, episode, component)."""
    env_name = "CartPole-v1"
    _rollout_entry, _gae_entry = "erl_rollout_discrete_cartpole_f32", "erl_rollout_discrete_cartpole_gae_f32"
    _eval_entry = "erl_eval_discrete_cartpole_f32"

    def __init__(self, num_envs: int = 1024, max_step: int = 500, gpu_id: int = 0, seed: int = 0, **_):
        super().__init__(num_envs, 4, 2, max_step, gpu_id, seed)
        self.state = th.zeros((num_envs, 4), dtype=th.float32, device=self.device)

    def _live(self):
        return (self.state,)

    def _step(self, *rows):
        from .. import ops
        ops.cartpole_step(self.state, *rows)

    def reset(self) -> Tuple[TEN, dict]:
        self.state_epoch += 1
        g = th.Generator(device=self.device).manual_seed(self.seed)
        self.state = th.rand((self.num_envs, 4), device=self.device, generator=g) * 0.1 - 0.05
        self.step_count.zero_()
        self.episode.zero_()
        return self.state.clone(), {}


class AcrobotGpuVecEnv(_DiscreteGpuVecEnv):
    """Acrobot-v1 for N envs on the device (erl_acrobot_step_f32): gymnasium's "book" dynamics -- two unit links, g 9.8, dt 0.2, one RK4
    step, angles wrapped into [-pi, pi], velocities clipped to +-4 pi / +-9 pi; action 0 / 1 / 2 is torque -1 / 0 / +1 (any other value:
    0); terminal when -cos(theta1) - cos(theta1 + theta2) > 1 on the new state; reward 0 on the terminal step, -1 otherwise; truncation
    at max_step -- in one launch per step, and behind `fused_rollout_discrete` / `fused_evaluate_discrete` the whole horizon of a discrete
    agent in one launch.  `phys` (N, 4) = (theta1, theta2, omega1, omega2) is the state of record; `state` (N, 6) = (cos theta1,
    sin theta1, cos theta2, sin theta2, omega1, omega2) is the live observation.  A done row restarts from four U[-0.1, 0.1) Philox draws
    keyed by (seed, env, episode, component).
    In `fused_rollout_discrete` the policy's input at t = 0 is `state` as it stands (the caller may have written its own last state
    there; `phys` is not disturbed by that), from t = 1 on the observation of `phys`.  `phys`, `state` and the counters advance."""
    env_name = "Acrobot-v1"
    _rollout_entry, _gae_entry = "erl_rollout_discrete_acrobot_f32", "erl_rollout_discrete_acrobot_gae_f32"
    _eval_entry = "erl_eval_discrete_acrobot_f32"

    def __init__(self, num_envs: int = 1024, max_step: int = 500, gpu_id: int = 0, seed: int = 0, **_):
        super().__init__(num_envs, 6, 3, max_step, gpu_id, seed)
        self.phys = th.zeros((num_envs, 4), dtype=th.float32, device=self.device)
        self.state = self._observe(self.phys)

    def _live(self):
        return (self.phys, self.state)

    def _step(self, *rows):
        from .. import ops
        ops.acrobot_step(self.phys, self.state, *rows)

    @staticmethod
    def _observe(phys: TEN) -> TEN:
        return th.stack((phys[:, 0].cos(), phys[:, 0].sin(), phys[:, 1].cos(), phys[:, 1].sin(), phys[:, 2], phys[:, 3]), dim=1).contiguous()

    def reset(self) -> Tuple[TEN, dict]:
        self.state_epoch += 1
        g = th.Generator(device=self.device).manual_seed(self.seed)
        self.phys = th.rand((self.num_envs, 4), device=self.device, generator=g) * 0.2 - 0.1
        self.state = self._observe(self.phys)
        self.step_count.zero_()
        self.episode.zero_()
        return self.state.clone(), {}


class MountainCarGpuVecEnv(_DiscreteGpuVecEnv):
    """MountainCar-v0 for N envs on the device (erl_mountaincar_step_f32): gymnasium's dynamics -- `state` (N, 2) = (position, velocity)
    is the observation; action 0 / 1 / 2 pushes left / nowhere / right (any other value: nowhere); velocity += (action - 1) * 0.001 +
    cos(3 position) * (-0.0025), clipped to +-0.07; position += velocity, clipped to [-1.2, 0.6]; at position -1.2 a negative velocity
    becomes 0; terminal when position >= 0.5 with velocity >= 0 on the new state; reward -1 on every step, the terminal one included;
    truncation at max_step (200) -- in one launch per step, and behind `fused_rollout_discrete` / `fused_evaluate_discrete` the whole
    horizon of a discrete agent in one launch.  A done row restarts at velocity 0 and a position U[-0.6, -0.4) from one Philox draw keyed
    by (seed, env, episode, component).
    No claim that PPO learns it from scratch is made or tested: a uniformly random policy ends no episode by `terminal` within 200 steps
    (0 of 4096 gymnasium starts, in float64 and in float32), so every return such an agent sees is -200 and the reward carries no signal.
    What is tested is the env, the one-launch routes on it and the update kernels at state_dim 2."""
    env_name = "MountainCar-v0"
    _rollout_entry, _gae_entry = "erl_rollout_discrete_mountaincar_f32", "erl_rollout_discrete_mountaincar_gae_f32"
    _eval_entry = "erl_eval_discrete_mountaincar_f32"

    def __init__(self, num_envs: int = 1024, max_step: int = 200, gpu_id: int = 0, seed: int = 0, **_):
        super().__init__(num_envs, 2, 3, max_step, gpu_id, seed)
        self.state = th.zeros((num_envs, 2), dtype=th.float32, device=self.device)

    def _live(self):
        return (self.state,)

    def _step(self, *rows):
        from .. import ops
        ops.mountaincar_step(self.state, *rows)

    def reset(self) -> Tuple[TEN, dict]:
        self.state_epoch += 1
        g = th.Generator(device=self.device).manual_seed(self.seed)
        self.state = th.zeros((self.num_envs, 2), dtype=th.float32, device=self.device)
        self.state[:, 0] = th.rand((self.num_envs,), device=self.device, generator=g) * 0.2 - 0.6
        self.step_count.zero_()
        self.episode.zero_()
        return self.state.clone(), {}


class CartPoleVecEnv:
    """CartPole-v1 for N envs, written with plain torch ops on device tensors: an exemplar of "any env honouring the
    reference's vector protocol" for the discrete agents (action (N,) int64, auto-reset, 5-tuple).  gymnasium's physics:
    gravity 9.8, cart 1.0 kg, pole 0.1 kg, half-length 0.5 m, force 10 N, dt 0.02 s (Euler), terminal when |x| > 2.4 or
    |theta| > 12 degrees, reward 1 per step, truncation at max_step (500)."""
    env_name = "CartPole-v1"
    if_discrete = True

    def __init__(self, num_envs: int = 1024, max_step: int = 500, gpu_id: int = 0, seed: int = 0, **_):
        self.device = th.device(f"cuda:{gpu_id}" if (th.cuda.is_available() and gpu_id >= 0) else "cpu")
        self.num_envs, self.state_dim, self.action_dim, self.max_step = num_envs, 4, 2, max_step
        self.gen = th.Generator(device=self.device).manual_seed(int(seed))
        self.state = th.zeros((num_envs, 4), dtype=th.float32, device=self.device)
        self.step_count = th.zeros(num_envs, dtype=th.int32, device=self.device)

    def _fresh(self, n: int) -> TEN:
        return th.rand((n, 4), device=self.device, generator=self.gen) * 0.1 - 0.05

    def reset(self) -> Tuple[TEN, dict]:
        self.state = self._fresh(self.num_envs)
        self.step_count.zero_()
        return self.state.clone(), {}

    def step(self, action: TEN) -> Tuple[TEN, TEN, TEN, TEN, dict]:
        x, x_dot, theta, theta_dot = self.state.unbind(dim=1)
        force = th.where(action.to(self.device).reshape(-1) == 1, 10.0, -10.0).to(th.float32)
        cos, sin = theta.cos(), theta.sin()
        temp = (force + 0.05 * theta_dot * theta_dot * sin) / 1.1                       # polemass_length = 0.05, total mass 1.1
        theta_acc = (9.8 * sin - cos * temp) / (0.5 * (4.0 / 3.0 - 0.1 * cos * cos / 1.1))
        x_acc = temp - 0.05 * theta_acc * cos / 1.1
        state = th.stack((x + 0.02 * x_dot, x_dot + 0.02 * x_acc, theta + 0.02 * theta_dot, theta_dot + 0.02 * theta_acc), dim=1)
        self.step_count += 1
        terminal = (state[:, 0].abs() > 2.4) | (state[:, 2].abs() > 12 * 2 * math.pi / 360)
        truncate = (self.step_count >= self.max_step) & ~terminal
        done = terminal | truncate
        reward = th.ones(self.num_envs, dtype=th.float32, device=self.device)
        state = th.where(done[:, None], self._fresh(self.num_envs), state)
        self.step_count = th.where(done, th.zeros_like(self.step_count), self.step_count)
        self.state = state
        return state.clone(), reward, terminal, truncate, {}
