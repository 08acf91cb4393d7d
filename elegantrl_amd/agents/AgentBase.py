"""`AgentBase`: constructor contract, attributes and checkpoint format of elegantrl/agents/AgentBase.py,
plus the flat-parameter plumbing the HIP kernels need.

What is kept from the reference (it is the API run.py / Evaluator drive):
ctor `(net_dims, state_dim, action_dim, gpu_id, args)`, the hyper-parameter attributes read from
`Config`, `explore_env` dispatch (:70-74), settable `act` / `last_state`, `save_or_load_agent`
(:280-297, whole-object `th.save` files), `explore_rate` (run.py:126 needs it) and the torch-module
builders `build_mlp` / `layer_init_with_orthogonal` (:345-365).

What is new: `FlatNet` makes an actor/critic's trainable parameters views into one flat fp32 buffer laid
out as include/erl_hip.h describes, so kernels read/write weights in place while the objects stay
ordinary picklable `nn.Module`s; `_OffPolicyFlatAgent` is what AgentSAC / AgentModSAC / AgentTD3 / AgentDDPG share on top of it.
"""
from __future__ import annotations

import os
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch as th
from torch import nn

from .. import _hip
from ..train.config import Config

TEN = th.Tensor


def build_mlp(dims: List[int], activation=None, if_raw_out: bool = True) -> nn.Sequential:
    """Linear -> GELU -> ... -> Linear (no activation after the last layer when if_raw_out)."""
    act = nn.GELU if activation is None else activation
    layers: list = []
    for d_in, d_out in zip(dims[:-1], dims[1:]):
        layers += [nn.Linear(d_in, d_out), act()]
    if if_raw_out:
        layers.pop()
    return nn.Sequential(*layers)


def layer_init_with_orthogonal(layer, std: float = 1.0, bias_const: float = 1e-6):
    th.nn.init.orthogonal_(layer.weight, std)
    th.nn.init.constant_(layer.bias, bias_const)


class FlatNet:
    """Binds an `nn.Module` with sub-module `net` = build_mlp([S, h1, h2, out]) (and optionally
    `action_std_log`) to a slice of a flat fp32 parameter buffer.  After `bind`, each trainable
    parameter's `.data` is a view into the slice, in the order W1,b1,W2,b2,W3,b3[,action_std_log]."""

    def __init__(self, module: nn.Module, spec, flat_slice: TEN):
        self.module = module
        self.spec = spec
        self.flat = flat_slice
        self.bind(module)

    def _named(self, module):
        sd = dict(module.named_parameters())
        return [(name, sd[name], off, shape) for name, off, shape in self.spec.slices()]

    def bind(self, module: nn.Module) -> None:
        """copy the module's current values into the flat slice and re-point the parameters at it."""
        self.module = module
        self._probe = None
        with th.no_grad():
            for name, p, off, shape in self._named(module):
                assert tuple(p.shape) == tuple(shape), f"{name}: {tuple(p.shape)} != {shape}"
                view = self.flat[off:off + p.numel()].view(shape)
                view.copy_(p.data.to(self.flat.device, th.float32))
                p.data = view

    def is_bound(self, module: nn.Module) -> bool:
        """does the module's first parameter still live in the flat block?  (O(1): the owning sub-module and attribute are looked
        up once per bind -- walking named_parameters() on every explore_env / update_net cost ~20 us of interpreter time each,
        with the GPU idle behind the previous iteration's host sync)"""
        if module is not self.module:
            return False
        probe = self._probe
        if probe is None or probe[0] is not module:
            name, _, off, _ = self._named(module)[0]
            owner, _, attr = name.rpartition(".")
            probe = self._probe = (module, module.get_submodule(owner) if owner else module, attr, off)
        p = probe[1]._parameters.get(probe[2])
        return p is not None and p.data_ptr() == self.flat.data_ptr() + 4 * probe[3]


def criterion_code(criterion) -> Tuple[int, float]:
    """`args.criterion` (elegantrl/agents/AgentBase.py:62) as the (kind, threshold) pair the update entries take (include/erl_hip.h,
    ERL_CRIT_*; csrc/critic_loss.h).  The reference multiplies the element-wise loss by `unmask` (AgentPPO.py:190, AgentSAC.py:60), so only
    reduction='none' makes sense there, and only the three modules whose loss the kernels hold are accepted: nothing is ignored."""
    supported = "supported: torch.nn.MSELoss, torch.nn.SmoothL1Loss (beta > 0) and torch.nn.HuberLoss, each with reduction='none'"
    for cls, kind, attr in ((nn.MSELoss, _hip.CRIT_MSE, None), (nn.SmoothL1Loss, _hip.CRIT_SMOOTH_L1, "beta"),
                            (nn.HuberLoss, _hip.CRIT_HUBER, "delta")):
        if type(criterion) is not cls:
            continue
        if criterion.reduction != "none":
            raise ValueError(f"args.criterion = {criterion!r} has reduction={criterion.reduction!r}: the reference multiplies the element-wise "
                             f"loss by `unmask` before it takes the mean, so the criterion must be built with reduction='none'")
        beta = 1.0 if attr is None else float(getattr(criterion, attr))
        if not (beta > 0.0 and beta < float("inf")):
            why = "SmoothL1Loss(beta=0) is L1Loss, which the kernels do not hold" if cls is nn.SmoothL1Loss else "HuberLoss needs delta > 0"
            raise NotImplementedError(f"args.criterion = {criterion!r} with {attr}={beta}: {why}; {supported}")
        return kind, beta
    raise NotImplementedError(f"args.criterion = {criterion!r} is not implemented by the HIP kernels; {supported}")


class AgentBase:
    """Hyper-parameter capture + the generic pieces shared by the agents."""

    def __init__(self, net_dims: List[int], state_dim: int, action_dim: int, gpu_id: int = 0, args: Config = None):
        args = Config() if args is None else args
        self.if_discrete: bool = args.if_discrete
        self.if_off_policy: bool = args.if_off_policy
        self.net_dims = net_dims
        self.state_dim = state_dim
        self.action_dim = action_dim

        self.gamma = args.gamma
        self.max_step = args.max_step
        self.num_envs = args.num_envs
        self.batch_size = args.batch_size
        self.repeat_times = args.repeat_times
        self.reward_scale = args.reward_scale
        self.learning_rate = args.learning_rate
        self.clip_grad_norm = args.clip_grad_norm
        self.soft_update_tau = args.soft_update_tau
        self.state_value_tau = args.state_value_tau
        self.buffer_init_size = args.buffer_init_size

        self.explore_noise_std = getattr(args, "explore_noise_std", 0.05)
        self.explore_rate = getattr(args, "explore_rate", 1.0)  # read by run.py:126 in the single-process loop
        self.last_state: Optional[TEN] = None
        self.device = th.device(f"cuda:{gpu_id}" if (th.cuda.is_available() and gpu_id >= 0) else "cpu")

        self._act = None
        self.cri = None
        self.act_target = None
        self.cri_target = None
        self.act_optimizer = None
        self.cri_optimizer = None

        self.criterion = getattr(args, "criterion", th.nn.MSELoss(reduction="none"))     # the torch module, as the reference keeps it
        self.criterion_code = criterion_code(self.criterion)       # (kind, threshold): what every update route hands to its entry
        self.if_vec_env = self.num_envs > 1
        self.if_use_per = getattr(args, "if_use_per", None)
        self.lambda_fit_cum_r = getattr(args, "lambda_fit_cum_r", 0.0)

        self.save_attr_names = {"act", "act_target", "act_optimizer", "cri", "cri_target", "cri_optimizer"}

        # data-parallel context (one process per GPU; see elegantrl_amd/parallel.py)
        self.world_size = int(getattr(args, "world_size", 1))
        self.rank = int(getattr(args, "rank", 0))
        seed = getattr(args, "random_seed", None)
        self.rng_seed = (int(seed) if seed is not None else max(0, gpu_id)) * 1000003 + 7919 * self.rank
        self.rng_counter = 0
        self._last_state_token = None

    # ---- the last state between two one-launch rollouts: the env owns the live buffer, the agent holds the copy the launch wrote ------
    def _hand_state_to_env(self, env, state: TEN) -> None:
        """`state` (`last_state` on the device) becomes `env.state`, the live buffer -- unless `_last_state_token` says the buffer already
        holds it: `last_state` is the very tensor the last one-launch rollout of THIS env wrote as its copy of the final state, nobody
        has written to it, and the env has not moved since (no copy-back launch).  A copy counts as a move of the env."""
        if state.data_ptr() == env.state.data_ptr():
            return
        tok = self._last_state_token
        same = (tok is not None and tok[0] is self.last_state and tok[1] == self.last_state._version and tok[2] is env
                and tok[3] == getattr(env, "state_epoch", None) and tok[4] == (id(env.state), env.state._version))
        if not same:
            env.state.copy_(state)
            if hasattr(env, "state_epoch"):
                env.state_epoch += 1

    def _record_last_state(self, env, last_out: TEN) -> None:
        """`last_out`, the copy of its final state a one-launch rollout of `env` has just written, is `last_state`; the token is what
        `_hand_state_to_env` compares at the next call"""
        self.last_state = last_out
        self._last_state_token = (last_out, last_out._version, env, getattr(env, "state_epoch", None), (id(env.state), env.state._version))

    # ---- the env-pairing rule of every one-launch rollout and evaluation --------------------------------
    def _one_launch_reason(self, env, what: str) -> Optional[str]:
        """None when `env` and this agent take the one-launch route through the env's method `what` (a rollout or its evaluation
        twin: one rule, so the two cannot drift apart), else why not.  `_one_launch_agent_reason()` is the agent class's own part:
        its switches and the shapes its one-launch kernels cover."""
        if self.device.type != "cuda":
            return "no GPU"
        reason = self._one_launch_agent_reason()
        if reason is not None:
            return reason
        if not hasattr(env, what):
            return f"{type(env).__name__} has no {what}"
        if getattr(env, "device", None) != self.device:
            return f"the env lives on {getattr(env, 'device', None)}, the agent on {self.device}"
        if getattr(env, "num_envs", None) != self.num_envs:
            return f"the env has {getattr(env, 'num_envs', None)} envs, the agent {self.num_envs}"
        if getattr(env, "state_dim", None) != self.state_dim or getattr(env, "action_dim", None) != self.action_dim:
            return "the env's state / action dims are not the agent's"
        return None

    # ---- evaluation on the device (csrc/rollout_eval.hip) ---------------------------------------------
    def evaluate_env(self, env) -> Optional[TEN]:
        """(n_episodes, 2) float32 CPU tensor of (return, length) of every episode `env` finishes within `env.max_step` steps of the
        deterministic policy `act(state)`, from two launches -- or None where this agent / env pair has no fused evaluation (the
        Evaluator then runs its loop).  AgentPPO and AgentSAC implement it."""
        return None

    def _evaluate_env_fused(self, env, launch) -> TEN:
        """env.reset(), `launch(workspace)` = the persistent evaluation launch, the compaction launch, and two device-to-host copies:
        the episode count, then the rows.  Touches nothing the training loop reads: the buffers here are the evaluation's own."""
        from ..envs.vec_envs import compact_episodes
        N, H, dev = int(env.num_envs), int(env.max_step), self.device
        nbytes = int(_hip.lib().erl_eval_workspace_bytes(N, H))
        if nbytes <= 0:
            raise _hip.HipExtensionError(f"evaluate_env: erl_eval_workspace_bytes({N}, {H}) = {nbytes}")
        bufs = getattr(self, "_eval_bufs", None)
        if bufs is None or bufs[0] != (N, H, dev):
            bufs = ((N, H, dev), th.empty(nbytes, dtype=th.uint8, device=dev), th.empty((N * H, 2), dtype=th.float32, device=dev),
                    th.empty(1, dtype=th.int32, device=dev))
            self._eval_bufs = bufs
        _, workspace, rows, count = bufs
        env.reset()
        launch(workspace)
        compact_episodes(workspace, N, H, rows, count)
        n = int(count.item())
        return rows[:n].cpu()

    # `act` is settable (run.py:404-407 replaces it with the learner's copy); subclasses re-bind kernels
    @property
    def act(self):
        return self._act

    @act.setter
    def act(self, module):
        self._act = module
        self._on_act_replaced()

    def _on_act_replaced(self):
        pass

    @_hip.on_device
    def explore_env(self, env, horizon_len: int, if_random: bool = False) -> Tuple[TEN, ...]:
        """AgentBase.py:70-74.  `if_random` is accepted for signature parity with the PPO rollout of the reference
        (AgentPPO.py:87), which never reads it either."""
        if self.if_vec_env:
            return self._explore_vec_env(env=env, horizon_len=horizon_len)
        return self._explore_one_env(env=env, horizon_len=horizon_len)

    # spellings used by older releases / the north star
    def explore_vec_env(self, env, horizon_len: int):
        return self._explore_vec_env(env=env, horizon_len=horizon_len)

    def explore_one_env(self, env, horizon_len: int):
        return self._explore_one_env(env=env, horizon_len=horizon_len)

    # ---- off-policy defaults (overridden by the on-policy agents): AgentBase.py:76-189 of the reference ----------
    def explore_action(self, state: TEN) -> TEN:
        return self.act.get_action(state)

    def _explore_vec_env(self, env, horizon_len: int, noise: Optional[TEN] = None) -> Tuple[TEN, ...]:
        """off-policy vectorised rollout -> (states, actions, rewards, undones, unmasks), time-major (H, N, .); the
        already-squashed action is both stored and sent to the env (AgentBase.py:130-170).  GPU-resident envs write
        reward / terminal / truncate straight into row t (`step_into`)."""
        H, N, dev = horizon_len, self.num_envs, self.device
        states = th.zeros((H, N, self.state_dim), dtype=th.float32, device=dev)
        actions = th.zeros((H, N, self.action_dim), dtype=th.float32, device=dev)
        rewards = th.zeros((H, N), dtype=th.float32, device=dev)
        terminals = th.zeros((H, N), dtype=th.bool, device=dev)
        truncates = th.zeros((H, N), dtype=th.bool, device=dev)
        native = hasattr(env, "step_into")
        state = self.last_state.to(dev, th.float32)
        assert state.shape == (N, self.state_dim)
        import inspect
        sig = inspect.signature(self.explore_action).parameters
        into_row = "out" in sig                     # the agent's kernel writes the action into its buffer row
        state_row = into_row and "out_state" in sig     # ... and `states[t] = state` too
        # (the rows as views made once: the loop is bound by the interpreter -- ~45 us per time step for three launches)
        st_rows, ac_rows, rw_rows, te_rows, tr_rows = states.unbind(0), actions.unbind(0), rewards.unbind(0), terminals.unbind(0), truncates.unbind(0)
        for t in range(H):
            if state_row:
                action = self.explore_action(state, None if noise is None else noise[t], out=ac_rows[t], out_state=st_rows[t])
            elif into_row:
                action = self.explore_action(state, None if noise is None else noise[t], out=ac_rows[t])
            else:
                action = self.explore_action(state) if noise is None else self.explore_action(state, noise[t])
                ac_rows[t].copy_(action)
            if not state_row:
                st_rows[t].copy_(state)
            if native:
                state = env.step_into(action if into_row else action.contiguous(), rw_rows[t], te_rows[t], tr_rows[t])
            else:
                state, reward, terminal, truncate, _ = env.step(action)
                state = state.to(dev, th.float32)
                rewards[t] = reward
                terminals[t] = terminal
                truncates[t] = truncate
        self.last_state = state.clone() if native else state
        rewards *= self.reward_scale
        return states, actions, rewards, th.logical_not(terminals), th.logical_not(truncates)

    def _explore_one_env(self, env, horizon_len: int) -> Tuple[TEN, ...]:
        """single numpy env (AgentBase.py:76-128): same 5-tuple with a middle dimension of 1."""
        H, dev = horizon_len, self.device
        states = th.zeros((H, 1, self.state_dim), dtype=th.float32, device=dev)
        actions = th.zeros((H, 1, self.action_dim), dtype=th.float32, device=dev)
        rewards = th.zeros((H, 1), dtype=th.float32, device=dev)
        terminals = th.zeros((H, 1), dtype=th.bool, device=dev)
        truncates = th.zeros((H, 1), dtype=th.bool, device=dev)
        state = self.last_state.to(dev, th.float32).reshape(1, self.state_dim)
        for t in range(H):
            action = self.explore_action(state)
            states[t], actions[t] = state, action
            ary_state, reward, terminal, truncate, _ = env.step(action[0].detach().cpu().numpy())
            if terminal or truncate:
                ary_state, _ = env.reset()
            state = th.as_tensor(ary_state, dtype=th.float32, device=dev).reshape(1, self.state_dim)
            rewards[t, 0], terminals[t, 0], truncates[t, 0] = float(reward), bool(terminal), bool(truncate)
        self.last_state = state
        rewards *= self.reward_scale
        return states, actions, rewards, th.logical_not(terminals), th.logical_not(truncates)

    @_hip.on_device
    def update_net(self, buffer) -> Tuple[float, ...]:
        """off-policy update loop (AgentBase.py:172-189): `update_times = int(cur_size * repeat_times / batch_size)` steps of
        `update_objectives`, each drawing one minibatch through ReplayBuffer.sample (HIP K9)."""
        import numpy as np
        objs_critic, objs_actor = [], []
        if self.lambda_fit_cum_r != 0:
            buffer.update_cum_rewards(get_cumulative_rewards=self.get_cumulative_rewards)
        th.set_grad_enabled(True)
        update_times = int(buffer.cur_size * self.repeat_times / self.batch_size)
        for update_t in range(update_times):
            obj_critic, obj_actor = self.update_objectives(buffer=buffer, update_t=update_t)
            objs_critic.append(obj_critic)
            if isinstance(obj_actor, float):
                objs_actor.append(obj_actor)
        th.set_grad_enabled(False)
        return (float(np.nanmean(objs_critic)) if objs_critic else 0.0, float(np.nanmean(objs_actor)) if objs_actor else 0.0)

    def update_objectives(self, buffer, update_t: int) -> Tuple[float, float]:
        raise NotImplementedError

    @_hip.on_device
    def get_cumulative_rewards(self, rewards: TEN, undones: TEN) -> TEN:
        """n-step discounted return of the newest `add_size` rows of the replay buffer (AgentBase.py:226-237), bootstrapped
        with `cri_target(last_state, act_target(last_state))`; the backward scan runs in erl_cum_rewards_f32 (bit-exact op
        order).  Agents without a target actor (the reference's AgentSAC leaves `act_target = None` and would raise
        'NoneType is not callable' here) bootstrap with the current actor instead."""
        from .. import ops
        if self.device.type != "cuda":
            raise _hip.HipExtensionError("get_cumulative_rewards runs on the HIP kernels only; no GPU is visible")
        last_state = self.last_state.to(self.device, th.float32)
        actor = self.act_target if self.act_target is not None else self.act
        critic = self.cri_target if self.cri_target is not None else self.cri
        with th.no_grad():
            next_value = critic(last_state, actor(last_state)).detach().reshape(-1).to(th.float32).contiguous()
        return ops.cum_rewards(rewards.contiguous(), undones.to(th.float32).contiguous(), next_value, float(self.gamma))

    def optimizer_backward(self, optimizer, objective: TEN):
        """zero_grad, backward, global-norm clip of the optimiser's first param group, step (AgentBase.py:239-248)."""
        optimizer.zero_grad()
        objective.backward()
        th.nn.utils.clip_grad_norm_(parameters=optimizer.param_groups[0]["params"], max_norm=self.clip_grad_norm)
        optimizer.step()

    @staticmethod
    def soft_update(target_net: nn.Module, current_net: nn.Module, tau: float):
        with th.no_grad():
            for tar, cur in zip(target_net.parameters(), current_net.parameters()):
                tar.data.mul_(1.0 - tau).add_(cur.data, alpha=tau)

    def save_or_load_agent(self, cwd: str, if_save: bool):
        """whole-object checkpoint files `{cwd}/{attr}.pth`, as AgentBase.py:280-297."""
        assert self.save_attr_names.issuperset({"act", "act_optimizer"})
        for attr_name in self.save_attr_names:
            path = f"{cwd}/{attr_name}.pth"
            obj = getattr(self, attr_name, None)
            if if_save:
                if obj is not None:
                    th.save(obj, path)
            elif os.path.isfile(path):
                setattr(self, attr_name, th.load(path, map_location=self.device, weights_only=False))


class _Slices:
    def __init__(self, slices):
        self._s = slices

    def slices(self):
        return self._s


class _FlatAdamState:
    """Adam moments of one parameter block as flat tensors (what `save_or_load_agent` stores for the optimisers)."""

    def __init__(self, numel: int, lr: float, device):
        self.exp_avg = th.zeros(numel, dtype=th.float32, device=device)
        self.exp_avg_sq = th.zeros(numel, dtype=th.float32, device=device)
        self.step_count = 0
        self.param_groups = [{"lr": lr, "betas": (0.9, 0.999), "eps": 1e-8}]


class UpdateRoute(NamedTuple):
    """what `_OffPolicyFlatAgent._update_net_route` decides"""
    route: str                       # "ring_loop" | "per_loop" | "ring_step" | "batch_step" | "per_step"
    update_path: str                 # what `update_path` reads after the call
    per_path: Optional[str]          # what `per_path` reads after it (None: the agent names no prioritised route; left as it is)
    source: object = None            # what the buffer handed over for the route: ring_for_fused_sample's / per_for_fused_loop's tuple


class _OffPolicyFlatAgent(AgentBase):
    """What the off-policy agents on the HIP steps share (AgentSAC / AgentModSAC, AgentTD3 / AgentDDPG): networks as `nn.Module`s bound
    to flat fp32 blocks (the bind table), optimisers as `_FlatAdamState`s, the checkpoint round trip, and `update_net` -- a decision that
    launches nothing (`_update_net_route`) and one executor.  A subclass builds its nets with `_bind`, names its optimisers
    (`_optimizers`; `_set_step_counts` writes their `step_count`s, what a checkpoint stores) and provides the calls into ops
    (`_update_on_batch`, `_update_from_ring`, `_update_ring_loop`, `_update_per_loop`), `_step_kwargs(buffer, update_t, noise=None)` (the
    keyword arguments of the three per-step calls for step `update_t`) and its own reasons for leaving the one-call routes:
    `_ring_step_reason()`, and `_ring_loop_reason(buffer, ring)` on what the buffer's ring_for_fused_sample returned (maybe None)."""
    sample_ids_ahead = True          # update_net draws the sample ids of all its steps with one th.randint (AgentSAC reads args)
    _ring_loop_path = ""             # `update_path` of update_net's loop as one C call
    _per_why = ""                    # `update_path` behind "per step: " under prioritised replay

    def __init__(self, net_dims: List[int], state_dim: int, action_dim: int, gpu_id: int = 0, args: Config = None):
        super().__init__(net_dims, state_dim, action_dim, gpu_id, args)
        self.if_off_policy = True
        self._binds = {}                           # attribute name of a module -> the FlatNet that ties it to its flat block
        self.update_path = None                    # which route the last update_net took: "one C call ..." / "per step: <reason>"
        self.per_path = None                       # which route the last prioritised update_net took (None: none yet / not named)
        self.rollout_path = None                   # which route the last rollout took
        self._step = 0                             # the critic optimiser's Adam step = update steps taken
        self._objs = th.zeros(2, dtype=th.float32, device=self.device)
        self.objs_all = None                       # (update_times, 2) device tensor: the last update_net's (obj_critic, obj_actor) per step
        self._td_error = None                      # per-sample td errors of a prioritised step

    # ---- modules <-> flat blocks ------------------------------------------------------------------------
    def _bind(self, name: str, module: nn.Module, slices, flat: TEN) -> None:
        """`module` becomes the attribute `name`, its parameters views into `flat` in the order of `slices`"""
        self._binds[name] = FlatNet(module, _Slices(slices), flat)
        setattr(self, name, module)

    def _on_act_replaced(self):
        bind = getattr(self, "_binds", {}).get("_act")
        if bind is not None and self._act is not None and not bind.is_bound(self._act):
            self._act = self._act.to(self.device)
            bind.bind(self._act)

    def _sync_modules(self):
        for name, bind in self._binds.items():
            mod = getattr(self, name)
            if not bind.is_bound(mod):
                bind.bind(mod)

    # ---- checkpoints ------------------------------------------------------------------------------------
    def _optimizers(self) -> tuple:
        return self.act_optimizer, self.cri_optimizer

    def _checkpoint_extras(self, if_save: bool):
        """what a subclass stamps onto its optimisers before a save / reads back after a load beyond `_step` and `rng_counter`"""

    def save_or_load_agent(self, cwd: str, if_save: bool):
        """AgentBase.save_or_load_agent; the optimisers carry their Adam step counts and the Philox counter, so a resumed agent
        continues bit for bit"""
        if if_save:
            self._set_step_counts()
            for opt in self._optimizers():
                opt.rng_counter = self.rng_counter
            self._checkpoint_extras(True)
        super().save_or_load_agent(cwd, if_save)
        if not if_save:
            for opt in self._optimizers():
                opt.exp_avg = opt.exp_avg.to(self.device, th.float32).contiguous()
                opt.exp_avg_sq = opt.exp_avg_sq.to(self.device, th.float32).contiguous()
            self._step = int(self.cri_optimizer.step_count)
            self.rng_counter = int(getattr(self.act_optimizer, "rng_counter", self.rng_counter))
            self._checkpoint_extras(False)
            for name in self._binds:
                if name != "_act" and getattr(self, name, None) is not None:
                    setattr(self, name, getattr(self, name).to(self.device))
            self._on_act_replaced()
            self._sync_modules()

    # ---- one step -----------------------------------------------------------------------------------------
    def _per_step(self, buffer, objs_out: TEN, *args, uniform: Optional[TEN] = None, **kwargs):
        """one step on a prioritised sample: importance weights into the critic objective, td errors back into the trees"""
        *batch, is_weight, is_index = buffer.sample_for_per(self.batch_size) if uniform is None else buffer.sample_for_per(self.batch_size, uniform)
        if self._td_error is None or self._td_error.numel() != is_weight.numel():
            self._td_error = th.empty_like(is_weight)
        self._update_on_batch(batch, objs_out, *args, is_weight=is_weight, td_error_out=self._td_error, buffer=buffer, **kwargs)
        buffer.td_error_update_for_per(is_index, self._td_error)

    @_hip.on_device
    def update_objectives(self, buffer, update_t: int, ids: Optional[TEN] = None, noises=None) -> Tuple[float, float]:
        """one step of the reference's `update_objectives`.  `ids` / `noises` inject the random draws."""
        assert isinstance(update_t, int)
        self._sync_modules()
        kw = self._step_kwargs(buffer, update_t, noises)
        if self.if_use_per:
            self._per_step(buffer, self._objs, **kw)
        else:
            self._update_on_batch(buffer.sample(self.batch_size, ids=ids), self._objs, buffer=buffer, **kw)       # HIP K9
        oc, oa = self._objs.cpu().tolist()
        _hip.check_async_faults()          # the stream is drained: a skipped optimiser step (grid-wait timeout) raises here
        return oc, oa

    # ---- update_net: the decision ... ---------------------------------------------------------------------
    def _ring_step_reason(self) -> Optional[str]:
        """None when this agent's step can take the replay sample itself from the ring and the ids, else why it reads a finished batch"""
        return None

    def _per_route(self, buffer) -> tuple:
        """(`per_path`, per_for_fused_loop's tuple or None) of a prioritised update_net; the default names no route and steps"""
        return None, None

    def _update_net_route(self, buffer) -> UpdateRoute:
        """Which route `update_net(buffer)` takes and what `update_path` / `per_path` say about it.  Launches nothing: it reads the
        agent's switches and asks the buffer what it offers (ring_for_fused_sample, per_for_fused_loop)."""
        if self.if_use_per:
            per_path, per = self._per_route(buffer)
            return UpdateRoute("per_loop" if per else "per_step", "per step: " + self._per_why, per_path, per or None)
        ring, why = None, self._ring_step_reason()
        if why is None:
            ring = (getattr(buffer, "ring_for_fused_sample", None) and buffer.ring_for_fused_sample(self.batch_size)) or None
            why = self._ring_loop_reason(buffer, ring)
        if why is None:
            return UpdateRoute("ring_loop", self._ring_loop_path, None, ring)
        return UpdateRoute("ring_step" if ring else "batch_step", "per step: " + why, None, ring)

    # ---- ... and its execution ----------------------------------------------------------------------------
    def _before_update_net(self, buffer):
        """what a subclass does to the buffer ahead of the loop"""

    @_hip.on_device
    def update_net(self, buffer, per_uniform: Optional[TEN] = None) -> Tuple[float, float]:
        """AgentBase.update_net (:172-189) with ONE host sync: the per-step objectives stay on the device until the end.  The route is
        `_update_net_route`'s; `update_path` / `per_path` name it.
        `per_uniform` (update_times, num_seqs, batch_size // num_seqs) in [0, 1) injects the prioritised sampler's random numbers (tests)."""
        self._before_update_net(buffer)
        self._sync_modules()
        update_times = int(buffer.cur_size * self.repeat_times / self.batch_size)
        if update_times < 1:
            return 0.0, 0.0
        objs = self.objs_all = th.zeros((update_times, 2), dtype=th.float32, device=self.device)
        id_all = id_rows = None
        if not self.if_use_per and self.sample_ids_ahead:
            # the sample ids of ALL the steps in one th.randint (the reference draws batch_size of them per step, replay_buffer.py:121-122:
            # same distribution, same generator, one launch instead of `update_times`; nothing is written to the buffer inside this loop)
            id_all = th.randint((buffer.cur_size - 1) * buffer.num_seqs, size=(update_times, self.batch_size), requires_grad=False,
                                device=self.device)
            id_rows = id_all.unbind(0)
        route, self.update_path, per_path, src = self._update_net_route(buffer)
        if per_path is not None:
            self.per_path = per_path
        if route == "ring_loop":
            self._update_ring_loop(buffer, src, id_all, objs)
        elif route == "per_loop":
            self._update_per_loop(buffer, src, objs, per_uniform)
        else:
            for t in range(update_times):
                kw = self._step_kwargs(buffer, t)
                if route == "per_step":
                    self._per_step(buffer, objs[t], uniform=None if per_uniform is None else per_uniform[t], **kw)
                elif route == "ring_step":
                    self._update_from_ring(buffer, src, id_rows[t], objs[t], **kw)
                else:       # (the batch is consumed before the next draw)
                    self._update_on_batch(buffer.sample(self.batch_size, ids=None if id_rows is None else id_rows[t], reuse=True), objs[t],
                                          buffer=buffer, **kw)
        o = objs.cpu().numpy()
        _hip.check_async_faults()          # the stream is drained: a skipped optimiser step (grid-wait timeout) raises here
        oa = o[:, 1][~np.isnan(o[:, 1])]   # (steps whose actor update was skipped log nan, AgentBase.py:186-188)
        return float(np.nanmean(o[:, 0])), float(oa.mean()) if oa.size else 0.0
