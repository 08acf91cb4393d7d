"""Shared by tests/test_criterion_cpu.py and tests/test_criterion_gpu.py: fp64 restatements of the critic objectives under `args.criterion`,
built from the oracle's own pieces with the torch criterion module itself applied -- that module is literally what the reference calls
(elegantrl/agents/AgentPPO.py:190, AgentSAC.py:60, :68).

  PPO   critic_objective: oracle/ppo_numpy.py:critic_value(keep=True) and mlp_backward with dv = l'(diff) * unmask / B, l and l' from the
        module and its autograd; the actor half stays oracle/ppo_numpy.py:actor_objective
  SAC   step_gradients: oracle/sac_torch.py:step_gradients with criterion(q_values, q_label.view(-1, 1).expand_as(q_values)) in the td
        term and criterion(cum_reward_mean, q_values.mean(dim=0)) in the fit term

Threshold of the kernel-level cases: the float32 median of |d| over the unmasked elements of the fp64 restatement, so that both arms of the
loss are exercised by construction; `assert_both_arms` holds every case to it (each arm at least a quarter of the unmasked elements)."""
from __future__ import annotations

from copy import deepcopy

import numpy as np
import torch as th

from oracle import ppo_numpy as O

MSE, SMOOTH_L1, HUBER = 0, 1, 2                      # include/erl_hip.h ERL_CRIT_*
# the library entries that take the criterion of the call (include/erl_hip.h, erl_criterion_next_call)
UPDATE_ENTRIES = ("erl_ppo_step_f32", "erl_ppo_update_f32", "erl_ppo_update_dp_f32", "erl_mlpn_ppo_step_f32", "erl_mlpn_ppo_step_discrete_f32",
                  "erl_ppo_step_discrete_f32", "erl_ppo_update_discrete_f32", "erl_sac_update_f32", "erl_sac_update_opt_f32",
                  "erl_sac_update_ring_f32", "erl_sac_update_ring_loop_f32", "erl_sac_update_per_loop_f32", "erl_sac_update_mod_f32",
                  "erl_sac_update_mod_ring_f32", "erl_sac_update_mod_ring_loop_f32", "erl_sac_update_mod_per_loop_f32",
                  "erl_sac_update_per_draw_loop_f32")


def module(kind: int, beta: float) -> th.nn.Module:
    if kind == MSE:
        return th.nn.MSELoss(reduction="none")
    if kind == SMOOTH_L1:
        return th.nn.SmoothL1Loss(reduction="none", beta=float(beta))
    assert kind == HUBER
    return th.nn.HuberLoss(reduction="none", delta=float(beta))


def closed_form(kind: int, beta: float, d: np.ndarray):
    """(l(d), l'(d)) of include/erl_hip.h's table, fp64"""
    d = np.asarray(d, np.float64)
    a = np.abs(d)
    if kind == MSE:
        return d * d, 2.0 * d
    if kind == SMOOTH_L1:
        return np.where(a < beta, 0.5 * d * d / beta, a - 0.5 * beta), np.clip(d, -beta, beta) / beta
    return np.where(a <= beta, 0.5 * d * d, beta * (a - 0.5 * beta)), np.clip(d, -beta, beta)


def module_loss_and_grad(crit: th.nn.Module, pred: np.ndarray, target: np.ndarray):
    """the module applied element-wise in fp64, and d loss / d pred by autograd"""
    with th.enable_grad():
        p = th.tensor(np.asarray(pred, np.float64), requires_grad=True)
        loss = crit(p, th.tensor(np.asarray(target, np.float64)))
        (g,) = th.autograd.grad(loss.sum(), p)
    return loss.detach().numpy(), g.numpy()


def median_threshold(abs_d: np.ndarray) -> float:
    return float(np.float32(np.median(np.asarray(abs_d, np.float64))))


def assert_both_arms(abs_d: np.ndarray, thr: float) -> None:
    """a case that cannot meet this is an error in the case, not a skip"""
    abs_d = np.asarray(abs_d, np.float64).reshape(-1)
    n = abs_d.size
    assert n >= 1
    below, above = int((abs_d < thr).sum()), int((abs_d > thr).sum())
    if n == 1:                                      # one element sits on its own median: the quadratic / linear boundary itself
        return
    assert 4 * below >= n and 4 * above >= n, f"{below} below and {above} above the threshold {thr} of {n} unmasked elements"


# ---- PPO ---------------------------------------------------------------------------------------------------------------------------
def ppo_diff(state, reward_sum, critic: O.Mlp):
    return O.critic_value(state, critic) - reward_sum


def ppo_critic_objective(crit: th.nn.Module):
    """a drop-in for oracle/ppo_numpy.py:critic_objective under `crit`"""
    def critic_objective(state, reward_sum, unmask, critic: O.Mlp):
        dt = state.dtype
        v, cache = O.critic_value(state, critic, keep=True)
        um = unmask.astype(dt)
        loss, dl = module_loss_and_grad(crit, v, reward_sum)
        obj = (loss.astype(dt) * um).mean()
        B = dt.type(state.shape[0])
        dv = (dl.astype(dt) * um / B)[:, None]
        gw, gb = O.mlp_backward(dv, critic, cache)
        return obj, gw, gb
    return critic_objective


def ppo_flat_grads(buf, ids, actor, critic, clip, lam_ent, crit: th.nn.Module, objective="reference", discrete=False):
    """tests/test_kernels_gpu.py:oracle_flat_grads in fp64 with the critic half under `crit`: (actor grads, critic grads, 3 objectives, diff)"""
    dt = np.float64
    states, actions, um, lp, adv, rs = buf
    H = states.shape[0]
    i0, i1 = O.split_ids(ids, H)
    s = states[i0, i1].astype(dt)
    critic = critic.astype(dt)
    oc, gw, gb = ppo_critic_objective(crit)(s, rs[i0, i1].astype(dt), um[i0, i1], critic)
    gc = np.concatenate([x.reshape(-1) for pair in zip(gw, gb) for x in pair])
    if discrete:
        os_, oe, gw, gb = O.actor_objective_discrete(s, actions[i0, i1], lp[i0, i1].astype(dt), adv[i0, i1].astype(dt), um[i0, i1], actor.astype(dt),
                                                     clip, lam_ent)
        ga = np.concatenate([x.reshape(-1) for pair in zip(gw, gb) for x in pair])
    else:
        os_, oe, gw, gb, gsl = O.actor_objective(s, actions[i0, i1].astype(dt), lp[i0, i1].astype(dt), adv[i0, i1].astype(dt), um[i0, i1],
                                                 actor.astype(dt), clip, lam_ent, objective)
        ga = np.concatenate([x.reshape(-1) for pair in zip(gw, gb) for x in pair] + [gsl.reshape(-1)])
    diff = ppo_diff(s, rs[i0, i1].astype(dt), critic)
    return ga, gc, np.array([oc, os_, oe], dtype=np.float64), diff[um[i0, i1].astype(bool)]


# ---- SAC ---------------------------------------------------------------------------------------------------------------------------
def sac_step_gradients(stepper, batch, eps_next, eps_cur, *, dtype, crit: th.nn.Module, is_weight=None, cum_reward=None,
                       lambda_fit_cum_r: float = 0.0, update_actor: bool = True):
    """oracle/sac_torch.py:step_gradients, statement for statement, with `crit` where the reference calls self.criterion; info also holds
    "diff": q_values - q_label of the unmasked rows"""
    cast = lambda x: None if x is None else x.detach().to(dtype)  # noqa: E731
    act, cri, tar = (deepcopy(m).to(dtype) for m in (stepper.act, stepper.cri, stepper.cri_target))
    alpha_log = stepper.alpha_log.detach().to(dtype).requires_grad_(True)
    state, action, reward, undone, unmask, next_state = (cast(x) for x in batch)
    eps_next, eps_cur, is_weight, cum_reward = cast(eps_next), cast(eps_cur), cast(is_weight), cast(cum_reward)
    gamma, tau = stepper.gamma, stepper.tau
    for m in (act, cri, tar):
        m.zero_grad()
    with th.enable_grad():
        with th.no_grad():
            next_action, next_logprob = act.get_action_logprob(next_state, eps_next)
            next_q = th.min(tar.get_q_values(next_state, next_action), dim=1)[0]
            q_label = reward + undone * gamma * (next_q - next_logprob * alpha_log.exp())
        q_values = cri.get_q_values(state, action)
        td = crit(q_values, q_label.view(-1, 1).expand_as(q_values)).mean(dim=1) * unmask
        obj_critic = td.mean() if is_weight is None else (td * is_weight).mean()
        if lambda_fit_cum_r:
            cum_reward_mean = cum_reward.mean().repeat(q_values.shape[1])
            obj_critic = obj_critic + crit(cum_reward_mean, q_values.mean(dim=0)).mean() * lambda_fit_cum_r
        obj_critic.backward()
        with th.no_grad():
            for t, c in zip(tar.parameters(), cri.parameters()):
                t.copy_(c * tau + t * (1.0 - tau))
        action_pg, logprob = act.get_action_logprob(state, eps_cur)
        (alpha_log * (stepper.target_entropy - logprob).detach()).mean().backward()
        grads = {k: p.grad.detach().clone() for k, p in cri.named_parameters()}
        grads["alpha_log"] = alpha_log.grad.detach().clone()
        obj_actor = th.tensor(float("nan"), dtype=dtype)
        if update_actor:
            obj_actor = (tar(state, action_pg).mean() - logprob * alpha_log.exp().detach()).mean()
            (-obj_actor).backward()
            grads.update({k: p.grad.detach().clone() for k, p in act.named_parameters()})
    diff = (q_values - q_label.view(-1, 1)).detach()[unmask > 0]
    info = {"obj_critic": obj_critic.item(), "obj_actor": obj_actor.item(), "td_error": td.detach().clone(), "diff": diff.double().numpy()}
    return grads, info


def sac_references(case, x, crit: th.nn.Module):
    """tests/sac_gradient_cases.py:references under `crit`"""
    out = []
    for dtype in (th.float64, th.float32):
        grads, info = sac_step_gradients(x.stepper, x.batch, x.eps_next, x.eps_cur, dtype=dtype, crit=crit, is_weight=x.is_weight,
                                         cum_reward=x.cum_reward, lambda_fit_cum_r=case.lambda_fit, update_actor=case.update_actor)
        out.append(({k: v.double().numpy() for k, v in grads.items()}, info))
    return out


def sac_stepper_under(crit: th.nn.Module, base):
    """oracle/sac_torch.py:SacStepper (or ModSacStepper) whose `step` calls `crit` where the reference calls self.criterion
    (AgentSAC.py:60, :68); everything else is the oracle's own step, statement for statement"""
    class CriterionStepper(base):
        def step(self, batch, eps_next, eps_cur, is_weight=None, cum_reward=None, lambda_fit_cum_r: float = 0.0):
            state, action, reward, undone, unmask, next_state = batch
            with th.no_grad():
                next_action, next_logprob = self.act.get_action_logprob(next_state, eps_next)
                next_q = th.min(self.cri_target.get_q_values(next_state, next_action), dim=1)[0]
                q_label = reward + undone * self.gamma * (next_q - next_logprob * self.alpha_log.exp())
            q_values = self.cri.get_q_values(state, action)
            td = crit(q_values, q_label.view(-1, 1).expand_as(q_values)).mean(dim=1) * unmask
            self.td_error = td.detach().clone()
            obj_critic = td.mean() if is_weight is None else (td * is_weight).mean()
            if lambda_fit_cum_r:
                cum_reward_mean = cum_reward.mean().repeat(q_values.shape[1])
                obj_critic = obj_critic + crit(cum_reward_mean, q_values.mean(dim=0)).mean() * lambda_fit_cum_r
            self._opt(self.cri_opt, obj_critic)
            with th.no_grad():
                for tar, cur in zip(self.cri_target.parameters(), self.cri.parameters()):
                    tar.data.copy_(cur.data * self.tau + tar.data * (1.0 - self.tau))
            action_pg, logprob = self.act.get_action_logprob(state, eps_cur)
            self._opt(self.alpha_opt, (self.alpha_log * (self.target_entropy - logprob).detach()).mean())
            alpha = self.alpha_log.exp().detach()
            with th.no_grad():
                self.alpha_log[:] = self.alpha_log.clamp(-16, 2)
            obj_actor = (self.cri_target(state, action_pg).mean() - logprob * alpha).mean()
            self._opt(self.act_opt, -obj_actor)
            return obj_critic.item(), obj_actor.item()
    return CriterionStepper
