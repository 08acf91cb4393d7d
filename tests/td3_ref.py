"""Plain torch restatement of one TD3 / DDPG update step (elegantrl/agents/AgentTD3.py:34-70 in the reference), in fp64 by default:
the oracle of tests/test_td3_golden_cpu.py (against the recorded reference run, tests/golden/td3_small.npz) and of tests/test_td3_gpu.py
(against the HIP step, csrc/td3.hip).  Every random draw is an argument.

    next_action = clip(tanh(act(next_state)) + policy_noise_std * noise, -1, 1)      the CURRENT actor; the action is clipped, not the noise
    q_label     = reward + undone * gamma * min_e cri_target(next_state, next_action)
    td_error    = mean_e criterion(q_e, q_label) * unmask;  obj_critic = mean(td_error [* is_weight])
    critic: clip_grad_norm_ + Adam, soft update of cri_target
    update_actor:  obj_actor = mean_{b, e} cri(state, tanh(act(state)))  -- the critic after its step; actor: clip + Adam on -obj_actor,
                   soft update of act_target;  otherwise obj_actor = nan and nothing of the actor moves

With E = 1 and policy_noise_std = 0 this is the DDPG oracle under deviation D1: the per-sample objective
criterion(q_i, label_i) * unmask_i, not the reference's (B, B) broadcast (AgentBase.py:206-207).
"""
import copy
import math

import torch as th
from torch import nn


def build_mlp(dims):
    layers = []
    for d_in, d_out in zip(dims[:-1], dims[1:]):
        layers += [nn.Linear(d_in, d_out), nn.GELU()]
    return nn.Sequential(*layers[:-1])


class _Net(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.net = build_mlp(dims)


class Td3Ref:
    def __init__(self, net_dims, S, A, E, *, lr, gamma, tau, max_norm, policy_noise_std, criterion=None, dtype=th.float64, seed=0):
        g = th.Generator().manual_seed(seed)
        self.S, self.A, self.E, self.dtype = S, A, E, dtype
        self.lr, self.gamma, self.tau, self.max_norm, self.policy_noise_std = lr, gamma, tau, max_norm, policy_noise_std
        self.criterion = criterion if criterion is not None else nn.MSELoss(reduction="none")
        self.act, self.cri = _Net([S, *net_dims, A]).to(dtype), _Net([S + A, *net_dims, E]).to(dtype)
        with th.no_grad():                         # seeded values of a useful size (tests that load recorded nets overwrite them)
            for net in (self.act, self.cri):
                for p in net.parameters():
                    p.copy_(th.randn(p.shape, generator=g, dtype=th.float32) * (1.0 / math.sqrt(p.shape[-1]) if p.dim() == 2 else 0.1))
        self.sync_targets()

    def sync_targets(self):
        """targets = copies of the current nets, fresh Adam state"""
        self.act_target, self.cri_target = copy.deepcopy(self.act), copy.deepcopy(self.cri)
        self.act_opt = th.optim.Adam(self.act.parameters(), self.lr)
        self.cri_opt = th.optim.Adam(self.cri.parameters(), self.lr)

    def load(self, act_sd, cri_sd):
        """state dicts of numpy arrays / tensors (keys net.0.weight ...) -> current nets and targets"""
        for net, sd in ((self.act, act_sd), (self.cri, cri_sd)):
            net.load_state_dict({k: th.as_tensor(v).to(self.dtype) for k, v in sd.items()})
        self.sync_targets()

    def policy(self, state, action_std=0.0, noise=None):
        """Actor.forward (action_std 0) / Actor.get_action"""
        a = self.act.net(state.to(self.dtype)).tanh()
        return a if not action_std else (a + action_std * noise.to(self.dtype)).clip(-1.0, 1.0)

    def _opt_step(self, opt, net, objective):
        opt.zero_grad()
        objective.backward()
        nn.utils.clip_grad_norm_(net.parameters(), self.max_norm)
        opt.step()

    def _soft(self, tar, cur):
        with th.no_grad():
            for t, c in zip(tar.parameters(), cur.parameters()):
                t.copy_(c * self.tau + t * (1.0 - self.tau))

    def step(self, batch, noise, update_actor, is_weight=None):
        """-> (obj_critic, obj_actor, td_error (B,) tensor)"""
        state, action, reward, undone, unmask, next_state = [th.as_tensor(x).to(self.dtype) for x in batch]
        with th.enable_grad():
            with th.no_grad():
                a_next = self.act.net(next_state).tanh()
                if self.policy_noise_std:
                    a_next = (a_next + self.policy_noise_std * th.as_tensor(noise).to(self.dtype)).clip(-1.0, 1.0)
                next_q = self.cri_target.net(th.cat((next_state, a_next), 1)).min(dim=1)[0]
                label = reward + undone * self.gamma * next_q
            q = self.cri.net(th.cat((state, action), 1))
            td = self.criterion(q, label[:, None].expand_as(q)).mean(dim=1) * unmask
            obj_c = (td * th.as_tensor(is_weight).to(self.dtype)).mean() if is_weight is not None else td.mean()
            self._opt_step(self.cri_opt, self.cri, obj_c)
            self._soft(self.cri_target, self.cri)
            obj_a = float("nan")
            if update_actor:
                o = self.cri.net(th.cat((state, self.act.net(state).tanh()), 1)).mean()
                self._opt_step(self.act_opt, self.act, -o)
                self._soft(self.act_target, self.act)
                obj_a = float(o.detach())
        return float(obj_c.detach()), obj_a, td.detach()


def gather(ring, ids, sample_len):
    """ReplayBuffer.sample given the drawn ids (elegantrl/train/replay_buffer.py:120-134): ring = dict of (rows, N, .) arrays"""
    ids = th.as_tensor(ids)
    i0, i1 = ids % sample_len, ids // sample_len
    t = {k: th.as_tensor(v) for k, v in ring.items()}
    return (t["states"][i0, i1], t["actions"][i0, i1], t["rewards"][i0, i1], t["undones"][i0, i1].to(th.float32),
            t["unmasks"][i0, i1].to(th.float32), t["states"][i0 + 1, i1]), (i0, i1)
