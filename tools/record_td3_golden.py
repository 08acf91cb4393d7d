"""Record tests/golden/td3_small.npz by RUNNING the reference's AgentTD3 on the CPU (gpu_id=-1).

    python tools/record_td3_golden.py --reference <checkout of the reference>     (or ERL_REFERENCE=<checkout>)

Nothing of the reference is copied: only what its agent computes on our inputs is stored.  `Normal.sample` and `torch.randint` are
wrapped inside this process, so every draw the agent makes is logged beside what it returns -- tests/test_td3_golden_cpu.py replays the
steps with tests/td3_ref.py, tests/test_td3_gpu.py with the HIP step, from exactly those numbers.  The wrapped `Normal.sample` draws
eps = randn and returns loc + eps * scale, which is what `torch.normal(loc, scale)` computes; eps is what is logged.

Shape: 4 envs, S 11, A 3, a 40-row rollout on oracle/make_golden.py's ScriptedVecEnv, net (64, 32), batch 64, 8 critic heads, 4 updates
with update_freq 2: steps 0 and 2 update the actor, steps 1 and 3 log nan.  The learning rate, 1e-4, is fixed here before any replay:
Adam's first steps move a weight by about lr whatever its gradient's size, so where a gradient is small against the fp32 rounding of
the reference's own backward pass, an fp64 replay differs from the record by a fraction of lr -- with 1e-4 that stays below the 2e-6 the
golden tests allow on a weight.  The recorder asserts one `Normal.sample` per explore_action and per update, the nan pattern, and that
the reference's AgentDDPG constructs and steps at this shape as well."""
import argparse
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S, A, ROWS, NET, B, E, N_UPD, SEED = 4, 11, 3, 40, (64, 32), 64, 8, 4, 20250
LR, GAMMA, REWARD_SCALE, TAU, UPDATE_FREQ, POLICY_NOISE, EXPLORE_NOISE = 1e-4, 0.98, 0.5, 5e-3, 2, 0.10, 0.05


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("ERL_REFERENCE"), help="a checkout of the reference (or ERL_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "td3_small.npz"))
    opt = ap.parse_args()
    if not opt.reference:
        ap.error("--reference (or ERL_REFERENCE) is needed: the golden is what the reference computes")
    sys.path.insert(0, ROOT)
    from oracle.make_golden import ScriptedVecEnv, net_arrays, np32            # helpers only; nothing under oracle/ changes
    sys.path.insert(0, opt.reference)
    from elegantrl.agents.AgentTD3 import AgentDDPG, AgentTD3
    from elegantrl.train.config import Config
    from elegantrl.train.replay_buffer import ReplayBuffer
    assert os.path.abspath(sys.modules[AgentTD3.__module__].__file__).startswith(os.path.abspath(opt.reference))

    def config(cls):
        args = Config(cls, None, {"env_name": "scripted", "num_envs": N, "max_step": 100, "state_dim": S, "action_dim": A, "if_discrete": False})
        assert args.if_off_policy
        args.net_dims = list(NET)
        args.batch_size, args.learning_rate, args.gamma, args.reward_scale, args.soft_update_tau = B, LR, GAMMA, REWARD_SCALE, TAU
        args.update_freq, args.num_ensembles, args.policy_noise_std, args.explore_noise_std = UPDATE_FREQ, E, POLICY_NOISE, EXPLORE_NOISE
        return args

    th.manual_seed(SEED)
    args = config(AgentTD3)
    agent = AgentTD3(args.net_dims, S, A, gpu_id=-1, args=args)
    assert (agent.update_freq, agent.num_ensembles, agent.policy_noise_std, agent.explore_noise_std) == (UPDATE_FREQ, E, POLICY_NOISE, EXPLORE_NOISE)
    g = {}
    g.update(net_arrays("act0", agent.act))
    g.update(net_arrays("cri0", agent.cri))

    Normal = th.distributions.normal.Normal
    real_sample, real_randint = Normal.sample, th.randint
    eps_log, ids_log = [], []

    def sample(self, sample_shape=th.Size()):
        shape = self._extended_shape(sample_shape)
        with th.no_grad():
            eps = th.randn(shape, dtype=self.loc.dtype)
            eps_log.append(eps.clone())
            return self.loc.expand(shape) + eps * self.scale.expand(shape)

    def randint(*a, **k):
        out = real_randint(*a, **k)
        ids_log.append(out.clone())
        return out

    Normal.sample, th.randint = sample, randint
    try:
        env = ScriptedVecEnv(N, S, A, SEED + 1)
        agent.last_state = env.reset()[0]
        g["first_state"] = np32(agent.last_state)
        th.set_grad_enabled(False)
        items = agent.explore_env(env, ROWS)
        assert len(eps_log) == ROWS and not ids_log                    # one Normal.sample per explore_action
        states, actions, rewards, undones, unmasks = items
        g.update(ro_states=np32(states), ro_actions=np32(actions), ro_rewards=np32(rewards), ro_undones=np32(undones),
                 ro_unmasks=np32(unmasks), ro_eps=np.stack([np32(e) for e in eps_log]), ro_last_state=np32(agent.last_state))
        assert (~g["ro_undones"]).any() and (~g["ro_unmasks"]).any()    # terminal and truncated rows both occur
        eps_log.clear()
        buf = ReplayBuffer(max_size=ROWS + 5, state_dim=S, action_dim=A, gpu_id=-1, num_seqs=N)
        buf.update(items)
        th.set_grad_enabled(True)
        objs = []
        for t in range(N_UPD):
            objs.append(agent.update_objectives(buf, t))
            assert len(eps_log) == t + 1 and len(ids_log) == t + 1      # one Normal.sample and one randint per update
            for tag, net in (("act", agent.act), ("actt", agent.act_target), ("cri", agent.cri), ("crit", agent.cri_target)):
                g.update(net_arrays(f"{tag}{t + 1}", net))
        th.set_grad_enabled(False)
        assert [bool(np.isnan(o[1])) for o in objs] == [t % UPDATE_FREQ != 0 for t in range(N_UPD)], objs
        g.update(ids=np.stack([np32(i) for i in ids_log]).astype(np.int64), noise=np.stack([np32(e) for e in eps_log]),
                 objs=np.array(objs, dtype=np.float64),
                 hyper=np.array([GAMMA, LR, args.clip_grad_norm, REWARD_SCALE, TAU, POLICY_NOISE, EXPLORE_NOISE], dtype=np.float64),
                 dims=np.array([N, S, A, ROWS, B, N_UPD, E, UPDATE_FREQ, *NET], dtype=np.int64))

        # the reference's AgentDDPG constructs and steps at this shape too (its (B, B) broadcast is why DDPG has no recorded golden: D1)
        eps_log.clear()
        ddpg = AgentDDPG(list(NET), S, A, gpu_id=-1, args=config(AgentDDPG))
        th.set_grad_enabled(True)
        oc, oa = ddpg.update_objectives(buf, 0)
        th.set_grad_enabled(False)
        assert np.isfinite(oc) and not eps_log                          # DDPG draws no policy noise
        print("AgentDDPG steps on the CPU at this shape: obj_critic", oc, "obj_actor", oa)
    finally:
        Normal.sample, th.randint = real_sample, real_randint
    np.savez_compressed(opt.out, **g)
    print("wrote", opt.out, os.path.getsize(opt.out), "bytes; objs", objs)


if __name__ == "__main__":
    main()
