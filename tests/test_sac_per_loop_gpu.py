"""AgentSAC.update_net with prioritised replay as ONE C call (erl_sac_update_per_loop_f32; args.per_loop_in_c, the default) against the
per-step route (AgentSAC._per_step: th.rand, erl_per_sample_f32, erl_replay_sample_rows_f32, the step, fmod / div, erl_per_update_f32):
two agents from one seed, the same ring contents and the same injected uniforms must end bit-identical in everything the loop writes.
per_alpha = 0.6, so the priorities move between the steps and step t + 1 draws from the trees step t updated."""
import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

N, S, A, B, H, STEPS = 8, 11, 3, 64, 16, 4
NETS = {"one-launch-form": (256, 256), "layered-form": (64, 48, 32)}
RINGS = {"partly-filled": (64, 2), "full-and-wrapped": (32, 3)}          # max_size, rollouts of 16 rows


def _make(agent_class, net, max_size, rollouts, per_loop, **extra):
    from elegantrl_amd.envs import SynVecEnv
    from elegantrl_amd.train import Config, ReplayBuffer
    args = Config(agent_class, SynVecEnv, {"env_name": "SynVecEnv", "num_envs": N, "max_step": 50, "state_dim": S, "action_dim": A,
                                           "if_discrete": False})
    args.net_dims, args.horizon_len, args.batch_size, args.if_use_per, args.random_seed = list(net), H, B, True, 3
    args.per_alpha, args.per_beta, args.per_loop_in_c, args.quiet = 0.6, 0.4, per_loop, True
    for k, v in extra.items():
        setattr(args, k, v)
    th.manual_seed(5)
    agent = agent_class(args.net_dims, S, A, gpu_id=0, args=args)
    env = SynVecEnv(N, S, A, max_step=50, gpu_id=0, seed=1)
    agent.last_state = env.reset()[0]
    buf = ReplayBuffer(max_size=max_size, state_dim=S, action_dim=A, gpu_id=0, num_seqs=N, if_use_per=True, args=args)
    for _ in range(rollouts):
        buf.update(agent.explore_env(env, H))
    agent.repeat_times = STEPS * B / buf.cur_size             # update_times = int(cur_size * repeat_times / batch_size) = 4
    return agent, buf


def _spy(monkeypatch):
    """counts the entries into the loop wrapper and into the per-step route"""
    from elegantrl_amd import ops
    from elegantrl_amd.agents import AgentSAC
    calls = {"loop": 0, "per_step": 0}
    loop, per_step = ops.sac_update_per_loop, AgentSAC._per_step

    def spy_loop(*a, **k):
        calls["loop"] += 1
        return loop(*a, **k)

    def spy_step(self, *a, **k):
        calls["per_step"] += 1
        return per_step(self, *a, **k)
    monkeypatch.setattr(ops, "sac_update_per_loop", spy_loop)
    monkeypatch.setattr(AgentSAC, "_per_step", spy_step)
    return calls


@pytest.mark.parametrize("ring", list(RINGS))
@pytest.mark.parametrize("net", list(NETS))
def test_per_loop_in_c_is_bit_identical_to_the_per_step_route(net, ring, monkeypatch):
    from elegantrl_amd.agents import AgentSAC
    max_size, rollouts = RINGS[ring]
    calls = _spy(monkeypatch)
    u = th.rand((STEPS, N, B // N), device="cuda:0", generator=th.Generator(device="cuda:0").manual_seed(11))
    u[0, 0, 0], u[1, -1, -1] = 0.0, float(1 - 2.0 ** -24)
    a, ba = _make(AgentSAC, NETS[net], max_size, rollouts, True)
    b, bb = _make(AgentSAC, NETS[net], max_size, rollouts, False)
    assert ba.if_full == (ring == "full-and-wrapped") and ba.cur_size == min(max_size, rollouts * H) and ba.p == bb.p
    assert th.equal(ba._ring.block, bb._ring.block) and th.equal(ba.sum_trees.sum, bb.sum_trees.sum)
    trees0 = ba.sum_trees.sum.clone()
    oa = a.update_net(ba, per_uniform=u)
    assert calls == {"loop": 1, "per_step": 0} and "one C call" in a.per_path
    ob = b.update_net(bb, per_uniform=u)
    assert calls == {"loop": 1, "per_step": STEPS} and "per step" in b.per_path and "per_loop_in_c is off" in b.per_path
    assert oa == ob and all(np.isfinite(x) for x in oa)
    for name in ("_actor_flat", "_critic_flat", "_target_flat", "alpha_log"):
        assert th.equal(getattr(a, name), getattr(b, name)), name
    for opt in ("act_optimizer", "cri_optimizer", "alpha_optim"):                  # all six Adam moment vectors
        x, y = getattr(a, opt), getattr(b, opt)
        assert th.equal(x.exp_avg, y.exp_avg) and th.equal(x.exp_avg_sq, y.exp_avg_sq), opt
        assert x.step_count == y.step_count == STEPS
    assert th.equal(ba.sum_trees.sum, bb.sum_trees.sum) and th.equal(ba.sum_trees.min, bb.sum_trees.min)
    assert not th.equal(ba.sum_trees.sum, trees0)                                    # the priorities did move
    assert th.equal(ba.ids0, bb.ids0) and th.equal(ba.ids1, bb.ids1) and ba.ids0.shape == (B,)
    assert a._step == b._step == STEPS
    assert a.objs_all.shape == (STEPS, 2) and th.equal(a.objs_all, b.objs_all) and bool(th.isfinite(a.objs_all).all())   # the (4, 2) objectives
    assert len({float(x) for x in a.objs_all[:, 0]}) == STEPS


def test_the_default_route_is_the_loop(monkeypatch):
    """no injection, only the seed: a default AgentSAC with PER enters ops.sac_update_per_loop exactly once and never _per_step"""
    from elegantrl_amd.agents import AgentSAC
    from elegantrl_amd.envs import SynVecEnv
    from elegantrl_amd.train import Config, ReplayBuffer
    calls = _spy(monkeypatch)
    args = Config(AgentSAC, SynVecEnv, {"env_name": "SynVecEnv", "num_envs": N, "max_step": 50, "state_dim": S, "action_dim": A,
                                        "if_discrete": False})
    args.net_dims, args.horizon_len, args.batch_size, args.if_use_per, args.quiet = [256, 256], H, B, True, True
    assert not hasattr(args, "per_loop_in_c")                     # the switch is not named at all: the agent's own default decides
    th.manual_seed(5)
    agent = AgentSAC(args.net_dims, S, A, gpu_id=0, args=args)
    assert agent.per_loop_in_c and agent.per_path is None
    env = SynVecEnv(N, S, A, max_step=50, gpu_id=0, seed=1)
    agent.last_state = env.reset()[0]
    buf = ReplayBuffer(max_size=64, state_dim=S, action_dim=A, gpu_id=0, num_seqs=N, if_use_per=True, args=args)
    buf.update(agent.explore_env(env, H))
    buf.update(agent.explore_env(env, H))
    agent.repeat_times = STEPS * B / buf.cur_size
    th.manual_seed(9)
    objs = agent.update_net(buf)
    assert calls == {"loop": 1, "per_step": 0}
    assert "one C call" in agent.per_path and "erl_sac_update_per_loop_f32" in agent.per_path
    assert all(np.isfinite(o) for o in objs) and agent._step == STEPS and agent.act_optimizer.step_count == STEPS
    leaves = buf.sum_trees.sum.view(N, -1)[:, buf.sum_trees.leaves:buf.sum_trees.leaves + buf.cur_size]
    assert int((leaves != 10.0).sum()) > 20 and float(leaves.max()) <= 10.0 and float(leaves.min()) > 0.0
    assert buf.ids0.shape == (B,) and int(buf.ids0.max()) <= buf.cur_size - 2
    assert th.equal(buf.ids1, th.arange(N, device=buf.device).repeat_interleave(B // N))


def test_mod_sac_and_the_cumulative_reward_term_keep_the_per_step_route(monkeypatch):
    from elegantrl_amd.agents import AgentModSAC, AgentSAC
    calls = _spy(monkeypatch)
    agent, buf = _make(AgentModSAC, (64, 48, 32), 64, 2, True)
    objs = agent.update_net(buf)
    assert calls == {"loop": 0, "per_step": STEPS} and "per step" in agent.per_path and "AgentModSAC" in agent.per_path
    assert np.isfinite(objs[0]) and agent._step == STEPS
    agent, buf = _make(AgentSAC, (64, 48, 32), 64, 2, True, lambda_fit_cum_r=0.3)
    assert agent.lambda_fit_cum_r == 0.3
    objs = agent.update_net(buf)
    assert calls == {"loop": 0, "per_step": 2 * STEPS} and "per step" in agent.per_path and "lambda_fit_cum_r" in agent.per_path
    assert all(np.isfinite(o) for o in objs) and agent._step == STEPS
