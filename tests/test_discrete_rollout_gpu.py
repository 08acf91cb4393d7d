"""The one-launch discrete rollout and evaluation (csrc/rollout_discrete.hip: erl_rollout_discrete_cartpole_f32,
erl_eval_discrete_cartpole_f32) behind AgentDiscretePPO on CartPoleGpuVecEnv.  Teacher-forced: the policy rows are checked against an
fp64 restatement ON the recorded states, the env rows against a twin env stepped by the per-step kernel WITH the recorded actions, so
one legitimate flip of a draw cannot make everything after it differ."""
import os

import numpy as np
import pytest
import torch as th

from oracle import ppo_numpy as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 2e-6          # |u - CDF boundary| below which fp32 and fp64 may draw neighbouring actions (tests/test_discrete_gpu.py:50)
CASES = [(50, (64, 32), 40, 7, 0.25), (16, (32, 32), 9, 500, 1.0), (1000, (128, 64), 60, 500, 1.0), (300, (128, 128), 12, 500, 2.0)]


def make(N, net, max_step, reward_scale=1.0, env_seed=5, agent_seed=3, env_cls=None, fused=True, cls=None):
    from elegantrl_amd.agents import AgentDiscretePPO
    from elegantrl_amd.envs import CartPoleGpuVecEnv
    from elegantrl_amd.train import Config
    cls, env_cls = cls or AgentDiscretePPO, env_cls or CartPoleGpuVecEnv
    args = Config(cls, env_cls, {"env_name": "CartPole-v1", "num_envs": N, "max_step": max_step, "state_dim": 4, "action_dim": 2,
                                 "if_discrete": True})
    args.net_dims, args.reward_scale, args.random_seed, args.fused_rollout = list(net), reward_scale, 7, fused
    th.manual_seed(agent_seed)
    agent = cls(args.net_dims, 4, 2, gpu_id=0, args=args)
    with th.no_grad():
        g = th.Generator(device=DEV).manual_seed(agent_seed + 1)
        agent.act.state_avg[:] = 0.01 * th.randn(4, device=DEV, generator=g)          # CartPole's states are a few 1e-2 wide
        agent.act.state_std[:] = 0.05 + 0.2 * th.rand(4, device=DEV, generator=g)
        agent.act.net[-1].weight.mul_(6.0)          # logits far from uniform: every branch of the draw (spread(), test_discrete_gpu.py)
    env = env_cls(N, max_step=max_step, gpu_id=0, seed=env_seed)
    agent.last_state = env.reset()[0]
    return agent, env, args


def actor64(agent):
    f = lambda t: t.detach().cpu().numpy().astype(np.float64)  # noqa: E731
    lin = [m for m in agent.act.net if isinstance(m, th.nn.Linear)]
    return O.Mlp([f(m.weight) for m in lin], [f(m.bias) for m in lin], f(agent.act.state_avg), f(agent.act.state_std), None)


def policy64(agent, states):
    """fp64 softmax probabilities and CDF of the agent's policy on states (..., 4)"""
    p = O.softmax(O.actor_mean(states.reshape(-1, 4).cpu().numpy().astype(np.float64), actor64(agent)))
    return p, np.cumsum(p, axis=1)


def near_boundary(c, u):
    return (np.abs(c[:, :-1] - u.reshape(-1, 1).astype(np.float64)) < BAND).any(axis=1)       # (the last CDF entry is no boundary: u < 1)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"N{c[0]}-{c[1][0]}x{c[1][1]}-H{c[2]}")
def rollouts(request):
    """two consecutive one-launch rollouts with injected uniforms (env state, counters and rng_counter carry over), computed once"""
    N, net, H, max_step, rs = request.param
    agent, env, _ = make(N, net, max_step, rs)
    g = th.Generator(device=DEV).manual_seed(N + H)
    out = []
    for k in range(2):
        u = th.rand((H, N), device=DEV, generator=g)
        before, c0 = agent.last_state.clone(), agent.rng_counter
        items = agent._explore_vec_env(env, H, noise=u)
        assert agent.rollout_path == "one-launch"
        out.append(dict(u=u, before=before, c0=c0, items=items, last=agent.last_state.clone(), c1=agent.rng_counter,
                        env=(env.state.clone(), env.step_count.clone(), env.episode.clone())))
    return dict(agent=agent, N=N, H=H, max_step=max_step, rs=rs, out=out)


def test_policy_rows_against_fp64(rollouts):
    """band: 2e-6, as for the per-step kernel (the kernel's logits come from the same fp32 MFMA and GELU as the layered path's)"""
    agent, N, H = rollouts["agent"], rollouts["N"], rollouts["H"]
    for r in rollouts["out"]:
        states, actions, logprobs = r["items"][:3]
        assert actions.dtype == th.int32 and logprobs.dtype == th.float32 and states.dtype == th.float32
        assert states.shape == (H, N, 4) and actions.shape == logprobs.shape == (H, N)
        p, c = policy64(agent, states)
        u = r["u"].reshape(-1).cpu().numpy()
        ref = np.minimum((c <= u[:, None].astype(np.float64)).sum(axis=1), 1)
        got = actions.reshape(-1).cpu().numpy()
        near = near_boundary(c, u)
        dev = np.abs(c[:, 0] - u)[got != ref]
        print(f"cells {got.size}: {int((got != ref).sum())} differ from the fp64 draw, largest |u - CDF| among them {dev.max() if dev.size else 0:.3e}; "
              f"{int(near.sum())} within the band")
        np.testing.assert_array_equal(got[~near], ref[~near])
        assert (np.abs(got[near] - ref[near]) <= 1).all() and near.mean() < 0.01
        assert 0.05 < got.mean() < 0.95          # both actions are drawn
        lp_ref = O.categorical_logits(p)[np.arange(got.size), got]
        np.testing.assert_allclose(logprobs.reshape(-1).cpu().numpy(), lp_ref, rtol=1e-4, atol=1e-4)


def test_env_rows_against_the_per_step_twin(rollouts):
    from elegantrl_amd.envs import CartPoleGpuVecEnv
    N, H, rs = rollouts["N"], rollouts["H"], rollouts["rs"]
    twin = CartPoleGpuVecEnv(N, max_step=rollouts["max_step"], gpu_id=0, seed=5)
    twin.reset()
    n_term = n_trunc = 0
    for k, r in enumerate(rollouts["out"]):
        states, actions, logprobs, rewards, undones, unmasks = r["items"]
        assert rewards.dtype == th.float32 and undones.dtype == th.bool and unmasks.dtype == th.bool
        assert th.equal(states[0], r["before"])                    # states[0] is the last_state before the call
        assert r["c1"] == r["c0"] + H == (k + 1) * H               # rng_counter advanced by H
        rew = th.empty((H, N), device=DEV)
        term, trunc = th.empty((H, N), dtype=th.bool, device=DEV), th.empty((H, N), dtype=th.bool, device=DEV)
        for t in range(H):
            nxt = twin.step_into(actions[t].long(), rew[t], term[t], trunc[t])
            assert th.equal(nxt, states[t + 1] if t + 1 < H else r["last"]), (k, t)
        if rs != 1.0:
            rew *= rs                                              # the per-step path's `rewards *= reward_scale`
        assert th.equal(rewards, rew) and th.equal(undones, ~term) and th.equal(unmasks, ~trunc)
        state, sc, ep = r["env"]
        assert th.equal(state, twin.state) and th.equal(sc, twin.step_count) and th.equal(ep, twin.episode) and th.equal(r["last"], twin.state)
        n_term, n_trunc = n_term + int(term.sum()), n_trunc + int(trunc.sum())
    if rollouts["max_step"] == 7:
        assert n_trunc > 0                                         # truncation resets
    if N == 1000:
        assert n_term > 0 and n_trunc == 0                         # natural terminals


@pytest.mark.parametrize("N,net,H", [(50, (64, 32), 20), (600, (128, 128), 8)])
def test_philox_form(N, net, H):
    """uniform=None: the kernel's own draws are philox_uniform(seed, counter0 + t, env) -- the per-step path's stream"""
    agent, env, _ = make(N, net, 9, 0.5)
    agent.rng_counter = 1234567
    f32 = dict(dtype=th.float32, device=DEV)
    bufs = (th.empty((H, N, 4), **f32), th.empty((H, N), dtype=th.int32, device=DEV), th.empty((H, N), **f32), th.empty((H, N), **f32),
            th.empty((H, N), dtype=th.bool, device=DEV), th.empty((H, N), dtype=th.bool, device=DEV))
    last, uo = th.empty((N, 4), **f32), th.full((H, N), -1.0, **f32)
    env.fused_rollout_discrete(agent, H, None, bufs, last, uniform_out=uo)
    assert (uo >= 0).all() and (uo < 1).all() and 0.4 < float(uo.mean()) < 0.6 and len(th.unique(uo)) > 0.99 * H * N
    # a second agent / env pair given the recorded draws reproduces everything bit for bit
    agent2, env2, _ = make(N, net, 9, 0.5)
    items = agent2._explore_vec_env(env2, H, noise=uo)
    assert agent2.rollout_path == "one-launch"
    for a, b in zip(bufs, items):
        assert a.dtype == b.dtype and th.equal(a, b)
    assert th.equal(last, agent2.last_state) and th.equal(env.state, env2.state) and th.equal(env.episode, env2.episode)
    # the per-step kernel with the same seed and counter0 + t draws the same action outside the band
    agent3, _, _ = make(N, net, 9, 0.5)
    _, c = policy64(agent3, bufs[0])
    near = near_boundary(c, uo.reshape(-1).cpu().numpy()).reshape(H, N)
    assert near.mean() < 0.01
    for t in range(H):
        agent3.rng_counter = 1234567 + t
        act, lp = agent3.explore_action(bufs[0][t])
        ok = ~th.from_numpy(near[t]).to(DEV)
        assert th.equal(act[ok], bufs[1][t][ok]), t
        np.testing.assert_allclose(lp[ok].cpu().numpy(), bufs[2][t][ok].cpu().numpy(), rtol=1e-4, atol=1e-4)


def _spy(env):
    calls = []
    inner = env.fused_rollout_discrete
    env.fused_rollout_discrete = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    return calls


def test_routing():
    from elegantrl_amd.agents import AgentDiscreteA2C
    from elegantrl_amd.envs import CartPoleGpuVecEnv, CartPoleVecEnv
    H = 6
    for cls in (None, AgentDiscreteA2C):
        agent, env, _ = make(48, (64, 32), 500, cls=cls)
        calls = _spy(env)
        agent.explore_env(env, H)
        assert len(calls) == 1 and agent.rollout_path == "one-launch" and agent.rng_counter == H
        assert "one-launch rollout" in agent.kernel_path
        # the live-state handshake: nobody touched either side -> no copy back (a torch write would bump the version; the launch does
        # not); a last_state of the caller's -> the env takes it
        v = env.state._version
        agent.explore_env(env, H)
        assert env.state._version == v and len(calls) == 2
        agent.last_state = agent.last_state.clone()
        agent.explore_env(env, H)
        assert env.state._version == v + 1 and len(calls) == 3 and th.equal(agent.last_state, env.state)
    for kw, why in ((dict(fused=False), "fused_rollout is off"), (dict(net=(256, 128)), "outside"), (dict(net=(64, 64, 32)), "outside"),
                    (dict(other_n=32), "envs"), (dict(env_cls=CartPoleVecEnv), "has no")):
        other_n = kw.pop("other_n", None)
        agent, env, _ = make(48, kw.pop("net", (64, 32)), 500, **kw)
        if other_n:
            env = CartPoleGpuVecEnv(other_n, max_step=500, gpu_id=0, seed=5)
            env.reset()
        calls = _spy(env) if hasattr(env, "fused_rollout_discrete") else []
        assert why in agent._one_launch_reason(env, "fused_rollout_discrete"), (why, agent._one_launch_reason(env, "fused_rollout_discrete"))
        if other_n:
            with pytest.raises(RuntimeError):              # the loop runs, and an env of another size cannot fill the agent's rows
                agent.explore_env(env, H)
        else:
            items = agent.explore_env(env, H)
            assert items[1].dtype == th.int32 and items[4].dtype == th.bool and agent.rng_counter == H
        assert agent.rollout_path == "loop" and calls == []
        assert agent.evaluate_env(env) is None and why in agent._fused_eval_reason(env)


# ---- evaluation ---------------------------------------------------------------------------------------------------------------------------
EVAL_SEED = 9        # agent seed: every state the greedy policy visits has |z0 - z1| > 1e-3 (checked in the test; seeds 7 and 9 of 0..11 hold it), so no argmax is a near tie


def test_evaluation_matches_the_evaluator_loop(tmp_path, capsys):
    from elegantrl_amd.envs import CartPoleVecEnv
    from elegantrl_amd.train.evaluator import Evaluator, get_cumulative_rewards_and_step_from_vec_env
    N, max_step = 64, 40
    agent, env, args = make(N, (64, 32), max_step, agent_seed=EVAL_SEED)
    _, twin, _ = make(N, (64, 32), max_step, agent_seed=EVAL_SEED)
    # the loop's trajectory, step by step, and the condition on it: fp64 logits of every visited state are no near tie
    state, visited = twin.reset()[0], []
    with th.no_grad():
        for t in range(max_step):
            visited.append(state)
            state = twin.step(agent.act(state))[0]
    x = th.stack(visited).reshape(-1, 4).cpu().numpy().astype(np.float64)
    z = O.actor_mean(x, actor64(agent))
    gap = np.abs(z[:, 0] - z[:, 1]).min()
    print(f"smallest |z0 - z1| over {len(x)} visited states: {gap:.3e}")
    assert gap > 1e-3, gap
    with th.no_grad():
        loop = get_cumulative_rewards_and_step_from_vec_env(twin, agent.act)
    keep = dict(c=agent.rng_counter, last=agent.last_state, last_v=agent.last_state.clone(), flat=agent._flat.clone(),
                m1=agent._exp_avg.clone(), m2=agent._exp_avg_sq.clone(), step=agent._adam_step)
    rows = agent.evaluate_env(env)
    assert rows is not None and rows.dtype == th.float32 and rows.shape == loop.shape and rows.shape[0] >= N
    assert th.equal(rows, loop) and th.equal(rows[:, 0], rows[:, 1])          # return == length: the reward is 1 per step
    assert th.equal(env.state, twin.state) and th.equal(env.step_count, twin.step_count)
    assert agent.rng_counter == keep["c"] and agent.last_state is keep["last"] and th.equal(agent.last_state, keep["last_v"])
    assert th.equal(agent._flat, keep["flat"]) and th.equal(agent._exp_avg, keep["m1"]) and th.equal(agent._exp_avg_sq, keep["m2"])
    assert agent._adam_step == keep["step"]
    # Evaluator wiring
    args.cwd, args.eval_times = str(tmp_path), 3
    ev = Evaluator(args.cwd, env, args, agent=agent)
    rs = ev.get_cumulative_rewards_and_step(agent.act)
    assert ev.eval_path.startswith("fused evaluation") and th.equal(rs, rows)
    cenv = CartPoleVecEnv(N, max_step=max_step, gpu_id=0, seed=2)
    ev2 = Evaluator(args.cwd, cenv, args, agent=agent)
    ev2.get_cumulative_rewards_and_step(agent.act)
    assert ev2.eval_path.startswith("loop evaluation") and "CartPoleVecEnv" in ev2.eval_path


@pytest.mark.timeout(600)
def test_train_agent_learns_cartpole_on_the_one_launch_route(tmp_path, monkeypatch, capsys):
    """the hyper-parameters of test_train_agent_discrete_ppo_cartpole_learns on the device-resident env"""
    from elegantrl_amd import train_agent
    from elegantrl_amd.agents import AgentDiscretePPO
    from elegantrl_amd.envs import CartPoleGpuVecEnv
    from elegantrl_amd.train import Config
    calls = {"rollout": 0, "eval": 0}
    for name, key in (("fused_rollout_discrete", "rollout"), ("fused_evaluate_discrete", "eval")):
        inner = getattr(CartPoleGpuVecEnv, name)

        def spy(self, *a, _inner=inner, _key=key, **k):
            calls[_key] += 1
            return _inner(self, *a, **k)
        monkeypatch.setattr(CartPoleGpuVecEnv, name, spy)
    args = Config(AgentDiscretePPO, CartPoleGpuVecEnv, {"env_name": "CartPole-v1", "num_envs": 512, "max_step": 500, "state_dim": 4,
                                                        "action_dim": 2, "if_discrete": True})
    args.net_dims = [64, 32]
    args.fused_rollout = True          # the route is opt-in for the discrete agents until profiles/ holds its A/B record
    args.horizon_len, args.batch_size, args.repeat_times = 64, 4096, 4096 * 8 / 64
    args.gamma, args.learning_rate, args.lambda_entropy = 0.98, 2e-3, 0.01
    args.break_step, args.eval_per_step, args.eval_times = 64 * 40, 64 * 8, 8
    args.cwd, args.gpu_id, args.random_seed = str(tmp_path / "run"), 0, 0
    args.gae_algo = "exact"
    train_agent(args, if_single_process=True)
    rec = np.load(os.path.join(args.cwd, "recorder.npy"))
    assert np.isfinite(rec[:, :4]).all()
    assert rec[:, 1].max() > 150.0, f"discrete PPO did not learn CartPole: evaluated returns {np.round(rec[:, 1], 1).tolist()}"
    assert calls["rollout"] >= 40 and calls["eval"] >= 1, calls
    out = capsys.readouterr().out
    assert "| Evaluator: fused evaluation" in out and "loop evaluation" not in out
