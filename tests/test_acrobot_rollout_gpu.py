"""The one-launch discrete rollout and evaluation on Acrobot-v1 (csrc/rollout_discrete.hip: erl_rollout_discrete_acrobot_f32,
erl_eval_discrete_acrobot_f32) behind AgentDiscretePPO on AcrobotGpuVecEnv: 6 observations that are not the physical state, 3 actions,
a reward that is not constant.  Teacher-forced as tests/test_discrete_rollout_gpu.py: the policy rows are checked against an fp64
restatement ON the recorded states, the env rows against a twin env stepped by the per-step kernel WITH the recorded actions, so one
legitimate flip of a draw cannot make everything after it differ."""
import os

import numpy as np
import pytest
import torch as th

from oracle import ppo_numpy as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, A = 6, 3
BAND = 2e-6          # |u - CDF boundary| below which fp32 and fp64 may draw neighbouring actions (tests/test_discrete_rollout_gpu.py)
# (N, net, H, max_step, reward_scale, inject regime-B phys): ragged tile + truncation + reward scaling; a single full tile; many tiles;
# 257 tiles = two waves per workgroup and one row in the last tile; injected physical states, so that terminal rows occur
CASES = [(50, (64, 32), 40, 7, 0.25, False), (16, (32, 32), 9, 500, 1.0, False), (1000, (128, 64), 24, 500, 1.0, False),
         (4112, (32, 32), 8, 500, 1.0, False), (1000, (64, 32), 6, 500, 1.0, True)]


def regime_b(n, seed=21):
    """theta uniform in [-pi, pi], omega1 in U(-4, 4), omega2 in U(-8, 8): 14-19 % of such rows terminate within one step"""
    rng = np.random.default_rng(seed)
    p = np.stack((rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-4, 4, n), rng.uniform(-8, 8, n)), axis=1)
    return th.from_numpy(p.astype(np.float32)).to(DEV)


def inject(env, phys):
    env.phys.copy_(phys)
    env.state.copy_(env._observe(env.phys))
    env.state_epoch += 1


def make(N, net, max_step, reward_scale=1.0, env_seed=5, agent_seed=3, fused=True, cls=None, phys=None):
    from elegantrl_amd.agents import AgentDiscretePPO
    from elegantrl_amd.envs import AcrobotGpuVecEnv
    from elegantrl_amd.train import Config
    cls = cls or AgentDiscretePPO
    args = Config(cls, AcrobotGpuVecEnv, {"env_name": "Acrobot-v1", "num_envs": N, "max_step": max_step, "state_dim": S, "action_dim": A,
                                          "if_discrete": True})
    args.net_dims, args.reward_scale, args.random_seed, args.fused_rollout = list(net), reward_scale, 7, fused
    th.manual_seed(agent_seed)
    agent = cls(args.net_dims, S, A, gpu_id=0, args=args)
    with th.no_grad():
        g = th.Generator(device=DEV).manual_seed(agent_seed + 1)
        agent.act.state_avg[:] = 0.1 * th.randn(S, device=DEV, generator=g)
        agent.act.state_std[:] = 0.5 + th.rand(S, device=DEV, generator=g)
        agent.act.net[-1].weight.mul_(6.0)          # logits far from uniform: every branch of the draw (spread(), test_discrete_gpu.py)
    env = AcrobotGpuVecEnv(N, max_step=max_step, gpu_id=0, seed=env_seed)
    env.reset()
    if phys is not None:
        inject(env, phys)
    agent.last_state = env.state.clone()
    return agent, env, args


def actor64(agent):
    f = lambda t: t.detach().cpu().numpy().astype(np.float64)  # noqa: E731
    lin = [m for m in agent.act.net if isinstance(m, th.nn.Linear)]
    return O.Mlp([f(m.weight) for m in lin], [f(m.bias) for m in lin], f(agent.act.state_avg), f(agent.act.state_std), None)


def logits64(agent, states):
    return O.actor_mean(states.reshape(-1, S).cpu().numpy().astype(np.float64), actor64(agent))


def policy64(agent, states):
    """fp64 softmax probabilities and CDF of the agent's policy on states (..., 6)"""
    p = O.softmax(logits64(agent, states))
    return p, np.cumsum(p, axis=1)


def near_boundary(c, u):
    return (np.abs(c[:, :-1] - u.reshape(-1, 1).astype(np.float64)) < BAND).any(axis=1)       # (the last CDF entry is no boundary: u < 1)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"N{c[0]}-{c[1][0]}x{c[1][1]}-H{c[2]}" + ("-injected" if c[5] else ""))
def rollouts(request):
    """two consecutive one-launch rollouts with injected uniforms (env state, counters and rng_counter carry over), computed once"""
    N, net, H, max_step, rs, inj = request.param
    phys0 = regime_b(N) if inj else None
    agent, env, _ = make(N, net, max_step, rs, phys=phys0)
    g = th.Generator(device=DEV).manual_seed(N + H)
    out = []
    for k in range(2):
        u = th.rand((H, N), device=DEV, generator=g)
        before, c0 = agent.last_state.clone(), agent.rng_counter
        items = agent._explore_vec_env(env, H, noise=u)
        assert agent.rollout_path == "one-launch"
        out.append(dict(u=u, before=before, c0=c0, items=items, last=agent.last_state.clone(), c1=agent.rng_counter,
                        env=(env.phys.clone(), env.state.clone(), env.step_count.clone(), env.episode.clone())))
    return dict(agent=agent, N=N, H=H, max_step=max_step, rs=rs, phys0=phys0, out=out)


def test_policy_rows_against_fp64(rollouts):
    """band: 2e-6, as for the per-step kernel and the CartPole rollout; here a row has two CDF boundaries"""
    agent, N, H = rollouts["agent"], rollouts["N"], rollouts["H"]
    drawn = np.zeros(A, dtype=np.int64)
    for r in rollouts["out"]:
        states, actions, logprobs = r["items"][:3]
        assert actions.dtype == th.int32 and logprobs.dtype == th.float32 and states.dtype == th.float32
        assert states.shape == (H, N, S) and actions.shape == logprobs.shape == (H, N)
        p, c = policy64(agent, states)
        u = r["u"].reshape(-1).cpu().numpy()
        ref = np.minimum((c <= u[:, None].astype(np.float64)).sum(axis=1), A - 1)
        got = actions.reshape(-1).cpu().numpy()
        near = near_boundary(c, u)
        dev = np.abs(c[:, :-1] - u[:, None]).min(axis=1)[got != ref]
        print(f"cells {got.size}: {int((got != ref).sum())} differ from the fp64 draw, largest |u - CDF| among them {dev.max() if dev.size else 0:.3e}; "
              f"{int(near.sum())} within the band")
        assert got.min() >= 0 and got.max() <= A - 1
        np.testing.assert_array_equal(got[~near], ref[~near])
        assert (np.abs(got[near] - ref[near]) <= 1).all() and near.mean() < 0.01
        drawn += np.bincount(got, minlength=A)
        lp_ref = O.categorical_logits(p)[np.arange(got.size), got]
        np.testing.assert_allclose(logprobs.reshape(-1).cpu().numpy(), lp_ref, rtol=1e-4, atol=1e-4)
    print("draws per action:", drawn.tolist())
    assert (drawn > 0).all(), drawn          # all three actions are drawn


def test_env_rows_against_the_per_step_twin(rollouts):
    from elegantrl_amd.envs import AcrobotGpuVecEnv
    N, H, rs = rollouts["N"], rollouts["H"], rollouts["rs"]
    twin = AcrobotGpuVecEnv(N, max_step=rollouts["max_step"], gpu_id=0, seed=5)
    twin.reset()
    if rollouts["phys0"] is not None:
        inject(twin, rollouts["phys0"])
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
        assert th.equal(rew, th.where(term, 0.0, -1.0).to(th.float32))      # 0 on the terminal step, -1 otherwise
        if rs != 1.0:
            rew *= rs                                              # the per-step path's `rewards *= reward_scale`
        assert th.equal(rewards, rew) and th.equal(undones, ~term) and th.equal(unmasks, ~trunc)
        phys, state, sc, ep = r["env"]
        assert th.equal(phys, twin.phys) and th.equal(state, twin.state) and th.equal(sc, twin.step_count) and th.equal(ep, twin.episode)
        assert th.equal(r["last"], twin.state)
        n_term, n_trunc = n_term + int(term.sum()), n_trunc + int(trunc.sum())
    print(f"{n_term} terminal and {n_trunc} truncated cells")
    if rollouts["max_step"] == 7:
        assert n_trunc > 0                                         # truncation resets
    if rollouts["phys0"] is not None:
        assert n_term > 0 and n_trunc == 0                         # terminals, with the reward 0 and a reset behind them


@pytest.mark.parametrize("N,net,H", [(50, (64, 32), 20), (600, (128, 128), 8)])
def test_philox_form(N, net, H):
    """uniform=None: the kernel's own draws are philox_uniform(seed, counter0 + t, env) -- the per-step path's stream"""
    agent, env, _ = make(N, net, 9, 0.5)
    agent.rng_counter = 1234567
    f32 = dict(dtype=th.float32, device=DEV)
    bufs = (th.empty((H, N, S), **f32), th.empty((H, N), dtype=th.int32, device=DEV), th.empty((H, N), **f32), th.empty((H, N), **f32),
            th.empty((H, N), dtype=th.bool, device=DEV), th.empty((H, N), dtype=th.bool, device=DEV))
    last, uo = th.empty((N, S), **f32), th.full((H, N), -1.0, **f32)
    env.fused_rollout_discrete(agent, H, None, bufs, last, uniform_out=uo)
    assert (uo >= 0).all() and (uo < 1).all() and 0.4 < float(uo.mean()) < 0.6 and len(th.unique(uo)) > 0.99 * H * N
    # a second agent / env pair given the recorded draws reproduces everything bit for bit
    agent2, env2, _ = make(N, net, 9, 0.5)
    items = agent2._explore_vec_env(env2, H, noise=uo)
    assert agent2.rollout_path == "one-launch"
    for a, b in zip(bufs, items):
        assert a.dtype == b.dtype and th.equal(a, b)
    assert th.equal(last, agent2.last_state) and th.equal(env.state, env2.state) and th.equal(env.phys, env2.phys)
    assert th.equal(env.episode, env2.episode) and th.equal(env.step_count, env2.step_count)
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
    from elegantrl_amd.envs import AcrobotGpuVecEnv
    H = 6
    for cls in (None, AgentDiscreteA2C):
        agent, env, _ = make(48, (64, 32), 500, cls=cls)
        calls = _spy(env)
        agent.explore_env(env, H)
        assert len(calls) == 1 and agent.rollout_path == "one-launch" and agent.rng_counter == H
        assert "one-launch rollout" in agent.kernel_path and "AcrobotGpuVecEnv" in agent.kernel_path
        # the live-state handshake: nobody touched either side -> no copy back (a torch write would bump the version; the launch does
        # not); a last_state of the caller's -> the env takes it as the policy's input at t = 0, and phys is not disturbed by it
        v = env.state._version
        agent.explore_env(env, H)
        assert env.state._version == v and len(calls) == 2
        own = agent.last_state.clone()
        own[:, 4:] += 0.25                                         # NOT the observation of phys
        agent.last_state = own
        twin = AcrobotGpuVecEnv(48, max_step=500, gpu_id=0, seed=5)
        twin.phys.copy_(env.phys), twin.step_count.copy_(env.step_count), twin.episode.copy_(env.episode)
        items = agent.explore_env(env, H)
        assert env.state._version == v + 1 and len(calls) == 3 and th.equal(agent.last_state, env.state)
        assert th.equal(items[0][0], own)
        scratch = [th.empty(48, device=DEV), th.empty(48, dtype=th.bool, device=DEV), th.empty(48, dtype=th.bool, device=DEV)]
        for t in range(H):
            nxt = twin.step_into(items[1][t].long(), *scratch)
            assert th.equal(nxt, items[0][t + 1] if t + 1 < H else agent.last_state), t
        assert th.equal(twin.phys, env.phys)
    for kw, why in ((dict(fused=False), "fused_rollout is off"), (dict(net=(256, 128)), "outside"), (dict(net=(64, 64, 32)), "outside"),
                    (dict(other_n=32), "envs")):
        other_n = kw.pop("other_n", None)
        agent, env, _ = make(48, kw.pop("net", (64, 32)), 500, **kw)
        if other_n:
            env = AcrobotGpuVecEnv(other_n, max_step=500, gpu_id=0, seed=5)
            env.reset()
        calls = _spy(env)
        assert why in agent._one_launch_reason(env, "fused_rollout_discrete"), (why, agent._one_launch_reason(env, "fused_rollout_discrete"))
        if other_n:
            with pytest.raises(RuntimeError):              # the loop runs, and an env of another size cannot fill the agent's rows
                agent.explore_env(env, H)
        else:
            items = agent.explore_env(env, H)
            assert items[1].dtype == th.int32 and items[4].dtype == th.bool and agent.rng_counter == H and items[0].shape == (H, 48, S)
            assert int(items[1].min()) >= 0 and int(items[1].max()) <= A - 1
        assert agent.rollout_path == "loop" and calls == []
        assert agent.evaluate_env(env) is None and why in agent._fused_eval_reason(env)


# ---- evaluation ---------------------------------------------------------------------------------------------------------------------------
EVAL_SEED = 0        # agent seed: every state the greedy policy visits from reset has a top-two logit gap > 1e-3 in fp64 (checked in the test; seeds 0, 1, 2, 7
                     # and 10 of 0..11 hold it, seed 0 with 2.3e-2), so no argmax is a near tie
GAP = 1e-3


def top_two_gap(agent, visited):
    z = np.sort(logits64(agent, th.stack(visited)), axis=1)
    return float((z[:, -1] - z[:, -2]).min())


def test_evaluation_matches_the_evaluator_loop(tmp_path, capsys):
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
    gap = top_two_gap(agent, visited)
    print(f"smallest top-two logit gap over {N * max_step} visited states: {gap:.3e}")
    assert gap > GAP, gap
    with th.no_grad():
        loop = get_cumulative_rewards_and_step_from_vec_env(twin, agent.act)
    keep = dict(c=agent.rng_counter, last=agent.last_state, last_v=agent.last_state.clone(), flat=agent._flat.clone(),
                m1=agent._exp_avg.clone(), m2=agent._exp_avg_sq.clone(), step=agent._adam_step)
    rows = agent.evaluate_env(env)
    assert rows is not None and rows.dtype == th.float32 and rows.shape == loop.shape and rows.shape[0] >= N
    assert th.equal(rows, loop)
    assert th.equal(env.state, twin.state) and th.equal(env.phys, twin.phys) and th.equal(env.step_count, twin.step_count)
    # -1 per step and 0 on the terminal step: a truncated episode returns -length, a terminated one -(length - 1)
    ret, length = rows[:, 0], rows[:, 1]
    assert (((ret == -length) & (length == max_step)) | ((ret == -(length - 1)) & (length <= max_step))).all()
    assert agent.rng_counter == keep["c"] and agent.last_state is keep["last"] and th.equal(agent.last_state, keep["last_v"])
    assert th.equal(agent._flat, keep["flat"]) and th.equal(agent._exp_avg, keep["m1"]) and th.equal(agent._exp_avg_sq, keep["m2"])
    assert agent._adam_step == keep["step"]
    # Evaluator wiring
    args.cwd, args.eval_times = str(tmp_path), 3
    ev = Evaluator(args.cwd, env, args, agent=agent)
    rs = ev.get_cumulative_rewards_and_step(agent.act)
    assert ev.eval_path.startswith("fused evaluation") and th.equal(rs, rows)


# ---- the fused update at this shape ---------------------------------------------------------------------------------------------------------
def test_fused_update_step_gradients_at_acrobot_shape():
    """erl_ppo_step_discrete_f32 at (S 6, net (64, 32), A 3), B = 100 against the fp64 oracle, at the tolerances of
    tests/test_discrete_update_gpu.py (which has no case at this shape)"""
    from elegantrl_amd import ops
    from tests.test_discrete_gpu import discrete_case, spread
    from tests.test_discrete_update_gpu import H, N, check_against_oracle, oracle_step, run_step
    from tests.test_mlpn_gpu import random_net_n
    hidden, B = (64, 32), 100
    rng = np.random.default_rng(S + B + A)
    case = discrete_case(rng, H, N, S, A, B)
    actor, critic = spread(random_net_n(rng, [S, *hidden, A], False), 3.0), random_net_n(rng, [S, *hidden, 1], False)
    Pa, Pc = ops.MlpSpecN([S, *hidden, A], False).count, ops.MlpSpecN([S, *hidden, 1], False).count
    got, slabs = run_step(ops, actor, critic, case, S, hidden, A)
    check_against_oracle(got, slabs, oracle_step(actor, critic, case), Pa, Pc)


# ---- learning -------------------------------------------------------------------------------------------------------------------------------
LEARN = dict(num_envs=512, horizon_len=128, batch_size=4096, updates=16, gamma=0.99, learning_rate=2e-3, lambda_entropy=0.01,
             reward_scale=0.1, iterations=40, eval_every=5, eval_times=8, net_dims=[64, 32], seed=0)


def learning_args(cwd, hp=LEARN):
    from elegantrl_amd.agents import AgentDiscretePPO
    from elegantrl_amd.envs import AcrobotGpuVecEnv
    from elegantrl_amd.train import Config
    H = hp["horizon_len"]
    args = Config(AgentDiscretePPO, AcrobotGpuVecEnv, {"env_name": "Acrobot-v1", "num_envs": hp["num_envs"], "max_step": 500, "state_dim": S,
                                                       "action_dim": A, "if_discrete": True})
    args.net_dims = list(hp["net_dims"])
    args.fused_rollout = True          # the route is opt-in for the discrete agents
    args.fused_update = True
    args.horizon_len, args.batch_size, args.repeat_times = H, hp["batch_size"], hp["batch_size"] * hp["updates"] / H
    args.gamma, args.learning_rate, args.lambda_entropy, args.reward_scale = hp["gamma"], hp["learning_rate"], hp["lambda_entropy"], hp["reward_scale"]
    args.break_step, args.eval_per_step, args.eval_times = H * hp["iterations"], H * hp["eval_every"], hp["eval_times"]
    args.cwd, args.gpu_id, args.random_seed = str(cwd), 0, hp["seed"]
    args.gae_algo = "exact"
    return args


@pytest.mark.timeout(600)
def test_train_agent_learns_acrobot_on_the_one_launch_route(tmp_path, monkeypatch, capsys):
    """a policy that never reaches the bar scores exactly -500 and random play is there (1.4 % of random-policy episodes terminate within
    500 steps); the bar is the best evaluated mean return >= -max_step / 2 = -250.  The settings and the curve of the recorded run are in
    profiles/acrobot_learning.txt."""
    from elegantrl_amd import train_agent
    from elegantrl_amd.envs import AcrobotGpuVecEnv
    calls = {"rollout": 0, "eval": 0}
    for name, key in (("fused_rollout_discrete", "rollout"), ("fused_evaluate_discrete", "eval")):
        inner = getattr(AcrobotGpuVecEnv, name)

        def spy(self, *a, _inner=inner, _key=key, **k):
            calls[_key] += 1
            return _inner(self, *a, **k)
        monkeypatch.setattr(AcrobotGpuVecEnv, name, spy)
    args = learning_args(tmp_path / "run")
    train_agent(args, if_single_process=True)
    rec = np.load(os.path.join(args.cwd, "recorder.npy"))
    print("evaluated mean returns:", np.round(rec[:, 1], 1).tolist())
    assert np.isfinite(rec[:, :4]).all()
    assert rec[:, 1].max() >= -500 / 2, f"discrete PPO did not learn Acrobot: evaluated returns {np.round(rec[:, 1], 1).tolist()}"
    assert calls["rollout"] >= LEARN["iterations"] and calls["eval"] >= 1, calls
    out = capsys.readouterr().out
    assert "| Evaluator: fused evaluation" in out and "loop evaluation" not in out
