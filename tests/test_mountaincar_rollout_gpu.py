"""The one-launch discrete rollout, its GAE form and the evaluation form on MountainCar-v0 (csrc/rollout_discrete.hip:
erl_rollout_discrete_mountaincar_f32, erl_rollout_discrete_mountaincar_gae_f32, erl_eval_discrete_mountaincar_f32) behind
AgentDiscretePPO on MountainCarGpuVecEnv, and the fused minibatch step at (S, A) = (2, 3): the first shape that drives these kernels
below four observations (elements 2 and 3 of layer 1's operand tile are zero operands, not features).

"Against the loop" means what it means in tests/test_discrete_rollout_gpu.py and tests/test_acrobot_rollout_gpu.py: teacher-forced.  The
per-step loop's policy kernel (erl_mlpn_rollout_step_discrete_f32: GEMM tiles, erf GELU) and the rollout's register chain are two
fp32 evaluations of the same network, so their logits agree to rounding and not to the bit, and one flipped draw would make every later
row differ.  So the env planes (states, rewards, undones, unmasks), the last state, the counters and the env's live state are compared
bit for bit with a twin env stepped by the per-step kernel WITH the recorded actions, the actions with the per-step policy kernel on the
recorded states and uniforms outside the 2e-6 band, and logits / actions / log-probs with an fp64 restatement ON the recorded states.
There is no learning test: a random policy never reaches the goal, so PPO from scratch sees a constant reward."""
import math

import numpy as np
import pytest
import torch as th

from oracle import ppo_numpy as O
from tests import mountaincar_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, A = 2, 3
BAND = 2e-6          # |u - CDF boundary| below which fp32 and fp64 may draw neighbouring actions (tests/test_acrobot_rollout_gpu.py)
GOAL_ROW = (0.45, 0.05)          # terminal at step 1 under action 2, at step 2 under actions 0 and 1 (tests/test_mountaincar_env_gpu.py)
# (N, net, H, max_step, reward_scale, rows injected at GOAL_ROW): a partial 16-env tile; the largest LDS image on 38 tiles; truncation
# and restart inside the launch, with reward scaling; terminals inside the launch
CASES = [(50, (64, 32), 20, 200, 1.0, False), (600, (128, 128), 8, 200, 1.0, False), (50, (64, 32), 20, 7, 0.25, False),
         (600, (128, 128), 8, 200, 1.0, True)]


def inject(env, row=GOAL_ROW):
    env.state[:] = th.tensor(row, dtype=th.float32, device=DEV)
    env.state_epoch += 1


def make(N, net, max_step, reward_scale=1.0, env_seed=5, agent_seed=3, fused=True, cls=None, goal=False, **extra):
    from elegantrl_amd.agents import AgentDiscretePPO
    from elegantrl_amd.envs import MountainCarGpuVecEnv
    from elegantrl_amd.train import Config
    cls = cls or AgentDiscretePPO
    args = Config(cls, MountainCarGpuVecEnv, {"env_name": "MountainCar-v0", "num_envs": N, "max_step": max_step, "state_dim": S,
                                              "action_dim": A, "if_discrete": True})
    args.net_dims, args.reward_scale, args.random_seed, args.fused_rollout, args.quiet = list(net), reward_scale, 7, fused, True
    for k, v in extra.items():
        setattr(args, k, v)
    th.manual_seed(agent_seed)
    agent = cls(args.net_dims, S, A, gpu_id=0, args=args)
    with th.no_grad():
        g = th.Generator(device=DEV).manual_seed(agent_seed + 1)
        centre, width = th.tensor([-0.5, 0.0], device=DEV), th.tensor([0.3, 0.03], device=DEV)          # where the car lives
        agent.act.state_avg[:] = centre + 0.1 * width * th.randn(S, device=DEV, generator=g)
        agent.act.state_std[:] = width * (0.5 + th.rand(S, device=DEV, generator=g))
        agent.act.net[-1].weight.mul_(6.0)          # logits far from uniform: every branch of the draw (spread(), test_discrete_gpu.py)
        # the critic's own normalisation, not the actor's; a last layer that takes |values| to order 1
        agent.cri.state_avg[:] = centre + 0.1 * width * th.randn(S, device=DEV, generator=g)
        agent.cri.state_std[:] = width * (0.5 + th.rand(S, device=DEV, generator=g))
        agent.cri.net[-1].weight.mul_(8.0)
        agent.cri.net[-1].bias.fill_(0.5)
    env = MountainCarGpuVecEnv(N, max_step=max_step, gpu_id=0, seed=env_seed)
    env.reset()
    if goal:
        inject(env)
    agent.last_state = env.state.clone()
    return agent, env, args


def net64(net, with_norm):
    f = lambda t: t.detach().cpu().numpy().astype(np.float64)  # noqa: E731
    lin = [m for m in net.net if isinstance(m, th.nn.Linear)]
    return O.Mlp([f(m.weight) for m in lin], [f(m.bias) for m in lin], f(with_norm.state_avg), f(with_norm.state_std), None)


def logits64(agent, states):
    return O.actor_mean(states.reshape(-1, S).cpu().numpy().astype(np.float64), net64(agent.act, agent.act))


def policy64(agent, states):
    """fp64 softmax probabilities and CDF of the agent's policy on states (..., 2)"""
    p = O.softmax(logits64(agent, states))
    return p, np.cumsum(p, axis=1)


def near_boundary(c, u):
    return (np.abs(c[:, :-1] - u.reshape(-1, 1).astype(np.float64)) < BAND).any(axis=1)       # (the last CDF entry is no boundary: u < 1)


def case_id(c):
    return f"N{c[0]}-{c[1][0]}x{c[1][1]}-H{c[2]}-ms{c[3]}" + ("-goal" if c[5] else "")


@pytest.fixture(scope="module", params=CASES, ids=case_id)
def rollouts(request):
    """two consecutive one-launch rollouts with injected uniforms (env state, counters and rng_counter carry over), computed once"""
    N, net, H, max_step, rs, goal = request.param
    agent, env, _ = make(N, net, max_step, rs, goal=goal)
    g = th.Generator(device=DEV).manual_seed(N + H)
    out = []
    for k in range(2):
        u = th.rand((H, N), device=DEV, generator=g)
        before, c0 = agent.last_state.clone(), agent.rng_counter
        items = agent._explore_vec_env(env, H, noise=u)
        assert agent.rollout_path == "one-launch"
        out.append(dict(u=u, before=before, c0=c0, items=items, last=agent.last_state.clone(), c1=agent.rng_counter,
                        env=(env.state.clone(), env.step_count.clone(), env.episode.clone())))
    return dict(agent=agent, N=N, H=H, max_step=max_step, rs=rs, goal=goal, out=out)


def test_policy_rows_against_fp64(rollouts):
    """band and tolerances: those of tests/test_acrobot_rollout_gpu.py for the same quantities (a row has two CDF boundaries); the logits
    themselves are held to fp64 through the log-probs, which are log-softmax of them at the drawn action"""
    agent, N, H = rollouts["agent"], rollouts["N"], rollouts["H"]
    drawn = np.zeros(A, dtype=np.int64)
    for r in rollouts["out"]:
        states, actions, logprobs = r["items"][:3]
        assert actions.dtype == th.int32 and logprobs.dtype == th.float32 and states.dtype == th.float32
        assert states.shape == (H, N, S) and actions.shape == logprobs.shape == (H, N)
        assert np.isfinite(logprobs.cpu().numpy()).all()
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
    if not rollouts["goal"]:
        assert (drawn > 0).all(), drawn          # all three actions are drawn


def test_planes_against_the_per_step_loop(rollouts):
    """bit for bit: the four env planes, the last state, the counters and the env's live state against the per-step kernel fed the
    recorded actions; the action plane against the per-step policy kernel on the recorded states and uniforms (outside the band), the
    log-prob plane within that kernel's own tolerance"""
    from elegantrl_amd.envs import MountainCarGpuVecEnv
    agent, N, H, rs = rollouts["agent"], rollouts["N"], rollouts["H"], rollouts["rs"]
    twin = MountainCarGpuVecEnv(N, max_step=rollouts["max_step"], gpu_id=0, seed=5)
    twin.reset()
    if rollouts["goal"]:
        inject(twin)
    n_term = n_trunc = 0
    keep_counter = agent.rng_counter
    for k, r in enumerate(rollouts["out"]):
        states, actions, logprobs, rewards, undones, unmasks = r["items"]
        assert rewards.dtype == th.float32 and undones.dtype == th.bool and unmasks.dtype == th.bool
        assert th.equal(states[0], r["before"])                    # states[0] is the last_state before the call
        assert r["c1"] == r["c0"] + H == (k + 1) * H               # rng_counter advanced by H
        rew = th.empty((H, N), device=DEV)
        term, trunc = th.empty((H, N), dtype=th.bool, device=DEV), th.empty((H, N), dtype=th.bool, device=DEV)
        _, c = policy64(agent, states)
        near = near_boundary(c, r["u"].reshape(-1).cpu().numpy()).reshape(H, N)
        for t in range(H):
            act, lp = agent.explore_action(states[t], uniform=r["u"][t].contiguous())          # the loop's policy kernel
            ok = ~th.from_numpy(near[t]).to(DEV)
            assert th.equal(act[ok], actions[t][ok]), (k, t)
            np.testing.assert_allclose(lp[ok].cpu().numpy(), logprobs[t][ok].cpu().numpy(), rtol=1e-4, atol=1e-4)
            nxt = twin.step_into(actions[t].long(), rew[t], term[t], trunc[t])                  # the loop's env kernel
            assert th.equal(nxt, states[t + 1] if t + 1 < H else r["last"]), (k, t)
        assert (rew == -1).all()                                   # -1 on every step, the terminal one included
        if rs != 1.0:
            rew *= rs                                              # the per-step path's `rewards *= reward_scale`
        assert th.equal(rewards, rew) and th.equal(undones, ~term) and th.equal(unmasks, ~trunc)
        state, sc, ep = r["env"]
        assert th.equal(state, twin.state) and th.equal(sc, twin.step_count) and th.equal(ep, twin.episode)
        assert th.equal(r["last"], twin.state)
        n_term, n_trunc = n_term + int(term.sum()), n_trunc + int(trunc.sum())
    agent.rng_counter = keep_counter
    print(f"{n_term} terminal and {n_trunc} truncated cells")
    if rollouts["max_step"] == 7:
        assert n_trunc >= 4 * N                                    # truncation and restart inside the launch: 40 steps, every 7th
    if rollouts["goal"]:
        assert n_term >= N and n_trunc == 0                        # every injected row reaches the goal within two steps, and restarts
    else:
        assert n_term == 0


@pytest.mark.parametrize("N,net,H", [(50, (64, 32), 20), (600, (128, 128), 8)])
def test_philox_form(N, net, H):
    """uniform=None: the kernel's own draws are philox_uniform(seed, counter0 + t, env) -- the per-step path's stream.  max_step 7:
    truncation and restart inside the launch"""
    agent, env, _ = make(N, net, 7, 0.5)
    agent.rng_counter = 1234567
    f32 = dict(dtype=th.float32, device=DEV)
    bufs = (th.empty((H, N, S), **f32), th.empty((H, N), dtype=th.int32, device=DEV), th.empty((H, N), **f32), th.empty((H, N), **f32),
            th.empty((H, N), dtype=th.bool, device=DEV), th.empty((H, N), dtype=th.bool, device=DEV))
    last, uo = th.empty((N, S), **f32), th.full((H, N), -1.0, **f32)
    env.fused_rollout_discrete(agent, H, None, bufs, last, uniform_out=uo)
    assert (uo >= 0).all() and (uo < 1).all() and 0.4 < float(uo.mean()) < 0.6 and len(th.unique(uo)) > 0.99 * H * N
    assert (~bufs[5]).sum() == N * (H // 7)
    # a second agent / env pair given the recorded draws reproduces everything bit for bit
    agent2, env2, _ = make(N, net, 7, 0.5)
    items = agent2._explore_vec_env(env2, H, noise=uo)
    assert agent2.rollout_path == "one-launch"
    for a, b in zip(bufs, items):
        assert a.dtype == b.dtype and th.equal(a, b)
    assert th.equal(last, agent2.last_state) and th.equal(env.state, env2.state)
    assert th.equal(env.episode, env2.episode) and th.equal(env.step_count, env2.step_count)
    # the per-step kernel with the same seed and counter0 + t draws the same action outside the band; the env rows are the twin's
    agent3, twin, _ = make(N, net, 7, 0.5)
    _, c = policy64(agent3, bufs[0])
    near = near_boundary(c, uo.reshape(-1).cpu().numpy()).reshape(H, N)
    assert near.mean() < 0.01
    scratch = [th.empty(N, device=DEV), th.empty(N, dtype=th.bool, device=DEV), th.empty(N, dtype=th.bool, device=DEV)]
    for t in range(H):
        agent3.rng_counter = 1234567 + t
        act, lp = agent3.explore_action(bufs[0][t])
        ok = ~th.from_numpy(near[t]).to(DEV)
        assert th.equal(act[ok], bufs[1][t][ok]), t
        np.testing.assert_allclose(lp[ok].cpu().numpy(), bufs[2][t][ok].cpu().numpy(), rtol=1e-4, atol=1e-4)
        nxt = twin.step_into(bufs[1][t].long(), *scratch)
        assert th.equal(nxt, bufs[0][t + 1] if t + 1 < H else last), t
        assert th.equal(scratch[0] * 0.5, bufs[3][t]) and th.equal(~scratch[1], bufs[4][t]) and th.equal(~scratch[2], bufs[5][t])
    assert th.equal(twin.state, env.state) and th.equal(twin.step_count, env.step_count) and th.equal(twin.episode, env.episode)


# ---- the GAE form: the contract of tests/test_discrete_rollout_gae_gpu.py at S = 2 -------------------------------------------------------
GAE_CASES = [(50, (64, 32), 20, 7, 0.25, True), (50, (64, 32), 20, 7, 0.25, False), (600, (128, 128), 8, 200, 1.0, True)]


@pytest.fixture(scope="module", params=GAE_CASES, ids=lambda c: f"N{c[0]}-{c[1][0]}x{c[1][1]}-H{c[2]}-{'vtrace' if c[5] else 'plain'}")
def gae_runs(request):
    """two consecutive rollouts with injected uniforms, with the epilogue (`on`) and without (`off`), computed once"""
    N, net, H, max_step, rs, vtrace = request.param
    g = th.Generator(device=DEV).manual_seed(N + H)
    uniforms = [th.rand((H, N), device=DEV, generator=g) for _ in range(2)]
    res = {}
    for key, fused_gae in (("on", True), ("off", False)):
        agent, env, _ = make(N, net, max_step, rs, fused_gae=fused_gae, if_use_v_trace=vtrace)
        out = []
        for u in uniforms:
            items = agent._explore_vec_env(env, H, noise=u)
            assert agent.rollout_path == "one-launch"
            out.append(dict(items=items, last=agent.last_state, env=(env.state.clone(), env.step_count.clone(), env.episode.clone()),
                            cache=agent._rollout_cache, kept=(items[3].clone(), items[4].clone())))
        res[key] = out
        res.setdefault("agent", agent)
    return dict(res, N=N, H=H, max_step=max_step, vtrace=vtrace)


def test_gae_form_leaves_the_rollout_unchanged(gae_runs):
    for a, b in zip(gae_runs["on"], gae_runs["off"]):
        assert b["cache"] is None or "adv" not in b["cache"]
        assert a["cache"] is not None and "adv" in a["cache"]
        for x, y in zip(a["items"], b["items"]):
            assert x.dtype == y.dtype and th.equal(x, y)
        assert th.equal(a["last"], b["last"])
        for x, y in zip(a["env"], b["env"]):
            assert th.equal(x, y)


def test_gae_form_values_against_fp64(gae_runs):
    """tolerance: the layered value pass's (tests/test_mlpn_gpu.py::test_mlpn_value_forward), as tests/test_discrete_rollout_gae_gpu.py"""
    agent, N, H = gae_runs["agent"], gae_runs["N"], gae_runs["H"]
    critic = net64(agent.cri, agent.cri)
    top = 0.0
    for r in gae_runs["on"]:
        c = r["cache"]
        assert c["values"].shape == (H, N) and c["next_value"].shape == (N,) and c["values"].dtype == th.float32
        ref = O.critic_value(r["items"][0].cpu().numpy().astype(np.float64), critic)
        ref_next = O.critic_value(r["last"].cpu().numpy().astype(np.float64), critic)
        got, got_next = c["values"].cpu().numpy(), c["next_value"].cpu().numpy()
        print(f"values: max |err| {np.abs(got - ref).max():.3e} (next: {np.abs(got_next - ref_next).max():.3e}), max |value| {np.abs(ref).max():.3f}")
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(got_next, ref_next, rtol=1e-4, atol=2e-5)
        top = max(top, float(np.abs(ref).max()))
    assert top > 0.3                                                    # the comparison is not one of zeros


def test_gae_form_is_the_exact_scan_on_its_own_values(gae_runs):
    from elegantrl_amd import ops
    agent, N, H, vtrace = gae_runs["agent"], gae_runs["N"], gae_runs["H"], gae_runs["vtrace"]
    n_trunc = 0
    for r in gae_runs["on"]:
        states, actions, logprobs, rewards, undones, unmasks = r["items"]
        c = r["cache"]
        stats = th.zeros(8, dtype=th.float64, device=DEV)
        adv, ret = ops.gae_scan(rewards.clone(), undones.clone(), unmasks, c["values"], c["next_value"], float(agent.gamma),
                                float(agent.lambda_gae_adv), use_v_trace=vtrace, mutate=True, algo="exact", stats=stats)
        assert th.equal(c["adv"], adv), f"advantages differ in {(c['adv'] != adv).sum().item()} elements"
        assert th.equal(c["ret"], ret)
        assert th.equal(rewards, r["kept"][0]) and th.equal(undones, r["kept"][1])       # explore_env's outputs are not mutated
        assert c["n_parts"] == math.ceil(N / 16) and c["parts"].numel() == 3 * c["n_parts"]
        folded = ops.adv_stats_fold(c["parts"], c["n_parts"], H, N, th.full((8,), -1.0, dtype=th.float64, device=DEV))
        np.testing.assert_allclose(folded.cpu().numpy()[:5], stats.cpu().numpy()[:5], rtol=1e-12, atol=1e-9)
        assert folded[5:].abs().sum().item() == 0
        n_trunc += int((~unmasks).sum())
    if gae_runs["max_step"] < H:
        assert n_trunc > 0


# ---- evaluation ---------------------------------------------------------------------------------------------------------------------------
GAP = 5e-5           # smallest fp64 top-two logit gap the visited states may show (at rest the gap is the bias itself, 1e-4, in any arithmetic)


def set_sign_policy(agent):
    """the actor's weights by hand: greedy action 2 while the velocity is not negative, else 0.  With a = 10 v / (0.01 + 1e-4):
    layer 1 holds gelu(a) and gelu(-a), layer 2 gelu(4 .) of each, logit 2 = 10 * the first + 1e-4, logit 0 = 10 * the second, logit 1 =
    -10; gelu(x) > 0 >= gelu(-x) for x > 0, so the sign of the velocity decides, and the bias on logit 2 decides at rest, where every
    hidden unit is exactly 0"""
    lin = [m for m in agent.act.net if isinstance(m, th.nn.Linear)]
    with th.no_grad():
        for m in lin:
            m.weight.zero_()
            m.bias.zero_()
        agent.act.state_avg.zero_()
        agent.act.state_std[:] = th.tensor([1.0, 0.01], device=DEV)
        lin[0].weight[0, 1], lin[0].weight[1, 1] = 10.0, -10.0
        lin[1].weight[0, 0], lin[1].weight[1, 1] = 4.0, 4.0
        lin[2].weight[2, 0], lin[2].weight[0, 1] = 10.0, 10.0
        lin[2].bias[1], lin[2].bias[2] = -10.0, 1e-4


def test_evaluation_matches_the_evaluator_loop(tmp_path):
    from elegantrl_amd.train.evaluator import Evaluator
    N, max_step = 64, 200
    agent, env, args = make(N, (64, 32), max_step)
    _, twin, _ = make(N, (64, 32), max_step)
    set_sign_policy(agent)
    # the condition, on the fp64 restatement alone: the network's greedy action IS the sign policy on every state it visits, no argmax
    # is a near tie, and every first episode ends at the goal before max_step
    state = twin.reset()[0].cpu().numpy().astype(np.float64)
    first, gap = np.zeros(N, dtype=np.int64), np.inf
    for t in range(1, max_step + 1):
        z = logits64(agent, th.from_numpy(state))
        act = z.argmax(axis=1)
        np.testing.assert_array_equal(act, R.sign_policy(state))
        zs = np.sort(z, axis=1)
        gap = min(gap, float((zs[:, -1] - zs[:, -2]).min()))
        state, term, _ = R.mountaincar_step(state, act)
        first[(first == 0) & term] = t
        if (first > 0).all():
            break
    print(f"fp64: first episodes end after {first.min()}..{first.max()} steps; smallest top-two logit gap on the way {gap:.3e}")
    assert (first > 0).all() and first.max() < max_step, "the hand-set policy does not end every episode before max_step in fp64"
    assert gap > GAP, gap
    # the Evaluator by two launches against the Evaluator's per-step loop
    args.cwd, args.eval_times = str(tmp_path), 3
    keep = dict(c=agent.rng_counter, last=agent.last_state, last_v=agent.last_state.clone())
    fused = Evaluator(args.cwd, env, args, agent=agent)
    rows = fused.get_cumulative_rewards_and_step(agent.act)
    assert fused.eval_path.startswith("fused evaluation")
    loop_ev = Evaluator(args.cwd, twin, args)
    with th.no_grad():
        loop = loop_ev.get_cumulative_rewards_and_step(agent.act)
    assert loop_ev.eval_path.startswith("loop evaluation")
    assert rows.dtype == th.float32 and rows.shape == loop.shape and rows.shape[0] >= N
    assert th.equal(rows, loop)
    ret, length = rows[:, 0], rows[:, 1]
    assert (ret == -length).all() and (length < max_step).all()                       # -1 per step, the terminal one included; none truncated
    assert rows.shape[0] == N and int(length.min()) >= first.min() - 1 and int(length.max()) <= first.max() + 1          # one episode each
    assert th.equal(env.state, twin.state) and th.equal(env.step_count, twin.step_count) and th.equal(env.episode, twin.episode)
    assert agent.rng_counter == keep["c"] and agent.last_state is keep["last"] and th.equal(agent.last_state, keep["last_v"])


# ---- the fused update at this shape ---------------------------------------------------------------------------------------------------------
def test_fused_update_step_gradients_at_mountaincar_shape():
    """erl_ppo_step_discrete_f32 at (S 2, net (64, 32), A 3), B = 100 against the fp64 oracle, at the tolerances of
    tests/test_discrete_update_gpu.py (which has no case below S = 4), as test_fused_update_step_gradients_at_acrobot_shape at (6, 3)"""
    from elegantrl_amd import ops
    from tests.test_discrete_gpu import discrete_case, spread
    from tests.test_discrete_update_gpu import H, N, check_against_oracle, oracle_step, run_step
    from tests.test_mlpn_gpu import random_net_n
    hidden, B = (64, 32), 100
    assert ops.ppo_discrete_supported(S, *hidden, A)
    rng = np.random.default_rng(S + B + A)
    case = discrete_case(rng, H, N, S, A, B)
    actor, critic = spread(random_net_n(rng, [S, *hidden, A], False), 3.0), random_net_n(rng, [S, *hidden, 1], False)
    Pa, Pc = ops.MlpSpecN([S, *hidden, A], False).count, ops.MlpSpecN([S, *hidden, 1], False).count
    got, slabs = run_step(ops, actor, critic, case, S, hidden, A)
    check_against_oracle(got, slabs, oracle_step(actor, critic, case), Pa, Pc)


# ---- routing --------------------------------------------------------------------------------------------------------------------------------
def _spy(env):
    calls = []
    inner = env.fused_rollout_discrete
    env.fused_rollout_discrete = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    return calls


def test_routing():
    H = 6
    agent, env, _ = make(48, (64, 32), 200)
    calls = _spy(env)
    items = agent.explore_env(env, H)
    assert len(calls) == 1 and agent.rollout_path == "one-launch" and agent.rng_counter == H
    assert "one-launch rollout" in agent.kernel_path and "MountainCarGpuVecEnv" in agent.kernel_path
    assert agent._one_launch_reason(env, "fused_rollout_discrete") is None and agent._fused_eval_reason(env) is None
    assert items[0].shape == (H, 48, S) and th.equal(agent.last_state, env.state)
    # without args.fused_rollout the loop runs, on the same env class
    agent, env, _ = make(48, (64, 32), 200, fused=False)
    calls = _spy(env)
    assert "fused_rollout is off" in agent._one_launch_reason(env, "fused_rollout_discrete")
    items = agent.explore_env(env, H)
    assert agent.rollout_path == "loop" and calls == [] and agent.rng_counter == H
    assert "per-step rollout loop" in agent.kernel_path
    assert items[1].dtype == th.int32 and items[4].dtype == th.bool and items[0].shape == (H, 48, S)
    assert int(items[1].min()) >= 0 and int(items[1].max()) <= A - 1 and (items[3] == -1).all()
    assert agent.evaluate_env(env) is None and "fused_rollout is off" in agent._fused_eval_reason(env)
