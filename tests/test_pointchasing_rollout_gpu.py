"""The one-launch rollouts and evaluations on PointChasingVecEnv (erl_rollout_pointchasing_f32, erl_eval_pointchasing_f32,
erl_sac_rollout_[mod_]pointchasing_f32, erl_sac_eval_[mod_]pointchasing_f32), mirroring the Pendulum cases of tests/test_rollout_fused_gpu.py,
tests/test_sac.py, tests/test_modsac_rollout_gpu.py and tests/test_eval_fused_gpu.py:
  1. one launch against the per-step loop on the rollout's own per-step kernels, bit for bit -- the six buffers, last state, live state,
     `distance` and counters -- with resets inside the launch (max_step 5 < H 12), a full and a one-env tile behind the first (N = 33), and
     the epilogue's advantages against erl_gae_scan_f32(EXACT) on the same rows (the flags are no longer constant, as they are for
     Pendulum), fed from LDS (H = 12) and read back from the buffers (H = 130).
     The critic's `values` and `next_value` have no per-step kernel of the same arithmetic: the per-step side's values are update_net's
     pre-pass (agent.get_values), which sums in another order, so against it they agree to rtol = atol = 2e-5 only (the Pendulum twin's
     bound: a few fp32 ulp of sums of 32..128 products of O(1) values).  Their bit-exact pin is the launch against itself: one launch of
     H steps against H launches of one step each from the same state -- there the critic's input of step t comes from the kernel's
     prologue (global state -> normalised tile) where the long launch takes it from the tile the env step wrote, and the bootstrap pass
     of launch t is the regular pass of launch t + 1;
  2. the evaluation form against the training form under zero noise, bit for bit;
  3. agent.evaluate_env against the Evaluator's loop, to the tolerances of the Pendulum twins;
  4. the reset draw does not depend on the kernel that makes it;
  5. train_agent end to end (finite logs, files written: no learning claim)."""
import os

import numpy as np
import pytest
import torch as th

from tests.eval_helpers import oracle_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, MAX_STEP = 12, 5


def _agent_class(kind):
    from elegantrl_amd.agents import AgentModSAC, AgentPPO, AgentSAC
    return {"ppo": AgentPPO, "sac": AgentSAC, "modsac": AgentModSAC}[kind]


def _make(kind, N, dim, net, max_step=MAX_STEP, scale=1.0, fused=True, seed=5, env_seed=1):
    from elegantrl_amd.envs import PointChasingVecEnv
    from elegantrl_amd.train import Config
    cls, S, A = _agent_class(kind), 4 * dim, dim
    args = Config(cls, None, {"env_name": "PointChasingVecEnv", "num_envs": N, "max_step": max_step, "state_dim": S, "action_dim": A,
                              "if_discrete": False})
    args.net_dims, args.reward_scale, args.fused_rollout = list(net), scale, fused
    args.random_seed = 7 if kind == "ppo" else 3
    if kind == "ppo":
        args.learning_rate = 1e-3
    if kind == "modsac":
        args.fused_mod_rollout = True
    th.manual_seed(seed)
    agent = cls(args.net_dims, S, A, gpu_id=0, args=args)
    if kind == "ppo":
        with th.no_grad():                                     # non-trivial normalisation vectors and action std
            g = th.Generator(device=DEV).manual_seed(seed + 1)
            agent.act.state_avg[:] = 0.1 * th.randn(S, device=DEV, generator=g)
            agent.act.state_std[:] = 1.0 + 0.2 * th.rand(S, device=DEV, generator=g)
            agent.cri.state_avg[:] = 0.1 * th.randn(S, device=DEV, generator=g)
            agent.cri.state_std[:] = 1.0 + 0.2 * th.rand(S, device=DEV, generator=g)
            agent.act.action_std_log[:] = -0.3 + 0.1 * th.randn(A, device=DEV, generator=g)
    env = PointChasingVecEnv(dim=dim, num_envs=N, max_step=max_step, gpu_id=0, seed=env_seed)
    agent.last_state = env.reset()[0]
    return agent, env, args


def _near_starts(*envs):
    """odd envs a hair outside the catch radius, on the side their target drifts to (its velocity gains a U[0, 1) draw per component and
    step), so that the launches contain terminals (catches) besides the time limits; the same rows on every env"""
    for env in envs:
        d = env.dim
        s = env.state.clone()
        odd = th.arange(env.num_envs, device=DEV) % 2 == 1
        shift = th.zeros(d, device=DEV)
        shift[0] = d + 0.002
        s[odd, 2 * d:3 * d] = s[odd, :d] + shift
        env.state.copy_(s)
        env.distance.copy_(th.where(odd, th.tensor(d + 0.002, device=DEV), env.distance))
        env.state_epoch += 1


def _count(env, name):
    calls = []
    inner = getattr(env, name)
    setattr(env, name, lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    return calls


# ---- 1. one launch against the per-step loop ---------------------------------------------------------------------------------------------------
PPO_CASES = [(16, 2, (32, 32), 1.0), (16, 2, (128, 64), 0.5), (16, 3, (32, 32), 0.5), (16, 3, (128, 64), 1.0),
             (33, 2, (32, 32), 0.5), (33, 2, (128, 64), 1.0), (33, 3, (32, 32), 1.0), (33, 3, (128, 64), 0.5)]


@pytest.mark.parametrize("N,dim,net,scale", PPO_CASES)
@pytest.mark.parametrize("inject", [True, False], ids=["injected-noise", "philox"])
def test_ppo_one_launch_rollout_is_bit_identical_to_the_per_step_loop(N, dim, net, scale, inject):
    """erl_rollout_pointchasing_f32 against erl_rollout_step_f32 + erl_pointchasing_step_f32 per step, two consecutive rollouts; the
    epilogue's advantages and reward sums against erl_gae_scan_f32(EXACT) on the rows the launch wrote"""
    from elegantrl_amd import ops
    (fa, fe, _), (pa, pe, _) = (_make("ppo", N, dim, net, scale=scale, fused=f) for f in (True, False))
    _near_starts(fe, pe)
    fa.last_state, pa.last_state = fe.state.clone(), pe.state.clone()
    fa._fused_gae_explicit = True
    assert th.equal(fa._flat, pa._flat) and th.equal(fe.state, pe.state) and th.equal(fe.distance, pe.distance)
    launches, steps = _count(fe, "fused_rollout"), _count(pe, "raw_stepper")
    g = th.Generator(device=DEV).manual_seed(11)
    seen_terminal = seen_truncate = False
    for it in range(2):
        noise = th.randn((H, N, dim), device=DEV, generator=g) if inject else None
        f_items = fa._explore_vec_env(fe, H, noise=noise)
        p_items = pa._explore_vec_env(pe, H, noise=noise)
        # (the continuous AgentPPO has no `rollout_path` -- only AgentDiscretePPO sets one --: the route is read off the launch counts
        # and the rollout cache that only the one-launch route leaves)
        assert len(launches) == it + 1 and len(steps) == it + 1              # one launch on one side, the per-step kernels on the other
        assert fa._rollout_cache is not None and pa._rollout_cache is None
        for n, a, b in zip(("states", "actions", "logprobs", "rewards", "undones", "unmasks"), f_items, p_items):
            assert a.dtype == b.dtype and a.shape == b.shape, n
            assert th.equal(a, b), f"{n} differs at rollout {it}: {(a != b).sum().item()} elements"
        assert th.equal(fa.last_state, pa.last_state) and th.equal(fe.state, pe.state) and th.equal(fa.last_state, fe.state)
        assert th.equal(fe.distance, pe.distance)
        assert th.equal(fe.step_count, pe.step_count) and th.equal(fe.episode, pe.episode)
        assert fa.rng_counter == pa.rng_counter == (it + 1) * H
        states, _, _, rewards, undones, unmasks = f_items
        seen_terminal, seen_truncate = seen_terminal or bool((~undones).any()), seen_truncate or bool((~unmasks).any())
        c = fa._rollout_cache
        # against the value pre-pass (another summation order: a tolerance; the bit-exact pin of the values is the test below)
        np.testing.assert_allclose(c["values"].cpu().numpy(), pa.get_values(p_items[0]).cpu().numpy(), rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(c["next_value"].cpu().numpy(), pa.get_values(pa.last_state).cpu().numpy(), rtol=2e-5, atol=2e-5)
        # the epilogue on flags that are not constant
        adv, ret = ops.gae_scan(rewards.clone(), undones.clone(), unmasks, c["values"], c["next_value"], float(fa.gamma),
                                float(fa.lambda_gae_adv), use_v_trace=fa.if_use_v_trace, mutate=True, algo="exact")
        assert "adv" in c and th.equal(c["adv"], adv) and th.equal(c["ret"], ret)
    assert seen_terminal and seen_truncate, "the case is meant to contain catches and time limits"


@pytest.mark.parametrize("N,dim,net,scale", [(33, 2, (32, 32), 0.5), (16, 3, (128, 64), 1.0), (33, 3, (128, 64), 1.0)])
@pytest.mark.parametrize("inject", [True, False], ids=["injected-noise", "philox"])
def test_ppo_values_of_one_launch_are_those_of_single_step_launches_bit_for_bit(N, dim, net, scale, inject):
    """erl_rollout_pointchasing_f32 with H = 12 against twelve launches with H = 1 from the same state: `values` row t is the value the
    t-th short launch leaves, `next_value` is the last short launch's, and the bootstrap value of short launch t is the value of short
    launch t + 1 -- all bit for bit, as are the six buffers, the env and the epilogue's advantages recomputed from the short launches'
    values.  In the short launches every critic input is normalised by the kernel's prologue from the state in global memory; in the long
    one, from step 1 on, by the env step's statements that rewrite the tile (resets included)."""
    from elegantrl_amd import ops
    (la, le, _), (sa, se, _) = (_make("ppo", N, dim, net, scale=scale) for _ in range(2))
    _near_starts(le, se)
    la.last_state, sa.last_state = le.state.clone(), se.state.clone()
    la._fused_gae_explicit = sa._fused_gae_explicit = True
    short_launches = _count(se, "fused_rollout")
    g = th.Generator(device=DEV).manual_seed(11)
    noise = th.randn((H, N, dim), device=DEV, generator=g) if inject else None
    long_items = la._explore_vec_env(le, H, noise=noise)
    lc = la._rollout_cache
    rows, values, boots = [], [], []
    for t in range(H):
        items = sa._explore_vec_env(se, 1, noise=None if noise is None else noise[t:t + 1])
        c = sa._rollout_cache
        rows.append([x.clone() for x in items])
        values.append(c["values"].clone())
        boots.append(c["next_value"].clone())
    assert len(short_launches) == H and sa.rng_counter == la.rng_counter == H
    for i, n in enumerate(("states", "actions", "logprobs", "rewards", "undones", "unmasks")):
        assert th.equal(long_items[i], th.cat([r[i] for r in rows])), n
    assert th.equal(le.state, se.state) and th.equal(le.distance, se.distance) and th.equal(la.last_state, sa.last_state)
    assert th.equal(le.step_count, se.step_count) and th.equal(le.episode, se.episode)
    short_values = th.cat(values)
    assert lc["values"].shape == short_values.shape == (H, N)
    assert th.equal(lc["values"], short_values), f"values differ in {(lc['values'] != short_values).sum().item()} elements"
    assert th.equal(lc["next_value"], boots[-1])
    for t in range(H - 1):
        assert th.equal(boots[t], values[t + 1][0]), t
    _, _, _, rewards, undones, unmasks = long_items
    assert bool((~undones).any()) and bool((~unmasks).any()), "the case is meant to contain catches and time limits"
    adv, ret = ops.gae_scan(rewards.clone(), undones.clone(), unmasks, short_values, boots[-1], float(la.gamma), float(la.lambda_gae_adv),
                            use_v_trace=la.if_use_v_trace, mutate=True, algo="exact")
    assert th.equal(lc["adv"], adv) and th.equal(lc["ret"], ret)


def test_ppo_epilogue_beyond_128_steps_reads_non_constant_flags_back_from_the_buffers():
    """H = 130 > 128: the epilogue's inputs do not stay in LDS, it reads rewards, values and flags back from the rows the launch wrote
    (args.fused_gae forced on, as in the Pendulum twin) -- here with terminals (catches) and time limits among them"""
    from elegantrl_amd import ops
    N, dim, horizon = 33, 2, 130
    (fa, fe, _), (pa, pe, _) = (_make("ppo", N, dim, (32, 32), scale=0.5, fused=f) for f in (True, False))
    _near_starts(fe, pe)
    fa.last_state, pa.last_state = fe.state.clone(), pe.state.clone()
    fa._fused_gae_explicit = True
    f_items = fa._explore_vec_env(fe, horizon)
    p_items = pa._explore_vec_env(pe, horizon)
    assert fa._rollout_cache is not None and pa._rollout_cache is None
    for n, a, b in zip(("states", "actions", "logprobs", "rewards", "undones", "unmasks"), f_items, p_items):
        assert th.equal(a, b), n
    assert th.equal(fe.state, pe.state) and th.equal(fe.distance, pe.distance)
    assert th.equal(fe.step_count, pe.step_count) and th.equal(fe.episode, pe.episode)
    _, _, _, rewards, undones, unmasks = f_items
    assert bool((~undones).any()) and int((~unmasks).sum()) >= 25 * N
    c = fa._rollout_cache
    adv, ret = ops.gae_scan(rewards.clone(), undones.clone(), unmasks, c["values"], c["next_value"], float(fa.gamma),
                            float(fa.lambda_gae_adv), use_v_trace=fa.if_use_v_trace, mutate=True, algo="exact")
    assert "adv" in c and th.equal(c["adv"], adv) and th.equal(c["ret"], ret)


SAC_CASES = [(16, 2, (256, 256), 1.0), (33, 3, (64, 48), 0.5), (33, 2, (128, 64), 1.0), (16, 3, (128, 64), 0.5)]


@pytest.mark.parametrize("kind", ["sac", "modsac"])
@pytest.mark.parametrize("N,dim,net,scale", SAC_CASES)
@pytest.mark.parametrize("inject", [True, False], ids=["injected-noise", "philox"])
def test_sac_one_launch_rollout_is_bit_identical_to_the_per_step_loop(kind, N, dim, net, scale, inject):
    """erl_sac_rollout_[mod_]pointchasing_f32 against the explore launch (ModSAC: the tile action) + erl_pointchasing_step_f32 per step"""
    (fa, fe, _), (pa, pe, _) = (_make(kind, N, dim, net, scale=scale, fused=f) for f in (True, False))
    _near_starts(fe, pe)
    fa.last_state, pa.last_state = fe.state.clone(), pe.state.clone()
    assert th.equal(fa._actor_flat, pa._actor_flat) and th.equal(fe.state, pe.state)
    f_launches, p_launches, p_steps = _count(fe, "fused_rollout_offpolicy"), _count(pe, "fused_rollout_offpolicy"), _count(pe, "step_into")
    g = th.Generator(device=DEV).manual_seed(2)
    seen_terminal = seen_truncate = False
    for it in range(2):
        noise = th.randn((H, N, dim), device=DEV, generator=g) if inject else None
        f_items = fa._explore_vec_env(fe, H, noise=noise)
        p_items = pa._explore_vec_env(pe, H, noise=noise)
        assert len(f_launches) == it + 1 and len(p_launches) == 0 and len(p_steps) == (it + 1) * H
        entry = "erl_sac_rollout_mod_" if kind == "modsac" else "erl_sac_rollout_"
        assert fa.rollout_path.startswith(f"one launch ({entry}*_f32 through PointChasingVecEnv.fused_rollout_offpolicy"), fa.rollout_path
        assert pa.rollout_path.startswith("per-step loop") and "fused_rollout is off" in pa.rollout_path
        if kind == "modsac":
            assert "tile action erl_sac_explore_action_tile_f32" in pa.rollout_path
        for name, x, y in zip(("states", "actions", "rewards", "undones", "unmasks"), f_items, p_items):
            assert x.dtype == y.dtype and x.shape == y.shape, name
            assert th.equal(x, y), f"{name} differs at rollout {it}: {(x != y).sum().item()} elements"
        assert th.equal(fa.last_state, pa.last_state) and th.equal(fe.state, pe.state) and th.equal(fe.distance, pe.distance)
        assert th.equal(fe.step_count, pe.step_count) and th.equal(fe.episode, pe.episode)
        assert fa.rng_counter == pa.rng_counter == (it + 1) * H
        seen_terminal, seen_truncate = seen_terminal or bool((~f_items[3]).any()), seen_truncate or bool((~f_items[4]).any())
    assert seen_terminal and seen_truncate, "the case is meant to contain catches and time limits"


# ---- 2. the evaluation form against the training form under zero noise -------------------------------------------------------------------------
def _kernel_table(agent, env, horizon, offpolicy):
    """the evaluation entry with horizon `horizon` (no reset), then the compaction"""
    from elegantrl_amd import _hip
    from elegantrl_amd.envs.vec_envs import compact_episodes
    n_envs = env.num_envs
    nbytes = _hip.lib().erl_eval_workspace_bytes(n_envs, horizon)
    ws = th.full((nbytes,), 0xAB, dtype=th.uint8, device=DEV)          # garbage: the launch must write every element it later reads
    rows = th.full((n_envs * horizon, 2), -7.0, dtype=th.float32, device=DEV)
    count = th.full((1,), -1, dtype=th.int32, device=DEV)
    agent._sync_modules()
    (env.fused_evaluate_offpolicy if offpolicy else env.fused_evaluate)(agent, horizon, ws)
    compact_episodes(ws, n_envs, horizon, rows, count)
    n = int(count.item())
    assert 0 <= n <= n_envs * horizon and (rows[n:] == -7.0).all()
    return rows[:n].cpu().numpy()


@pytest.mark.parametrize("kind,net", [("ppo", (32, 32)), ("ppo", (128, 64)), ("sac", (256, 256)), ("sac", (64, 48)), ("modsac", (256, 256)),
                                      ("modsac", (128, 64))])
@pytest.mark.parametrize("N,dim", [(33, 2), (16, 3)])
def test_eval_kernel_is_the_training_rollout_under_zero_noise(kind, net, N, dim):
    """the episode table, the env state, `distance` and the counters, two passes without a reset; catches and time limits both end episodes"""
    (a_agent, a_env, _), (b_agent, b_env, _) = (_make(kind, N, dim, net, env_seed=5) for _ in range(2))
    _near_starts(a_env, b_env)
    b_agent.last_state = b_env.state.clone()
    zeros = th.zeros((H, N, dim), device=DEV)
    for it in range(2):
        rewards, undones, unmasks = b_agent._explore_vec_env(b_env, H, noise=zeros)[-3:]
        ref = oracle_table(rewards, undones, unmasks)
        got = _kernel_table(a_agent, a_env, H, offpolicy=kind != "ppo")
        done = ~(undones & unmasks)
        assert int(done.sum(0).max()) >= 2 and bool((~done[-1]).any()), "the case is meant to contain several episodes per env and an open tail"
        if it == 0:
            assert bool((~undones).any()) and bool((~unmasks).any()), "the case is meant to contain catches and time limits"
        assert th.equal(a_env.state, b_env.state) and th.equal(a_env.distance, b_env.distance), f"env differs at pass {it}"
        assert th.equal(a_env.step_count, b_env.step_count) and th.equal(a_env.episode, b_env.episode)
        assert got.shape == ref.shape, f"{got.shape[0]} episodes from the kernels, {ref.shape[0]} from the rollout"
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"episode table differs at pass {it}"


# ---- 3. agent.evaluate_env against the Evaluator's loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,net", [("ppo", (128, 64)), ("sac", (128, 64)), ("modsac", (128, 64))])
def test_evaluate_env_agrees_with_the_evaluator_loop(kind, net):
    """episode count and lengths exactly; returns to the bounds of the Pendulum twins (tests/test_eval_fused_gpu.py PEND_*_BOUND, for
    AgentModSAC tests/test_modsac_rollout_gpu.py MOD_*_BOUND: three times the largest gap measured there between the loop on the torch
    module and the kernels' arithmetic)"""
    from elegantrl_amd.train.evaluator import get_cumulative_rewards_and_step_from_vec_env
    from tests.test_eval_fused_gpu import PEND_EP_BOUND, PEND_MEAN_BOUND
    from tests.test_modsac_rollout_gpu import MOD_EP_BOUND, MOD_MEAN_BOUND
    ep_bound, mean_bound = (MOD_EP_BOUND, MOD_MEAN_BOUND) if kind == "modsac" else (PEND_EP_BOUND, PEND_MEAN_BOUND)
    agent, env, _ = _make(kind, 64, 2, net, max_step=40, env_seed=5)
    fused = agent.evaluate_env(env)
    assert fused is not None and fused.dtype == th.float32 and fused.device.type == "cpu"
    loop = get_cumulative_rewards_and_step_from_vec_env(env, agent.act)
    assert fused.shape == loop.shape and fused.shape[0] >= 64 and fused.shape[1] == 2
    assert th.equal(fused[:, 1], loop[:, 1])
    ep = float((fused[:, 0] - loop[:, 0]).abs().max())
    mean = abs(float(fused[:, 0].mean()) - float(loop[:, 0].mean()))
    print(f"[{kind}] per-episode gap {ep:.6g} (bound {ep_bound:.6g}), mean gap {mean:.6g} (bound {mean_bound:.6g})")
    assert ep <= ep_bound and mean <= mean_bound


# ---- 4. the draw does not depend on the kernel that makes it ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_reset_rows_are_the_same_from_the_three_kernels(dim):
    """max_step = 3: after three steps every env has been reset once, whatever its actions were -- the rows drawn by the per-step kernel, by the
    PPO launch and by the SAC launch (and the distances recomputed from them) are equal bit for bit"""
    N = 33
    ppo, e_ppo, _ = _make("ppo", N, dim, (32, 32), max_step=3)
    sac, e_sac, _ = _make("sac", N, dim, (64, 48), max_step=3)
    _, e_step, _ = _make("sac", N, dim, (64, 48), max_step=3, fused=False)
    launches = _count(e_ppo, "fused_rollout"), _count(e_sac, "fused_rollout_offpolicy")
    ppo._explore_vec_env(e_ppo, 3)
    sac._explore_vec_env(e_sac, 3)
    for _ in range(3):
        _, _, te, tr, _ = e_step.step(th.zeros((N, dim), device=DEV))
    assert [len(x) for x in launches] == [1, 1] and bool(tr.all()) and not bool(te.any())
    for env in (e_ppo, e_sac, e_step):
        assert bool((env.episode == 1).all()) and bool((env.step_count == 0).all())
    assert th.equal(e_ppo.state, e_step.state) and th.equal(e_sac.state, e_step.state)
    assert th.equal(e_ppo.distance, e_step.distance) and th.equal(e_sac.distance, e_step.distance)
    assert not bool(e_step.state[:, dim:2 * dim].any()) and not bool(e_step.state[:, 3 * dim:].any())
    assert float(e_step.distance.min()) > dim


# ---- 5. train_agent end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ppo", "sac"])
def test_train_agent_three_iterations(kind, tmp_path, capsys):
    from elegantrl_amd import train_agent
    from elegantrl_amd.envs import PointChasingVecEnv
    from elegantrl_amd.train import Config
    made = []

    base = _agent_class(kind)

    def watched_init(self, *a, **k):
        base.__init__(self, *a, **k)
        made.append(self)

    Watched = type(base.__name__ + "Watched", (base,), {"__init__": watched_init})      # (Config reads on- / off-policy from the class name)
    args = Config(Watched, PointChasingVecEnv, {"env_name": "PointChasingVecEnv", "num_envs": 64, "max_step": 20, "state_dim": 8,
                                                "action_dim": 2, "if_discrete": False, "dim": 2})
    args.net_dims = [128, 64]
    args.horizon_len, args.batch_size = 16, 128
    args.repeat_times = 16.0                                   # two minibatch steps per iteration either way
    if kind == "sac":
        args.buffer_size = 4096
    args.break_step, args.eval_per_step, args.eval_times = 16 * 3, 16 * 2, 64
    args.cwd, args.gpu_id, args.random_seed = str(tmp_path / "run"), 0, 0
    train_agent(args, if_single_process=True)
    th.set_grad_enabled(True)                                                           # (train_agent leaves autograd switched off)
    out = capsys.readouterr().out
    agent, = made
    if kind == "ppo":
        assert agent._one_launch_reason(PointChasingVecEnv(dim=2, num_envs=64, max_step=20), "fused_rollout") is None
    else:
        assert agent.rollout_path.startswith("one launch (erl_sac_rollout_*_f32 through PointChasingVecEnv")
    assert "| Evaluator: fused evaluation" in out and "loop evaluation" not in out
    files = os.listdir(args.cwd)
    assert "act.pth" in files and "recorder.npy" in files
    rec = np.load(os.path.join(args.cwd, "recorder.npy"))
    assert rec.shape[0] >= 1 and np.isfinite(rec[:, :4]).all(), rec
    actor = th.load(os.path.join(args.cwd, "act.pth"), weights_only=False)
    assert all(bool(th.isfinite(p).all()) for p in actor.parameters())
