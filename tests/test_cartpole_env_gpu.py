"""CartPoleGpuVecEnv (erl_cartpole_step_f32, csrc/cartpole_step.h): the per-step kernel against the fp64 restatement of the physics
(tests/cartpole_ref.py), its counters and flags, the Philox reset draws, and the env protocol under AgentDiscretePPO's per-step loop."""
import numpy as np
import pytest
import torch as th

from tests.cartpole_ref import cartpole_step_f64

DEV = "cuda:0"
N, STEPS, MAX_STEP, SEED = 300, 60, 25, 11
BAND = 1e-5          # |margin| below which fp32 and fp64 may disagree on a terminal flag


def _actions():
    return np.random.default_rng(SEED).integers(0, 2, (STEPS, N))


def test_restatement_alone_keeps_the_threshold_band_rare():
    """no GPU: the fp64 restatement under the test's own actions (resets from numpy's generator) -- rows whose |x| - 2.4 or
    |theta| - 12 degrees lies within 1e-5 of zero are under 1 % of rows, so the band excuses almost nothing"""
    rng = np.random.default_rng(SEED + 1)
    acts = _actions()
    s = rng.random((N, 4)) * 0.1 - 0.05
    sc = np.zeros(N, dtype=np.int64)
    near = terms = truncs = 0
    for t in range(STEPS):
        s, term, margins = cartpole_step_f64(s, acts[t])
        near += int((np.abs(margins) < BAND).any(axis=1).sum())
        sc += 1
        trunc = (sc >= MAX_STEP) & ~term
        done = term | trunc
        terms, truncs = terms + int(term.sum()), truncs + int(trunc.sum())
        s[done] = rng.random((int(done.sum()), 4)) * 0.1 - 0.05
        sc[done] = 0
    assert terms > 0 and truncs > 0
    assert near < 0.01 * STEPS * N, near


@pytest.mark.gpu
def test_step_kernel_matches_fp64_restatement_and_twin():
    from elegantrl_amd.envs import CartPoleGpuVecEnv
    env, twin = (CartPoleGpuVecEnv(N, max_step=MAX_STEP, gpu_id=0, seed=5) for _ in range(2))
    other = CartPoleGpuVecEnv(N, max_step=MAX_STEP, gpu_id=0, seed=6)
    assert env.if_discrete and (env.state_dim, env.action_dim, env.env_name) == (4, 2, "CartPole-v1")
    s0, _ = env.reset()
    t0, _ = twin.reset()
    assert th.equal(s0, t0) and not th.equal(s0, other.reset()[0])
    assert s0.shape == (N, 4) and s0.dtype == th.float32 and (s0 >= -0.05).all() and (s0 < 0.05).all()
    acts = _actions()
    sc_ref, ep_ref = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    prev = s0.cpu().numpy()
    n_near = n_term = n_trunc = 0
    resets, epoch0 = [], env.state_epoch
    for t in range(STEPS):
        a = th.from_numpy(acts[t]).to(DEV)
        state, reward, terminal, truncate, info = env.step(a)
        st, rt, tt, ut, _ = twin.step(a.clone())
        assert th.equal(state, st) and th.equal(terminal, tt) and th.equal(truncate, ut)          # one seed: bit for bit
        assert state.dtype == th.float32 and reward.dtype == th.float32 and terminal.dtype == th.bool and truncate.dtype == th.bool
        assert info == {} and (reward == 1).all()
        got, term, trunc = state.cpu().numpy(), terminal.cpu().numpy(), truncate.cpu().numpy()
        ref, term_ref, margins = cartpole_step_f64(prev.astype(np.float64), acts[t])
        near = (np.abs(margins) < BAND).any(axis=1)
        n_near += int(near.sum())
        np.testing.assert_array_equal(term[~near], term_ref[~near])
        sc_ref += 1
        trunc_ref = (sc_ref >= MAX_STEP) & ~term
        np.testing.assert_array_equal(trunc, trunc_ref)
        done = term | trunc
        np.testing.assert_allclose(got[~done], ref[~done], rtol=1e-5, atol=1e-6)
        sc_ref[done] = 0
        ep_ref[done] += 1
        np.testing.assert_array_equal(env.step_count.cpu().numpy(), sc_ref)
        np.testing.assert_array_equal(env.episode.cpu().numpy(), ep_ref)
        assert (got[done] >= -0.05).all() and (got[done] < 0.05).all()
        resets.append(got[done])
        n_term, n_trunc = n_term + int(term.sum()), n_trunc + int(trunc.sum())
        prev = got
    assert env.state_epoch == epoch0 + STEPS
    assert n_term > 0 and n_trunc > 0, (n_term, n_trunc)
    assert n_near < 0.01 * STEPS * N, n_near
    resets = np.concatenate(resets)
    assert len(resets) == n_term + n_trunc > 50
    # the draws differ across envs and episodes: no two reset states alike, no component repeated inside one
    assert len(np.unique(resets, axis=0)) == len(resets)
    assert (np.diff(np.sort(resets, axis=1), axis=1) != 0).all()
    assert abs(resets.mean()) < 0.01 and 0.02 < resets.std() < 0.04          # U[-0.05, 0.05): std 0.0289


@pytest.mark.gpu
def test_any_action_other_than_one_pushes_left():
    from elegantrl_amd.envs import CartPoleGpuVecEnv
    a, b = (CartPoleGpuVecEnv(64, max_step=500, gpu_id=0, seed=2) for _ in range(2))
    a.reset(), b.reset()
    sa = a.step(th.zeros(64, dtype=th.int64, device=DEV))[0]
    sb = b.step(th.full((64,), 7, dtype=th.int64, device=DEV))[0]
    assert th.equal(sa, sb) and (sa[:, 1] < 0).all()


@pytest.mark.gpu
def test_protocol_under_the_per_step_loop():
    """one iteration of AgentDiscretePPO.explore_env with args.fused_rollout = False: the loop takes the new env as it takes CartPoleVecEnv"""
    from elegantrl_amd.agents import AgentDiscretePPO
    from elegantrl_amd.envs import CartPoleGpuVecEnv, CartPoleVecEnv
    from elegantrl_amd.train import Config
    n, H = 48, 12
    out = {}
    for cls in (CartPoleVecEnv, CartPoleGpuVecEnv):
        args = Config(AgentDiscretePPO, cls, {"env_name": "CartPole-v1", "num_envs": n, "max_step": 9, "state_dim": 4, "action_dim": 2,
                                              "if_discrete": True})
        args.net_dims, args.fused_rollout, args.random_seed = [64, 32], False, 1
        th.manual_seed(0)
        agent = AgentDiscretePPO(args.net_dims, 4, 2, gpu_id=0, args=args)
        env = cls(n, max_step=9, gpu_id=0, seed=3)
        agent.last_state = env.reset()[0]
        items = agent.explore_env(env, H)
        assert agent.rollout_path == "loop" and agent.rng_counter == H
        assert agent.last_state.shape == (n, 4) and agent.last_state.dtype == th.float32
        out[cls.__name__] = items
    for x, y in zip(out["CartPoleVecEnv"], out["CartPoleGpuVecEnv"]):
        assert x.shape == y.shape and x.dtype == y.dtype and x.device == y.device
    states, actions, logprobs, rewards, undones, unmasks = out["CartPoleGpuVecEnv"]
    assert actions.dtype == th.int32 and undones.dtype == th.bool and unmasks.dtype == th.bool and states.shape == (H, n, 4)
    assert (~unmasks).any() and (rewards == 1).all()          # max_step 9 within 12 steps: truncations happened
