"""MountainCarGpuVecEnv (erl_mountaincar_step_f32, csrc/mountaincar_step.h): the per-step kernel against the fp64 restatement of the
dynamics (tests/mountaincar_ref.py), teacher-forced -- every step is compared from the kernel's own previous state --, every branch of
the step from injected states, the goal reached through the dynamics, and the episode bookkeeping with the Philox reset draw.

Tolerance of (a).  Not a number chosen here: 4 times the largest one-step difference between the restatement run in fp32 and in fp64
on the very inputs the device saw (its own previous states, the same actions), computed in the test.  The factor covers cosf differing
from numpy's fp32 cosine by an ulp or two; everything else in a step is a handful of fp32 sums and products.  The same bound is applied
to position and velocity separately (the velocity is ten times smaller, a joint bound would say little about it).
No test here says that an agent learns the task: under a uniformly random policy no episode ends by `terminal` within 200 steps, so PPO
from scratch sees a constant reward."""
import numpy as np
import pytest
import torch as th

from tests import mountaincar_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def make_env(n, max_step=200, seed=5):
    from elegantrl_amd.envs import MountainCarGpuVecEnv
    env = MountainCarGpuVecEnv(n, max_step=max_step, gpu_id=0, seed=seed)
    env.reset()
    return env


def inject(env, rows):
    """rows (k, 2) into the first k envs"""
    rows = th.tensor(rows, dtype=th.float32, device=DEV)
    env.state[:len(rows)] = rows
    env.state_epoch += 1


def step(env, actions):
    """one env.step -> numpy (state, reward, terminal, truncate)"""
    state, reward, terminal, truncate, _ = env.step(th.as_tensor(np.asarray(actions), dtype=th.int64).to(DEV))
    assert state.dtype == th.float32 and reward.dtype == th.float32 and terminal.dtype == th.bool and truncate.dtype == th.bool
    assert th.equal(state, env.state)
    return state.cpu().numpy(), reward.cpu().numpy(), terminal.cpu().numpy(), truncate.cpu().numpy()


def test_attributes_and_reset():
    from elegantrl_amd.envs import MountainCarGpuVecEnv
    assert MountainCarGpuVecEnv(8).max_step == 200          # the constructor's default
    env, twin, other = make_env(300), make_env(300), make_env(300, seed=6)
    assert env.if_discrete and (env.state_dim, env.action_dim, env.env_name, env.num_envs) == (2, 3, "MountainCar-v0", 300)
    e0 = env.state_epoch
    s0, info = env.reset()
    assert info == {} and env.state_epoch == e0 + 1
    assert s0.shape == (300, 2) and s0.dtype == th.float32 and s0.is_contiguous() and env.state.is_contiguous()
    assert th.equal(s0, env.state) and th.equal(s0, twin.state) and not th.equal(s0, other.state)
    pos, vel = s0[:, 0].cpu().numpy(), s0[:, 1].cpu().numpy()
    assert (pos >= F32(R.RESET_LO)).all() and (pos < F32(R.RESET_HI)).all() and 0.05 < pos.std() < 0.065          # U[-0.6, -0.4): std 0.0577
    assert (vel == 0).all()
    assert int(env.step_count.abs().sum()) == 0 and int(env.episode.abs().sum()) == 0


def test_a_trajectories_from_reset_against_fp64():
    """N = 64, 200 steps of seeded random actions, two columns out of range; max_step is above 200, so that every one of the 200 steps is
    a step of the dynamics (truncation and restart: test_d)"""
    N, STEPS = 64, 200
    env = make_env(N, max_step=500)
    rng = np.random.default_rng(11)
    acts = rng.integers(0, 3, (STEPS, N))
    acts[:, 17], acts[:, 63] = 7, -1          # neither 0, 1 nor 2: no push
    dev_err, f32_err = np.zeros(2), np.zeros(2)
    for t in range(STEPS):
        prev = env.state.cpu().numpy()
        got, reward, term, trunc = step(env, acts[t])
        ref, term_ref, margin = R.mountaincar_step(prev, acts[t])
        ref32 = R.mountaincar_step(prev, acts[t], dtype=F32)[0]
        assert ref32.dtype == F32 and ref.dtype == np.float64
        np.testing.assert_array_equal(term, term_ref)
        assert not term.any() and not trunc.any() and (reward == -1).all()          # a random policy does not get there
        dev_err = np.maximum(dev_err, np.abs(got.astype(np.float64) - ref).max(axis=0))
        f32_err = np.maximum(f32_err, np.abs(ref32.astype(np.float64) - ref).max(axis=0))
    print(f"(a) {STEPS} steps x {N} envs, largest one-step deviation from fp64 (position, velocity): device {dev_err[0]:.3e}, {dev_err[1]:.3e}; "
          f"fp32 numpy {f32_err[0]:.3e}, {f32_err[1]:.3e}; bound 4 x fp32 numpy = {4 * f32_err.max():.3e}")
    assert f32_err.min() > 0
    assert dev_err.max() <= 4 * f32_err.max(), (dev_err, f32_err)
    assert (dev_err <= 4 * f32_err).all(), (dev_err, f32_err)
    # the car moved: the comparison is not one of states at rest
    assert float(env.state[:, 1].abs().max()) > 1e-3 and int(env.step_count.min()) == STEPS
    # an out-of-range action pushes nowhere: the same step as action 1
    a, b, c = make_env(64, seed=2), make_env(64, seed=2), make_env(64, seed=2)
    sa = step(a, np.ones(64))[0]
    sb = step(b, np.full(64, 5))[0]
    sc = step(c, np.zeros(64))[0]
    np.testing.assert_array_equal(sa, sb)
    assert (sa[:, 1] != sc[:, 1]).all()


# (position, velocity, action) of the injected rows of test_b; 3..5 are the goal rows
ROWS = [(-1.19, -0.05, 0),        # runs into the left wall: position exactly -1.2, velocity exactly 0
        (-0.5, 0.0699, 2),        # velocity clipped to +0.07
        (-0.5, -0.0699, 0),       # velocity clipped to -0.07
        (0.45, 0.05, 0),          # terminal at step 2
        (0.45, 0.05, 1),          # terminal at step 2
        (0.45, 0.05, 2),          # terminal at step 1
        (0.56, -0.03, 0),         # stays beyond the goal line while rolling back: not terminal
        (0.58, 0.06, 2)]          # clipped at the right end, 0.6: terminal


def test_b_every_branch_from_injected_states():
    """flags are compared exactly, nothing excluded: every row is well off its threshold (margins are printed)"""
    N, K = 16, len(ROWS)
    env = make_env(N, max_step=500)
    inject(env, [r[:2] for r in ROWS])
    acts = np.ones(N, dtype=np.int64)
    acts[:K] = [r[2] for r in ROWS]
    flags = []
    for t in range(2):
        prev = env.state.cpu().numpy()
        got, reward, term, trunc = step(env, acts)
        ref, term_ref, margin = R.mountaincar_step(prev, acts)
        ref32, term_ref32, _ = R.mountaincar_step(prev, acts, dtype=F32)
        print(f"(b) step {t + 1}: terminal {term[:K].astype(int).tolist()}, goal margins {np.round(margin[:K], 5).tolist()}")
        np.testing.assert_array_equal(term, term_ref)
        np.testing.assert_array_equal(term, term_ref32)
        assert not trunc.any() and (reward == -1).all()          # -1 on the terminal step as well
        live = ~term
        np.testing.assert_allclose(got[live], ref[live], rtol=0, atol=1e-6)
        if t == 0:
            assert got[0, 0] == F32(-1.2) and got[0, 1] == 0.0 and not term[0]
            assert got[1, 1] == F32(0.07) and ref[1, 1] == 0.07 and got[2, 1] == F32(-0.07) and ref[2, 1] == -0.07
            assert got[6, 0] >= 0.5 and got[6, 1] < 0 and not term[6]
            assert ref[7, 0] == 0.6 and term[7]
            assert term[:K].tolist() == [False, False, False, False, False, True, False, True]
        else:
            assert term[3] and term[4]
        # a terminal row restarted in the same step
        fresh = got[term]
        assert (fresh[:, 0] >= F32(R.RESET_LO)).all() and (fresh[:, 0] < F32(R.RESET_HI)).all() and (fresh[:, 1] == 0).all()
        flags.append(term)
    np.testing.assert_array_equal(env.episode.cpu().numpy(), flags[0].astype(np.int32) + flags[1].astype(np.int32))
    sc = env.step_count.cpu().numpy()
    assert sc[5] == 1 and sc[3] == 0 and sc[4] == 0 and sc[0] == 2


def test_c_the_goal_is_reached_through_the_dynamics():
    """push right while the velocity is not negative, else left: every env gets to the goal after 113..125 steps, at the step the fp64
    restatement says, except for at most 1 % of envs that may be one step off (a crossing within rounding of the goal line)"""
    N, H = 256, 130
    env = make_env(N)
    start = env.state.cpu().numpy()
    first = np.zeros(N, dtype=np.int64)
    for t in range(1, H + 1):
        act = th.where(env.state[:, 1] >= 0, 2, 0)
        _, reward, terminal, truncate, _ = env.step(act)
        term = terminal.cpu().numpy()
        assert not truncate.any() and (reward == -1).all()
        first[(first == 0) & term] = t
    ref = R.first_terminal_steps(start, H)
    assert (ref > 0).all(), "the restatement itself does not reach the goal"
    diff = np.abs(first - ref)
    print(f"(c) first terminal step: device {first.min()}..{first.max()}, fp64 {ref.min()}..{ref.max()}; {int((diff != 0).sum())} of {N} envs differ, "
          f"largest difference {int(diff.max())}")
    assert (first > 0).all(), f"{int((first == 0).sum())} envs never terminated"
    assert diff.max() <= 1 and (diff != 0).mean() <= 0.01


def test_d_episode_bookkeeping_and_reset_draws():
    N, M, MAX_STEP, STEPS = 300, 130, 7, 16
    env, small, other = make_env(N, MAX_STEP), make_env(M, MAX_STEP), make_env(N, MAX_STEP, seed=6)
    small.state.copy_(env.state[:M])          # the same trajectories on the shared rows (reset() draws depend on num_envs; the kernel's do not)
    rng = np.random.default_rng(41)
    sc_ref, ep_ref = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    resets, n_trunc, epoch0 = [], 0, env.state_epoch
    for t in range(STEPS):
        a = rng.integers(0, 3, N)
        got, reward, term, trunc = step(env, a)
        s2, r2, _, u2 = step(small, a[:M])
        step(other, a)
        np.testing.assert_array_equal(got[:M], s2)
        np.testing.assert_array_equal(trunc[:M], u2)
        sc_ref += 1
        assert not term.any() and (reward == -1).all()
        np.testing.assert_array_equal(trunc, sc_ref >= MAX_STEP)
        done = term | trunc
        sc_ref[done] = 0
        ep_ref[done] += 1
        np.testing.assert_array_equal(env.step_count.cpu().numpy(), sc_ref)
        np.testing.assert_array_equal(env.episode.cpu().numpy(), ep_ref)
        if done.any():
            fresh = got[done]
            assert (fresh[:, 0] >= F32(R.RESET_LO)).all() and (fresh[:, 0] < F32(R.RESET_HI)).all() and (fresh[:, 1] == 0).all()
            assert not th.equal(env.state, other.state)          # another seed, other draws
            resets.append(fresh[:, 0])
        n_trunc += int(trunc.sum())
    assert env.state_epoch == epoch0 + STEPS and n_trunc == 2 * N          # steps 7 and 14 truncate every env
    resets = np.concatenate(resets)
    # the draws differ across envs and episodes, and fill the interval
    assert len(np.unique(resets)) > 0.99 * len(resets) and abs(resets.mean() + 0.5) < 0.01 and 0.05 < resets.std() < 0.065


def test_d_the_draw_does_not_depend_on_the_kernel_that_makes_it():
    """(seed, env, episode) -> the same bits from the per-step kernel and from the one-launch rollout: with max_step 7 every env is
    truncated at steps 7 and 14 whatever the actions were, so after 14 steps both hold the draws of episode 2; and the draw has tag
    words of its own: CartPole's first component under the same keys is another number"""
    from elegantrl_amd.envs import CartPoleGpuVecEnv
    from tests.test_mountaincar_rollout_gpu import make
    N, MAX_STEP = 300, 7
    per_step = make_env(N, MAX_STEP)
    agent, fused, _ = make(N, (64, 32), MAX_STEP)
    assert th.equal(per_step.state, fused.state)
    rng = np.random.default_rng(43)
    for k in (1, 2):
        for t in range(MAX_STEP):
            step(per_step, rng.integers(0, 3, N))
        agent.explore_env(fused, MAX_STEP)
        assert agent.rollout_path == "one-launch"
        assert th.equal(per_step.state, fused.state) and (fused.state[:, 1] == 0).all()
        assert th.equal(per_step.episode, fused.episode) and int(fused.episode.min()) == int(fused.episode.max()) == k
        assert th.equal(per_step.step_count, fused.step_count) and int(fused.step_count.abs().sum()) == 0
    cart = CartPoleGpuVecEnv(N, max_step=1, gpu_id=0, seed=5)          # max_step 1: one step and every env holds the draw of episode 1
    cart.reset()
    cart.step(th.zeros(N, dtype=th.int64, device=DEV))
    mc = make_env(N, 1)
    step(mc, np.ones(N))
    u_cart = (cart.state[:, 0].double() + 0.05) / 0.1
    u_mc = (mc.state[:, 0].double() + 0.6) / 0.2
    assert float(((u_cart - u_mc).abs() < 1e-4).double().mean()) < 0.01
