"""AcrobotGpuVecEnv (erl_acrobot_step_f32, csrc/acrobot_step.h): the per-step kernel against the fp64 restatement of the dynamics
(tests/acrobot_ref.py), teacher-forced -- every step is compared from the kernel's own previous state -- in three regimes, and the
episode bookkeeping with the Philox reset draws.

Tolerances.  Regimes A and B: 1e-5, absolute on the four cos / sin, relative to max(1, |omega|) on the velocities; an fp32 numpy
evaluation of the restatement is within 7.4e-7 (A) / 1.2e-6 (B) of fp64 there, the rest is room for device sinf / cosf / division being
a few ulp off numpy's.  Regime C (velocities over the full +-4 pi / +-9 pi) amplifies rounding -- fp32 numpy is up to 1.8e-5 / 1.7e-3
off -- so there the bound is 8 times the error of the fp32 numpy evaluation on the same rows, computed here."""
import numpy as np
import pytest
import torch as th

from tests import acrobot_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
BAND = 1e-5          # |margin| below which fp32 and fp64 may disagree on a terminal flag
F32 = np.float32


def obs_err(got_obs, ref_phys):
    """(N, 6) error of an observation against the observation of an fp64 physical state: absolute on cos / sin, relative to
    max(1, |omega|) on the velocities (observations, not angles: a wrap may legitimately differ by one turn at +-pi)"""
    ref = R.observe(ref_phys.astype(np.float64))
    e = np.abs(got_obs.astype(np.float64) - ref)
    e[:, 4:] /= np.maximum(1.0, np.abs(ref[:, 4:]))
    return e


def make_env(n, max_step=500, seed=5):
    from elegantrl_amd.envs import AcrobotGpuVecEnv
    env = AcrobotGpuVecEnv(n, max_step=max_step, gpu_id=0, seed=seed)
    env.reset()
    return env


def inject(env, phys):
    env.phys.copy_(th.from_numpy(phys.astype(F32)).to(DEV))
    env.state.copy_(env._observe(env.phys))
    return env.phys.cpu().numpy()


def draw_phys(rng, n, w1, w2):
    return np.stack((rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-w1, w1, n), rng.uniform(-w2, w2, n)), axis=1)


def test_attributes_and_reset():
    env, twin, other = make_env(300), make_env(300), make_env(300, seed=6)
    assert env.if_discrete and (env.state_dim, env.action_dim, env.env_name) == (6, 3, "Acrobot-v1")
    e0 = env.state_epoch
    s0, info = env.reset()
    assert info == {} and env.state_epoch == e0 + 1
    assert s0.shape == (300, 6) and s0.dtype == th.float32 and env.phys.shape == (300, 4) and env.phys.dtype == th.float32
    assert th.equal(s0, twin.state) and th.equal(env.phys, twin.phys) and not th.equal(env.phys, other.phys)
    assert (env.phys >= -0.1).all() and (env.phys < 0.1).all() and 0.05 < float(env.phys.std()) < 0.065          # U[-0.1, 0.1): std 0.0577
    assert obs_err(s0.cpu().numpy(), env.phys.cpu().numpy()).max() < 1e-6
    assert int(env.step_count.abs().sum()) == 0 and int(env.episode.abs().sum()) == 0


def test_regime_a_trajectories_from_reset():
    """N = 300 is ragged against the 256-thread block; 40 steps of random actions, two of them out of range per step"""
    N, STEPS = 300, 40
    env = make_env(N)
    rng = np.random.default_rng(11)
    acts = rng.integers(0, 3, (STEPS, N))
    acts[:, 17], acts[:, 299] = 7, -1          # neither 0, 1 nor 2: torque 0
    worst = 0.0
    for t in range(STEPS):
        prev = env.phys.cpu().numpy()
        state, reward, terminal, truncate, _ = env.step(th.from_numpy(acts[t]).to(DEV))
        assert state.dtype == th.float32 and reward.dtype == th.float32 and terminal.dtype == th.bool and truncate.dtype == th.bool
        assert th.equal(state, env.state) and not truncate.any()
        ref, term_ref, margin, _ = R.acrobot_step(prev, acts[t])
        assert (np.abs(margin) >= BAND).all()          # (the restatement alone: no cell within 1e-5 of the threshold from reset)
        np.testing.assert_array_equal(terminal.cpu().numpy(), term_ref)
        keep = ~term_ref
        e = obs_err(state.cpu().numpy()[keep], ref[keep])
        worst = max(worst, e.max())
        assert e.max() <= TOL, (t, e.max())
        # phys is the state of record and the observation is its own
        assert obs_err(state.cpu().numpy(), env.phys.cpu().numpy()).max() < 1e-6
    print(f"regime A: largest deviation from fp64 over {STEPS} steps x {N} envs: {worst:.3e} (bound {TOL:.0e})")
    # an out-of-range action is torque 0: the same step as action 1
    a, b = make_env(64, seed=2), make_env(64, seed=2)
    sa = a.step(th.ones(64, dtype=th.int64, device=DEV))[0]
    sb = b.step(th.full((64,), 5, dtype=th.int64, device=DEV))[0]
    sc = make_env(64, seed=2).step(th.zeros(64, dtype=th.int64, device=DEV))[0]
    assert th.equal(sa, sb) and not th.equal(sa, sc)


def test_regime_b_injected_states_and_terminal_flags():
    N = 1000
    env = make_env(N)
    rng = np.random.default_rng(21)
    prev = inject(env, draw_phys(rng, N, 4.0, 8.0))
    acts = rng.integers(0, 3, N)
    state, reward, terminal, truncate, _ = env.step(th.from_numpy(acts).to(DEV))
    ref, term_ref, margin, _ = R.acrobot_step(prev, acts)
    near = np.abs(margin) < BAND
    term = terminal.cpu().numpy()
    print(f"regime B: {int(term_ref.sum())} terminal rows of {N} in fp64, {int(term.sum())} on the device; "
          f"{int(near.sum())} rows ({near.mean():.2%}) within {BAND:.0e} of the threshold")
    np.testing.assert_array_equal(term[~near], term_ref[~near])
    assert near.mean() < 0.01 and term_ref.sum() > 0 and not truncate.any()
    keep = ~term & ~term_ref
    e = obs_err(state.cpu().numpy()[keep], ref[keep])
    print(f"regime B: largest deviation from fp64: {e.max():.3e} (bound {TOL:.0e})")
    assert e.max() <= TOL
    # reward 0 exactly on the terminal rows, -1 elsewhere; a terminal row restarts
    assert th.equal(reward, th.where(terminal, 0.0, -1.0).to(th.float32))
    assert th.equal(env.episode, terminal.to(th.int32)) and th.equal(env.step_count, (~terminal).to(th.int32))
    done = env.phys[terminal]
    assert (done >= -0.1).all() and (done < 0.1).all()


def test_regime_c_full_velocity_range_is_self_calibrating():
    N = 3000          # three draws of 1000, one launch
    env = make_env(N)
    rng = np.random.default_rng(31)
    prev = inject(env, draw_phys(rng, N, R.MAX_VEL_1, R.MAX_VEL_2))
    acts = rng.integers(0, 3, N)
    state, _, terminal, _, _ = env.step(th.from_numpy(acts).to(DEV))
    got, term = state.cpu().numpy(), terminal.cpu().numpy()
    ref, term_ref, _, raw = R.acrobot_step(prev, acts)
    ref32 = R.acrobot_step(prev, acts, dtype=F32)[0]
    assert ref32.dtype == F32
    keep = ~term          # (a terminal row shows its reset state)
    e_dev, e_np = obs_err(got[keep], ref[keep]), obs_err(R.observe(ref32[keep]), ref[keep])
    ratios = (e_dev[:, :4].max() / e_np[:, :4].max(), e_dev[:, 4:].max() / e_np[:, 4:].max())
    print(f"regime C: cos / sin: device {e_dev[:, :4].max():.3e}, fp32 numpy {e_np[:, :4].max():.3e}, ratio {ratios[0]:.2f}; "
          f"velocities: device {e_dev[:, 4:].max():.3e}, fp32 numpy {e_np[:, 4:].max():.3e}, ratio {ratios[1]:.2f} (bound 8)")
    assert max(ratios) <= 8.0, ratios
    # the regime does what it is for: clipped rows, rows that take two turns off an angle, terminal rows
    over = np.abs(raw[:, 2:]) > np.array([R.MAX_VEL_1, R.MAX_VEL_2])
    twice = R.n_wraps(raw).max(axis=1) > 1
    print(f"regime C: {int(over.any(axis=1).sum())} clipped rows, {int(twice.sum())} rows wrap more than once, {int(term_ref.sum())} terminal")
    assert over.any(axis=1).sum() > 0 and twice.sum() > 0 and term_ref.sum() > 0
    assert (np.abs(got[keep][:, :4]) <= 1.0 + 1e-6).all()
    # where fp64 clips -- clear of the bound by more than this regime's fp32 error (1.7e-3 relative) -- the velocity IS the bound
    clear = np.abs(raw[:, 2:]) > 1.01 * np.array([R.MAX_VEL_1, R.MAX_VEL_2])
    bound = np.sign(raw[:, 2:]).astype(F32) * np.array([R.MAX_VEL_1, R.MAX_VEL_2]).astype(F32)
    sel = clear & keep[:, None]
    assert sel.sum() > 0
    np.testing.assert_array_equal(got[:, 4:][sel], bound[sel])
    assert (np.abs(got[keep][:, 4]) <= F32(R.MAX_VEL_1)).all() and (np.abs(got[keep][:, 5]) <= F32(R.MAX_VEL_2)).all()


def test_episode_bookkeeping_and_reset_draws():
    N, M, MAX_STEP, STEPS = 300, 130, 7, 16
    env, small, other = make_env(N, MAX_STEP), make_env(M, MAX_STEP), make_env(N, MAX_STEP, seed=6)
    small.phys.copy_(env.phys[:M])          # the same trajectories on the shared rows (reset() draws depend on num_envs; the kernel's do not)
    small.state.copy_(env.state[:M])
    rng = np.random.default_rng(41)
    sc_ref, ep_ref = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    resets, n_trunc, epoch0 = [], 0, env.state_epoch
    for t in range(STEPS):
        a = th.from_numpy(rng.integers(0, 3, N)).to(DEV)
        state, reward, terminal, truncate, _ = env.step(a)
        s2, r2, t2, u2, _ = small.step(a[:M].clone())
        other.step(a.clone())
        assert th.equal(state[:M], s2) and th.equal(env.phys[:M], small.phys) and th.equal(reward[:M], r2) and th.equal(truncate[:M], u2)
        term, trunc = terminal.cpu().numpy(), truncate.cpu().numpy()
        sc_ref += 1
        np.testing.assert_array_equal(trunc, (sc_ref >= MAX_STEP) & ~term)
        assert th.equal(reward, th.where(terminal, 0.0, -1.0).to(th.float32))
        done = term | trunc
        sc_ref[done] = 0
        ep_ref[done] += 1
        np.testing.assert_array_equal(env.step_count.cpu().numpy(), sc_ref)
        np.testing.assert_array_equal(env.episode.cpu().numpy(), ep_ref)
        if done.any():
            fresh = env.phys.cpu().numpy()[done]
            assert (fresh >= F32(-0.1)).all() and (fresh < F32(0.1)).all()
            assert obs_err(state.cpu().numpy()[done], fresh).max() < 1e-6
            assert not th.equal(env.phys, other.phys)          # another seed, other draws
            resets.append(fresh)
        n_trunc += int(trunc.sum())
    assert env.state_epoch == epoch0 + STEPS
    assert n_trunc >= 2 * N - 10          # steps 7 and 14 truncate every env that did not terminate
    resets = np.concatenate(resets)
    # the draws differ across envs, episodes and components
    assert len(np.unique(resets, axis=0)) == len(resets) and (np.diff(np.sort(resets, axis=1), axis=1) != 0).all()
    assert abs(resets.mean()) < 0.01 and 0.05 < resets.std() < 0.065
