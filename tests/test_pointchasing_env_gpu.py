"""The device-resident PointChasingVecEnv (erl_pointchasing_step_f32, csrc/pointchasing_step.h) against the numpy restatement of its step
(tests/pointchasing_ref.py, itself pinned to the reference's env by tests/test_pointchasing_golden_cpu.py), teacher-forced: every step is
compared from the kernel's own previous row, and where the kernel reset a row the comparison goes on from the row it drew.

N = 33: with 16 envs per tile of the one-launch kernels the second tile is full and the third holds one env (the per-step kernel itself is
one lane per env).  The restatement is fed the uniforms of a numpy Philox4x32-10 with the header's key layout, and in fp32 it is expected
to give the kernel's state, reward, distance, flags and counters BIT FOR BIT: every operation of the step is a correctly rounded fp32
product, sum, quotient or square root on both sides (hipcc rounds sqrtf and / correctly by default) and the header switches contraction
off.  Against the fp64 restatement of the same step from the same fp32 inputs, the fp32 step deviates by at most 4.8e-7 in a state
element and by 1.0e-6 / 1.4e-6 / 1.7e-6 / 2.3e-6 (dim 1 / 2 / 3 / 4) in the distance and in the reward over these runs (measured on an
MI355X; the test prints them): one to two ulp of values of size 8..16.

The reset draws are Box-Muller on hardware transcendentals, which numpy does not reproduce to the bit: they are checked as draws (moments
within 5 standard errors, distinct across env and episode, a function of the seed alone)."""
import numpy as np
import pytest
import torch as th

from tests import pointchasing_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 33


def _env(dim, n=N, max_step=17, seed=5):
    from elegantrl_amd.envs import PointChasingVecEnv
    env = PointChasingVecEnv(dim=dim, num_envs=n, max_step=max_step, gpu_id=0, seed=seed)
    state, _ = env.reset()
    return env, state


def _near_starts(env, dim, rng):
    """odd envs next to their target (distance dim + 0.02 on a random direction), the carried distance recomputed as reset() does"""
    s = env.state.cpu().numpy()
    direction = rng.standard_normal((env.num_envs, dim)).astype(np.float32)
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    odd = np.arange(env.num_envs) % 2 == 1
    s[odd, 2 * dim:3 * dim] = s[odd, :dim] - direction[odd] * np.float32(dim + 0.02)
    env.state.copy_(th.from_numpy(s))
    env.distance.copy_(th.from_numpy(R.distance_of(s, dim, np.float32)))


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_attributes_and_reset(dim):
    from elegantrl_amd.envs import PointChasingVecEnv
    env, state = _env(dim, n=4096)
    assert (env.env_name, env.num_envs, env.max_step, env.state_dim, env.action_dim, env.if_discrete) == \
        ("PointChasingVecEnv", 4096, 17, 4 * dim, dim, False)
    assert PointChasingVecEnv().dim == 2 and PointChasingVecEnv().max_step == 1024
    assert state.shape == (4096, 4 * dim) and state.dtype == th.float32 and state.data_ptr() != env.state.data_ptr()
    s = state.cpu().numpy()
    p0, v0, p1, v1 = R.split(s, dim)
    se, se_std = 1 / np.sqrt(4096 * dim), 1 / np.sqrt(2 * 4096 * dim)
    assert abs(p0.mean()) < 5 * se and abs(p1.mean() + 8) < 5 * se and abs(p0.std() - 1) < 5 * se_std and abs(p1.std() - 1) < 5 * se_std
    assert not v0.any() and not v1.any()
    assert np.array_equal(env.distance.cpu().numpy().view(np.uint32), R.distance_of(s, dim, np.float32).view(np.uint32))
    assert not env.step_count.any() and not env.episode.any()
    again = PointChasingVecEnv(dim=dim, num_envs=4096, max_step=17, gpu_id=0, seed=5).reset()[0]
    other = PointChasingVecEnv(dim=dim, num_envs=4096, max_step=17, gpu_id=0, seed=6).reset()[0]
    assert th.equal(again, state) and not th.equal(other, state)


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_forty_steps_are_the_fp32_restatement_bit_for_bit(dim):
    env, _ = _env(dim)
    rng = np.random.default_rng(40 + dim)
    _near_starts(env, dim, rng)
    bits = lambda x: np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)      # noqa: E731
    worst64 = np.zeros(3)
    n_caught = n_timeout = 0
    below = above = False
    for t in range(40):
        s, dist = env.state.cpu().numpy(), env.distance.cpu().numpy()
        sc, ep = env.step_count.cpu().numpy(), env.episode.cpu().numpy()
        chase = R.chase_action(s, dim)
        unit = chase / np.linalg.norm(chase, axis=1, keepdims=True)
        act = ((unit + 0.3 * rng.standard_normal((N, dim))) * (3.0 if t % 2 == 0 else 0.3)).astype(np.float32)
        u = R.step_uniforms(env.seed, np.arange(N), ep, sc, dim)
        assert (u >= 0).all() and (u < 1).all()
        new, reward, d, l2, caught = R.pointchasing_step(s, act, u, dist, dim, np.float32)
        new64, reward64, d64, _, _ = R.pointchasing_step(s, act, u, dist, dim, np.float64)
        timeout = (sc + 1 >= env.max_step) & ~caught
        done = caught | timeout
        assert np.abs(d.astype(np.float64) - dim).min() > 1e-5, "a flag of this run would hinge on one rounding"
        below, above = below or bool((l2 == 1).any()), above or bool((l2 > 1).any())

        got_s, got_r, got_te, got_tr, _ = env.step(th.from_numpy(act).to(DEV))
        got_s, got_r = got_s.cpu().numpy(), got_r.cpu().numpy()
        assert th.equal(got_te.cpu(), th.from_numpy(caught)) and th.equal(got_tr.cpu(), th.from_numpy(timeout)), (dim, t)
        assert np.array_equal(bits(got_s[~done]), bits(new[~done])), (dim, t, "state")
        assert np.array_equal(bits(got_r), bits(reward)), (dim, t, "reward")
        # the carried distance: d where the episode goes on, that of the drawn row where it was reset (D1)
        want_dist = R.carried_distance(d, got_s, done, dim, np.float32)
        assert np.array_equal(bits(env.distance.cpu().numpy()), bits(want_dist)), (dim, t, "distance")
        assert np.array_equal(env.step_count.cpu().numpy(), np.where(done, 0, sc + 1)), (dim, t)
        assert np.array_equal(env.episode.cpu().numpy(), ep + done), (dim, t)
        # a reset row: velocities exactly 0, positions drawn around 0 and -8
        r0, rv0, r1, rv1 = R.split(got_s[done], dim)
        assert not rv0.any() and not rv1.any() and (np.abs(r0) < 6).all() and (np.abs(r1 + 8) < 6).all()
        assert th.equal(env.state.cpu(), th.from_numpy(got_s))
        worst64 = np.maximum(worst64, [np.abs(new - new64).max(), np.abs(d - d64).max(), np.abs(reward - reward64).max()])
        n_caught, n_timeout = n_caught + int(caught.sum()), n_timeout + int(timeout.sum())
    print(f"dim {dim}: {n_caught} catches, {n_timeout} time-outs; fp32 step against fp64: state {worst64[0]:.3g} d {worst64[1]:.3g} "
          f"reward {worst64[2]:.3g}")
    assert n_caught >= 8 and n_timeout >= 2 * 17 and below and above


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_reset_draws(dim):
    """max_step = 1: every step resets every env.  Four steps of 4096 envs"""
    n = 4096
    runs = {}
    for name, seed in (("a", 5), ("same", 5), ("other", 6)):
        env, _ = _env(dim, n=n, max_step=1, seed=seed)
        rows = []
        act = th.zeros((n, dim), device=DEV)
        for t in range(4):
            s, _, te, tr, _ = env.step(act)
            assert bool((te | tr).all()) and bool((env.step_count == 0).all()) and bool((env.episode == t + 1).all())
            rows.append(s.cpu().numpy())
        runs[name] = np.stack(rows)                                            # (4, n, 4 dim)
    a = runs["a"]
    p0, v0, p1, v1 = R.split(a.reshape(-1, 4 * dim), dim)
    assert not v0.any() and not v1.any()
    count = p0.size
    se_mean, se_std = 1 / np.sqrt(count), 1 / np.sqrt(2 * count)
    for name, x in (("p0", p0.astype(np.float64)), ("p1 + 8", p1.astype(np.float64) + 8)):
        print(f"dim {dim} {name}: mean {x.mean():+.5f} (5 se = {5 * se_mean:.5f}), std {x.std():.5f} (1 +- {5 * se_std:.5f})")
        assert abs(x.mean()) < 5 * se_mean and abs(x.std() - 1) < 5 * se_std, name
    # distinct across env and episode (and p0 is not p1's draw): every drawn number of the run is its own
    drawn = np.concatenate((p0.ravel(), (p1 + np.float32(8)).ravel()))
    assert len(np.unique(drawn)) > 0.99 * drawn.size                      # (fp32 values of a 24-bit draw: a few hundred coincide by chance)
    assert len(np.unique(a.reshape(4 * n, -1), axis=0)) == 4 * n
    # a function of the seed alone
    assert np.array_equal(runs["same"], a) and not np.array_equal(runs["other"], a)
    assert (runs["other"] != a)[:, :, :dim].mean() > 0.99


def test_recovered_uniforms_are_in_the_half_open_unit_interval():
    """from rest (v0 = 0 after reset()) the new v0 = 0 * 0.5 + u IS the step's uniform: in [0, 1), and the numpy Philox's to the bit"""
    dim, n = 4, 4096
    env, _ = _env(dim, n=n, max_step=100, seed=11)
    for t in range(2):
        env.state[:, dim:2 * dim] = 0.0
        sc, ep = env.step_count.cpu().numpy(), env.episode.cpu().numpy()
        s, *_ = env.step(th.zeros((n, dim), device=DEV))
        u = s[:, dim:2 * dim].cpu().numpy()
        assert (u >= 0).all() and (u < 1).all() and 0.49 < u.mean() < 0.51
        assert np.array_equal(u.view(np.uint32), R.step_uniforms(11, np.arange(n), ep, sc, dim).view(np.uint32))
        assert len(np.unique(u)) > 0.99 * u.size


def test_step_entry_refuses_bad_shapes_on_device_tensors():
    from elegantrl_amd import ops
    env, _ = _env(2)
    bad_action = th.zeros((N, 3), device=DEV)
    with pytest.raises(Exception, match="erl_pointchasing_step_f32: bad shape"):
        ops.pointchasing_step(env.state, bad_action, env.distance, env.step_count, env.episode, env._reward, env._terminal, env._truncate, 17, 5)
