"""tests/pointchasing_ref.py (the numpy restatement the GPU tests compare the device env with) against what the reference's
PointChasingVecEnv computed on the CPU (tests/golden/pointchasing_run.npz, tools/record_pointchasing_golden.py): dim 1..4, 33 envs, 48
steps, max_step 17, 16 catches and 66 time-outs per dim.  One step at a time, from the golden's own previous state, distances, actions
and logged uniforms.

The bound is 2 ulp (np.spacing of max(|x|, 1); for the reward of max(d_old, d_new, 1)) and is derived, not measured: the restatement
repeats the reference's fp32 operations one for one, and the only operation that is not correctly rounded on either side is torch's CPU
sqrt, which can differ from numpy's by 1 ulp.  One ulp of l2 reaches a = a / l2 (|a| <= 1), through it v1 (1 ulp of a value of size <= 4)
and p1 (0.01 of that: far below its spacing); one ulp of d reaches the reward once.  A second ulp is allowed for the rounding of the
operation that carries the first one on.  Flags are compared exactly, nothing excluded: the recorder asserts that no |d - dim| is closer
than 1e-6."""
import os

import numpy as np
import pytest

from tests import pointchasing_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pointchasing_run.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def ulps(got, want, scale):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(scale), 1).astype(np.float32))


def replay(g, dim, stale_distance):
    """every step of the golden through the fp32 restatement -> per step (new state, reward, d, caught), the carried distance being the
    golden's own (stale over a reset) or the one recomputed from the golden's post-reset state"""
    k = f"d{dim}_"
    states, dist, acts, us, term = g[k + "states"], g[k + "distances"], g[k + "actions"], g[k + "uniforms"], g[k + "terminal"]
    out, carried = [], dist[0]
    for t in range(len(acts)):
        new, reward, d, l2, caught = R.pointchasing_step(states[t], acts[t], us[t], carried, dim, np.float32)
        out.append((new, reward, d, caught))
        carried = R.carried_distance(dist[t + 1], states[t + 1], term[t], dim, np.float32, stale_distance=stale_distance)
    return out


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_restatement_is_the_reference_step(golden, dim):
    g, k = golden, f"d{dim}_"
    states, dist, term, cur = g[k + "states"], g[k + "distances"], g[k + "terminal"], g[k + "cur_steps"]
    rewards, max_step = g[k + "rewards"], int(g["max_step"])
    worst = np.zeros(3)
    n_caught = n_timeout = 0
    for t, (new, reward, d, caught) in enumerate(replay(g, dim, stale_distance=True)):
        timeout = (cur[t] + 1 >= max_step) & ~caught
        assert np.array_equal(term[t], caught | timeout), (dim, t)                  # the reference's one flag, exactly
        n_caught, n_timeout = n_caught + int(caught.sum()), n_timeout + int(timeout.sum())
        live = ~term[t]                                                              # done rows return the reference's reset draws
        worst[0] = max(worst[0], ulps(new[live], states[t + 1][live], states[t + 1][live]).max())
        worst[1] = max(worst[1], ulps(d, dist[t + 1], dist[t + 1]).max())            # (the reference keeps the pre-reset d)
        worst[2] = max(worst[2], ulps(reward, rewards[t], np.maximum(dist[t], dist[t + 1])).max())
        done = term[t]
        reset = np.concatenate((g[k + "reset_p0"][t], np.zeros_like(new[:, :dim]), g[k + "reset_p1"][t], np.zeros_like(new[:, :dim])), axis=1)
        assert np.array_equal(states[t + 1][done], reset[done])
    print(f"dim {dim}: max ulp state {worst[0]:.2f} d {worst[1]:.2f} reward {worst[2]:.2f}; {n_caught} catches, {n_timeout} time-outs")
    assert n_caught >= 8 and n_timeout >= 33
    assert worst.max() <= 2.0, worst


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_recomputed_distance_differs_in_the_first_reward_after_a_reset_only(golden, dim):
    """deviation D1: with the distance recomputed after a reset, the rewards that differ from the reference's are exactly those of the first
    step after each reset (there the reference's reward carries the stale pre-reset d: after a catch it is off by about 8 sqrt(dim) - dim)"""
    g, k = golden, f"d{dim}_"
    dist, term, rewards = g[k + "distances"], g[k + "terminal"], g[k + "rewards"]
    differs = np.zeros_like(term)
    for t, (new, reward, d, caught) in enumerate(replay(g, dim, stale_distance=False)):
        differs[t] = ulps(reward, rewards[t], np.maximum(dist[t], dist[t + 1])) > 2.0
        if t > 0:
            fresh = term[t - 1]
            assert np.all(np.abs(reward[fresh] - rewards[t][fresh]) > 1e-2)          # not a rounding matter (2 ulp of a distance is 2e-6)
    expected = np.zeros_like(term)
    expected[1:] = term[:-1]
    assert expected.sum() >= 60
    assert np.array_equal(differs, expected)


def test_numpy_philox_known_answers():
    """Philox4x32-10's published known-answer vectors (Random123 kat_vectors)"""
    assert [int(x[0]) for x in R.philox4x32_10([0], 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ff = 0xffffffff
    assert [int(x[0]) for x in R.philox4x32_10([ff], ff, ff, ff, ff, ff)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert [int(x[0]) for x in R.philox4x32_10([0x243f6a88], 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)] == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    u = R.step_uniforms(12345, np.arange(1000), np.arange(1000) % 7, np.arange(1000) % 17, 4)
    assert u.dtype == np.float32 and u.shape == (1000, 4) and (u >= 0).all() and (u < 1).all() and abs(u.mean() - 0.5) < 0.03
