"""fp64 numpy restatement of one CartPole-v1 step (gymnasium's physics as CartPoleVecEnv.step states them), shared by the tests of the
device-resident CartPole env and of the one-launch discrete rollout.  No pytest import: tools may load it outside a test run."""
import math

import numpy as np

X_LIMIT, THETA_LIMIT = 2.4, 12 * 2 * math.pi / 360


def cartpole_step_f64(state, action):
    """state (N, 4) fp64, action (N,) -> (next state before any reset (N, 4), terminal (N,), margins (N, 2) = (|x'| - 2.4,
    |theta'| - 12 degrees): a row whose margin is within rounding of zero may legitimately get either flag)"""
    x, x_dot, theta, theta_dot = (state[:, i].astype(np.float64) for i in range(4))
    force = np.where(np.asarray(action) == 1, 10.0, -10.0)
    cos, sin = np.cos(theta), np.sin(theta)
    temp = (force + 0.05 * theta_dot * theta_dot * sin) / 1.1
    theta_acc = (9.8 * sin - cos * temp) / (0.5 * (4.0 / 3.0 - 0.1 * cos * cos / 1.1))
    x_acc = temp - 0.05 * theta_acc * cos / 1.1
    new = np.stack((x + 0.02 * x_dot, x_dot + 0.02 * x_acc, theta + 0.02 * theta_dot, theta_dot + 0.02 * theta_acc), axis=1)
    margins = np.stack((np.abs(new[:, 0]) - X_LIMIT, np.abs(new[:, 2]) - THETA_LIMIT), axis=1)
    return new, (margins > 0).any(axis=1), margins
