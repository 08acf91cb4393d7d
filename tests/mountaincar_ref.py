"""numpy restatement of one MountainCar-v0 step (gymnasium's dynamics, restated from the task's specification, not checked against the
package): fp64 by default, the reference of the tests of the device-resident MountainCar env and of the one-launch discrete rollout on
it; with dtype=np.float32 every operation runs in fp32, which says how much of a deviation from fp64 is the number format's own.  No
pytest import: tools may load it outside a test run."""
import numpy as np

FORCE, GRAVITY = 0.001, 0.0025
MAX_SPEED = 0.07
MIN_POS, MAX_POS = -1.2, 0.6
GOAL_POS, GOAL_VEL = 0.5, 0.0
RESET_LO, RESET_HI = -0.6, -0.4


def mountaincar_step(state, action, dtype=np.float64):
    """state (N, 2) = (position, velocity), action (N,): 0 / 1 / 2 pushes left / nowhere / right, anything else nowhere ->
    (next state before any reset (N, 2), terminal (N,), margin (N,) = position' - 0.5: where velocity' >= 0 a row whose margin is within
    rounding of zero may legitimately get either flag)"""
    f = dtype
    s = np.asarray(state).astype(f)
    action = np.asarray(action)
    push = np.where(action == 0, -1.0, np.where(action == 2, 1.0, 0.0)).astype(f)
    pos, vel = s[:, 0], s[:, 1]
    vel = vel + (push * f(FORCE) + np.cos(f(3) * pos) * f(-GRAVITY))
    vel = np.clip(vel, f(-MAX_SPEED), f(MAX_SPEED))
    pos = pos + vel
    pos = np.clip(pos, f(MIN_POS), f(MAX_POS))
    vel = np.where((pos == f(MIN_POS)) & (vel < 0), f(0), vel)
    new = np.stack((pos, vel), axis=1)
    assert new.dtype == f
    margin = pos - f(GOAL_POS)
    return new, (pos >= f(GOAL_POS)) & (vel >= f(GOAL_VEL)), margin


def sign_policy(state):
    """push right while the velocity is not negative, left otherwise: the policy that swings the car up"""
    return np.where(np.asarray(state)[:, 1] >= 0, 2, 0)


def first_terminal_steps(start, horizon, dtype=np.float64, policy=sign_policy):
    """the 1-based step at which each row of start (N, 2) first terminates under `policy` within `horizon` steps (0: never), no resets"""
    s = np.asarray(start).astype(dtype)
    first = np.zeros(len(s), dtype=np.int64)
    for t in range(1, horizon + 1):
        s, term, _ = mountaincar_step(s, policy(s), dtype)
        first[(first == 0) & term] = t
    return first
