"""numpy restatement of one Acrobot-v1 step (gymnasium's "book" dynamics, restated from the task's specification, not checked against the
package): fp64 by default, the reference of the tests of the device-resident Acrobot env and of the one-launch discrete rollout on it;
with dtype=np.float32 every operation runs in fp32, which says how much of a deviation from fp64 is the number format's own.  No pytest
import: tools may load it outside a test run."""
import numpy as np

M1 = M2 = 1.0
L1 = 1.0
LC1 = LC2 = 0.5
I1 = I2 = 1.0
G, DT = 9.8, 0.2
MAX_VEL_1, MAX_VEL_2 = 4 * np.pi, 9 * np.pi


def _dsdt(s, a, f):
    th1, th2, w1, w2 = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    c2, s2 = np.cos(th2), np.sin(th2)
    d1 = f(M1 * LC1 ** 2) + f(M2) * (f(L1 ** 2 + LC2 ** 2) + f(2 * L1 * LC2) * c2) + f(I1 + I2)
    d2 = f(M2) * (f(LC2 ** 2) + f(L1 * LC2) * c2) + f(I2)
    phi2 = f(M2 * LC2 * G) * np.cos(th1 + th2 - f(np.pi / 2))
    phi1 = (-f(M2 * L1 * LC2) * w2 * w2 * s2 - f(2 * M2 * L1 * LC2) * w2 * w1 * s2
            + f((M1 * LC1 + M2 * L1) * G) * np.cos(th1 - f(np.pi / 2)) + phi2)
    acc2 = (a + d2 / d1 * phi1 - f(M2 * L1 * LC2) * w1 * w1 * s2 - phi2) / (f(M2 * LC2 ** 2 + I2) - d2 * d2 / d1)
    acc1 = -(d2 * acc2 + phi1) / d1
    return np.stack((w1, w2, acc1, acc2), axis=1)


def wrap(x, f=np.float64):
    """into [-pi, pi] by whole turns, one at a time (gymnasium's wrap)"""
    x = x.copy()
    pi, two_pi = f(np.pi), f(2 * np.pi)
    while (x > pi).any():
        x[x > pi] -= two_pi
    while (x < -pi).any():
        x[x < -pi] += two_pi
    return x


def observe(phys):
    """(cos theta1, sin theta1, cos theta2, sin theta2, omega1, omega2) of phys (N, 4), in phys's dtype"""
    return np.stack((np.cos(phys[:, 0]), np.sin(phys[:, 0]), np.cos(phys[:, 1]), np.sin(phys[:, 1]), phys[:, 2], phys[:, 3]), axis=1)


def acrobot_step(phys, action, dtype=np.float64):
    """phys (N, 4) = (theta1, theta2, omega1, omega2), action (N,): 0 / 1 / 2 is torque -1 / 0 / +1, anything else torque 0 ->
    (next phys before any reset (N, 4), terminal (N,), margin (N,) = -cos theta1' - cos(theta1' + theta2') - 1: a row whose margin is
    within rounding of zero may legitimately get either flag, raw (N, 4): the RK4 result before the wrap and the clip)"""
    f = dtype
    s = np.asarray(phys).astype(f)
    action = np.asarray(action)
    a = np.where(action == 0, -1.0, np.where(action == 2, 1.0, 0.0)).astype(f)
    k1 = _dsdt(s, a, f)
    k2 = _dsdt(s + f(DT / 2) * k1, a, f)
    k3 = _dsdt(s + f(DT / 2) * k2, a, f)
    k4 = _dsdt(s + f(DT) * k3, a, f)
    raw = s + f(DT / 6) * (k1 + f(2) * k2 + f(2) * k3 + k4)
    assert raw.dtype == f
    new = np.stack((wrap(raw[:, 0], f), wrap(raw[:, 1], f), np.clip(raw[:, 2], f(-MAX_VEL_1), f(MAX_VEL_1)),
                    np.clip(raw[:, 3], f(-MAX_VEL_2), f(MAX_VEL_2))), axis=1)
    margin = -np.cos(new[:, 0]) - np.cos(new[:, 0] + new[:, 1]) - f(1)
    return new, margin > 0, margin, raw


def n_wraps(raw):
    """how many whole turns the wrap takes off each angle of raw (N, 4) -> (N, 2) int"""
    return np.ceil((np.abs(raw[:, :2].astype(np.float64)) - np.pi) / (2 * np.pi)).clip(min=0).astype(np.int64)
