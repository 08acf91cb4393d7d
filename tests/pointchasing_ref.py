"""numpy restatement of one PointChasingVecEnv step, written from the task's specification (not from the package, not from the reference's
text): fp64 by default; with dtype=np.float32 every product, sum, quotient and square root is rounded to fp32 on its own (numpy never
fuses a multiply into an add, and its sqrt and divide are correctly rounded), which is what the device step is expected to give bit for
bit.  Also a numpy Philox4x32-10 with the key layout of csrc/pointchasing_step.h, so that a test can feed the restatement the very
uniforms the device draws.  No pytest import: tools may load it outside a test run."""
import numpy as np

INIT_DISTANCE = 8.0
UNIFORM_TAG = 0x50434853          # second counter word of the per-step uniform call (csrc/pointchasing_step.h kPointChasingUniformTag)


def split(state, dim):
    """state (N, 4 dim) -> p0, v0, p1, v1, each (N, dim)"""
    s = np.asarray(state)
    return s[:, :dim], s[:, dim:2 * dim], s[:, 2 * dim:3 * dim], s[:, 3 * dim:]


def ordered_sum(x):
    """sum over axis 1 in index order, every partial sum rounded to x's dtype"""
    acc = x[:, 0].copy()
    for k in range(1, x.shape[1]):
        acc = acc + x[:, k]
    return acc


def distance_of(state, dim, dtype=np.float64):
    p0, _, p1, _ = split(np.asarray(state).astype(dtype), dim)
    return np.sqrt(ordered_sum((p0 - p1) ** 2))


def pointchasing_step(state, action, u, distance, dim, dtype=np.float64):
    """state (N, 4 dim), action (N, dim), u (N, dim) the step's uniforms, distance (N,) the carried |p0 - p1| (`carried_distance`) ->
    (new state before any reset (N, 4 dim), reward (N,), d (N,), l2 (N,), caught (N,))"""
    f = dtype
    p0, v0, p1, v1 = (x.astype(f) for x in split(state, dim))
    a = np.asarray(action).astype(f)
    u = np.asarray(u).astype(f)
    l2 = np.maximum(np.sqrt(ordered_sum(a * a)), f(1))
    a = a / l2[:, None]
    v1 = v1 * f(0.75) + a
    p1 = p1 + v1 * f(0.01)
    v0 = v0 * f(0.5) + u
    p0 = p0 + v0 * f(0.01)
    diff = p0 - p1
    d = np.sqrt(ordered_sum(diff * diff))
    reward = np.asarray(distance).astype(f) - d - l2 * f(0.02)
    new = np.concatenate((p0, v0, p1, v1), axis=1)
    assert new.dtype == f and reward.dtype == f and d.dtype == f
    return new, reward, d, l2, d < f(dim)


def carried_distance(d, post_reset_state, done, dim, dtype=np.float64, stale_distance=False):
    """the distance an env carries into its next step: d where the episode goes on; where it was reset, the distance of the state it
    was reset to -- or, with `stale_distance` (the reference's vec env, which never recomputes it; used against the golden only), still d"""
    if stale_distance:
        return np.asarray(d).astype(dtype)
    return np.where(done, distance_of(post_reset_state, dim, dtype), np.asarray(d).astype(dtype)).astype(dtype)


# ---- Philox4x32-10 ----------------------------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """counter words c0..c3 and key words k0, k1 (arrays or ints, broadcast together) -> four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        prod0, prod1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        hi0, lo0, hi1, lo1 = prod0 >> np.uint64(32), prod0 & _MASK, prod1 >> np.uint64(32), prod1 & _MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return [x.astype(np.uint32) for x in c]


def step_uniforms(seed, env, episode, step, dim):
    """the (N, dim) fp32 uniforms of one step: ONE call per env, counter (env, UNIFORM_TAG, episode, step-in-episode), key = the 64-bit
    seed's halves; u_k = (word_k >> 8) * 2^-24, in [0, 1)"""
    seed = int(seed) & (2 ** 64 - 1)
    words = philox4x32_10(np.asarray(env), UNIFORM_TAG, np.asarray(episode), np.asarray(step), seed & 0xFFFFFFFF, seed >> 32)
    u = np.stack([(w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) for w in words[:dim]], axis=1)
    return u


def chase_action(state, dim):
    """the reference's heuristic: head for the target"""
    p0, _, p1, _ = split(state, dim)
    return p0 - p1
