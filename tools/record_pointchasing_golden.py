"""Record tests/golden/pointchasing_run.npz by RUNNING the reference's PointChasingVecEnv on the CPU (sim_gpu_id=-1).

    python tools/record_pointchasing_golden.py --reference <checkout of the reference>     (or ERL_REFERENCE=<checkout>)

Nothing of the reference is copied: only what its env computes on our inputs is stored.  torch.rand and torch.normal are wrapped inside
this process, so every draw the env makes is logged beside what it returns -- tests/test_pointchasing_golden_cpu.py replays the steps
with tests/pointchasing_ref.py from exactly those numbers.

Per dim in 1..4: 33 envs, 48 steps, max_step 17.  Odd envs are moved to distance dim + 0.02 from their target on a random direction
before the first step, so that they catch it within a few steps; every env then runs into the time limit twice.  The action is the
reference's chase heuristic as a unit vector plus 0.3 N(0,1) noise, scaled 3.0 on even steps and 0.3 on odd ones: both sides of the
max(|a|, 1) clamp occur.  The recorder asserts that no |d - dim| is closer than 1e-6 (a flag then cannot hinge on one rounding) and that
catches, time limits and both clamp sides are all present."""
import argparse
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, N, T, MAX_STEP, SEED = (1, 2, 3, 4), 33, 48, 17, 20240
NEAR_MARGIN = 0.02


def record(dim: int, PointChasingVecEnv):
    th.manual_seed(SEED + dim)
    rng = np.random.default_rng(SEED + 100 + dim)
    env = PointChasingVecEnv(dim=dim, env_num=N, sim_gpu_id=-1)
    env.max_step = MAX_STEP
    env.reset()
    # odd envs next to their target (the env's own expression recomputes the distances it carries)
    direction = rng.standard_normal((N, dim)).astype(np.float32)
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    odd = np.arange(N) % 2 == 1
    p1s = env.p1s.numpy().copy()
    p1s[odd] = env.p0s.numpy()[odd] - direction[odd] * np.float32(dim + NEAR_MARGIN)
    env.p1s = th.from_numpy(p1s)
    env.distances = ((env.p0s - env.p1s) ** 2).sum(dim=1) ** 0.5

    log = {"rand": [], "normal": []}
    real_rand, real_normal = th.rand, th.normal

    def rand(*a, **k):
        out = real_rand(*a, **k)
        log["rand"].append(out.numpy().copy())
        return out

    def normal(*a, **k):
        out = real_normal(*a, **k)
        log["normal"].append(out.numpy().copy())
        return out

    states = np.zeros((T + 1, N, 4 * dim), np.float32)
    distances = np.zeros((T + 1, N), np.float32)
    cur_steps = np.zeros((T + 1, N), np.int32)
    actions, uniforms = np.zeros((T, N, dim), np.float32), np.zeros((T, N, dim), np.float32)
    rewards, terminal = np.zeros((T, N), np.float32), np.zeros((T, N), bool)
    reset_p0, reset_p1 = np.full((T, N, dim), np.nan, np.float32), np.full((T, N, dim), np.nan, np.float32)
    states[0], distances[0], cur_steps[0] = env.get_state().numpy(), env.distances.numpy(), env.cur_steps.numpy()
    th.rand, th.normal = rand, normal
    try:
        for t in range(T):
            chase = PointChasingVecEnv.get_action(th.from_numpy(states[t])).numpy()
            unit = chase / np.linalg.norm(chase, axis=1, keepdims=True)
            act = ((unit + 0.3 * rng.standard_normal((N, dim))) * (3.0 if t % 2 == 0 else 0.3)).astype(np.float32)
            log["rand"].clear()
            log["normal"].clear()
            s, r, term, trunc, _ = env.step(th.from_numpy(act))
            assert len(log["rand"]) == 1 and not bool(trunc.any())
            actions[t], uniforms[t], rewards[t], terminal[t] = act, log["rand"][0], r.numpy(), term.numpy() > 0.5
            hit = np.flatnonzero(terminal[t])                        # the env resets done rows in index order: two draws each
            assert len(log["normal"]) == 2 * len(hit)
            for j, i in enumerate(hit):
                reset_p0[t, i], reset_p1[t, i] = log["normal"][2 * j], log["normal"][2 * j + 1]
            states[t + 1], distances[t + 1], cur_steps[t + 1] = s.numpy(), env.distances.numpy(), env.cur_steps.numpy()
    finally:
        th.rand, th.normal = real_rand, real_normal

    caught = distances[1:] < dim
    timeout = (cur_steps[:-1] + 1 == MAX_STEP) & ~caught
    nearest = float(np.abs(distances[1:].astype(np.float64) - dim).min())
    l2 = np.sqrt((actions.astype(np.float64) ** 2).sum(axis=2))
    assert nearest >= 1e-6, (dim, nearest)
    assert caught.sum() >= 8 and timeout.sum() >= N and (l2 < 0.9).any() and (l2 > 1.1).any(), (dim, caught.sum(), timeout.sum())
    assert np.abs(l2 - 1).min() > 1e-4
    print(f"dim {dim}: {int(caught.sum())} catches, {int(timeout.sum())} time-outs, nearest |d - dim| = {nearest:.2e}")
    return {"states": states, "distances": distances, "cur_steps": cur_steps, "actions": actions, "uniforms": uniforms, "rewards": rewards,
            "terminal": terminal, "reset_p0": reset_p0, "reset_p1": reset_p1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("ERL_REFERENCE"), help="a checkout of the reference (or ERL_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pointchasing_run.npz"))
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or ERL_REFERENCE) is needed: the golden is what the reference computes")
    sys.path.insert(0, args.reference)
    from elegantrl.envs.PointChasingEnv import PointChasingVecEnv
    assert os.path.abspath(sys.modules[PointChasingVecEnv.__module__].__file__).startswith(os.path.abspath(args.reference))
    out = {"max_step": np.int32(MAX_STEP), "dims": np.array(DIMS, np.int32)}
    for dim in DIMS:
        for k, v in record(dim, PointChasingVecEnv).items():
            out[f"d{dim}_{k}"] = v
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
