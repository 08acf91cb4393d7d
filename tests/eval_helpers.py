"""Shared by the evaluation tests (tests/test_eval_fused_gpu.py) and the evaluation benchmark (tools/eval_bench.py): the seeded PPO agent +
env pair, the numpy oracle that cuts a rollout's planes into the evaluator's episode table, and the measurement of the gap between the
Evaluator's step loop and the zero-noise training rollout.  No pytest import: the benchmark loads it outside a test run."""
import numpy as np
import torch as th

DEV = "cuda:0"


def make_ppo(kind, N, S, A, net, max_step, seed=3, head_scale=1.0, gae_exact=False):
    """as tests/test_rollout_fused_gpu.py::_make (fused rollout on, reward_scale 1); head_scale multiplies the actor's last layer"""
    from elegantrl_amd.agents import AgentPPO
    from elegantrl_amd.envs import PendulumVecEnv, SynVecEnv
    from elegantrl_amd.train import Config
    args = Config(AgentPPO, None, {"env_name": kind, "num_envs": N, "max_step": max_step, "state_dim": S, "action_dim": A,
                                   "if_discrete": False})
    args.net_dims, args.reward_scale, args.random_seed, args.learning_rate = list(net), 1.0, 7, 1e-3
    args.fused_rollout = True
    if gae_exact:
        args.gae_algo = "exact"
    th.manual_seed(seed)
    agent = AgentPPO(args.net_dims, S, A, gpu_id=0, args=args)
    with th.no_grad():
        g = th.Generator(device=DEV).manual_seed(seed + 1)
        agent.act.state_avg[:] = 0.1 * th.randn(S, device=DEV, generator=g)
        agent.act.state_std[:] = 1.0 + 0.2 * th.rand(S, device=DEV, generator=g)
        agent.cri.state_avg[:] = 0.1 * th.randn(S, device=DEV, generator=g)
        agent.cri.state_std[:] = 1.0 + 0.2 * th.rand(S, device=DEV, generator=g)
        agent.act.action_std_log[:] = -0.3 + 0.1 * th.randn(A, device=DEV, generator=g)
        if head_scale != 1.0:
            agent.act.net[4].weight.mul_(head_scale)
    env = PendulumVecEnv(N, max_step=max_step, gpu_id=0, seed=5) if kind == "pendulum" else SynVecEnv(N, S, A, max_step=max_step, gpu_id=0, seed=5)
    agent.last_state = env.reset()[0]
    return agent, env, args


def oracle_table(rewards, undones, unmasks):
    """the evaluator's table from a rollout's planes: env-major, time order; return = float32 of the SEQUENTIAL fp64 sum of the episode's
    fp32 rewards (np.sum adds pairwise: another order), length = its steps; an episode still open at the end is dropped"""
    r = rewards.detach().cpu().numpy().astype(np.float32)
    done = ~(undones.cpu().numpy().astype(bool) & unmasks.cpu().numpy().astype(bool))
    H, N = r.shape
    rows = []
    for i in range(N):
        acc, n = np.float64(0.0), 0
        col, dcol = r[:, i], done[:, i]
        for t in range(H):
            acc = acc + np.float64(col[t])
            n += 1
            if dcol[t]:
                rows.append((np.float32(acc), np.float32(n)))
                acc, n = np.float64(0.0), 0
    return np.array(rows, dtype=np.float32).reshape(-1, 2)


def loop_vs_exact_gap(seed):
    """(max per-episode |return difference|, |difference of the mean return|, lengths all 200 on both sides) between the Evaluator's
    loop and the zero-noise kernel rollout cut by the oracle: Pendulum, 256 envs, max_step 200, net (128, 64).  Runs on the code
    before the fused evaluation as well (it uses nothing of it)."""
    from elegantrl_amd.train.evaluator import get_cumulative_rewards_and_step_from_vec_env
    agent, env, _ = make_ppo("pendulum", 256, 3, 1, (128, 64), 200, seed=seed)
    loop = get_cumulative_rewards_and_step_from_vec_env(env, agent.act).numpy()
    agent.last_state = env.reset()[0]
    items = agent._explore_vec_env(env, 200, noise=th.zeros((200, 256, 1), device=DEV))
    exact = oracle_table(items[3], items[4], items[5])
    assert loop.shape == exact.shape == (256, 2)
    return (float(np.abs(loop[:, 0] - exact[:, 0]).max()), float(abs(loop[:, 0].mean() - exact[:, 0].mean())),
            bool((loop[:, 1] == 200).all() and (exact[:, 1] == 200).all()))
