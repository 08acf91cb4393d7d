"""The skipped copy-back of the one-launch rollouts (AgentBase._hand_state_to_env / _record_last_state) on the device, for every agent /
env pair that has it: a second rollout that trusts the token (the env's live buffer still holds the agent's last state) and one that was
made to copy the last state back first (its token dropped and the live buffer written over, so a copy skipped by mistake shows) must
leave the same bits everywhere.  N = 40: two full 16-env tiles and a partial one."""
import pytest
import torch as th

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, H, NET, MAX_STEP = 40, 3, (64, 32), 4         # max_step < 2 H: truncations and resets inside the two rollouts


def _config(cls, name, S, A, discrete):
    from elegantrl_amd.train import Config
    args = Config(cls, None, {"env_name": name, "num_envs": N, "max_step": MAX_STEP, "state_dim": S, "action_dim": A, "if_discrete": discrete})
    args.net_dims, args.random_seed, args.reward_scale, args.quiet = list(NET), 7, 0.5, True
    args.fused_rollout = True                               # (off by default on the discrete agents)
    return args


def _ppo_syn():
    from elegantrl_amd.agents import AgentPPO
    from elegantrl_amd.envs import SynVecEnv
    S, A = 17, 3
    th.manual_seed(3)
    agent = AgentPPO(list(NET), S, A, gpu_id=0, args=_config(AgentPPO, "SynVecEnv", S, A, False))
    env = SynVecEnv(N, S, A, max_step=MAX_STEP, gpu_id=0, seed=5)
    return agent, env, "fused_rollout", (H, N, A), th.randn


def _discrete(env_cls, name, S, A):
    from elegantrl_amd.agents import AgentDiscretePPO
    th.manual_seed(3)
    agent = AgentDiscretePPO(list(NET), S, A, gpu_id=0, args=_config(AgentDiscretePPO, name, S, A, True))
    env = env_cls(N, max_step=MAX_STEP, gpu_id=0, seed=5)
    return agent, env, "fused_rollout_discrete", (H, N), th.rand


def _discrete_cartpole():
    from elegantrl_amd.envs import CartPoleGpuVecEnv
    return _discrete(CartPoleGpuVecEnv, "CartPole-v1", 4, 2)


def _discrete_acrobot():
    from elegantrl_amd.envs import AcrobotGpuVecEnv
    return _discrete(AcrobotGpuVecEnv, "Acrobot-v1", 6, 3)


def _sac_syn():
    from elegantrl_amd.agents import AgentSAC
    from elegantrl_amd.envs import SynVecEnv
    S, A = 11, 3
    th.manual_seed(3)
    agent = AgentSAC(list(NET), S, A, gpu_id=0, args=_config(AgentSAC, "SynVecEnv", S, A, False))
    env = SynVecEnv(N, S, A, max_step=MAX_STEP, gpu_id=0, seed=5)
    return agent, env, "fused_rollout_offpolicy", (H, N, A), th.randn


def _two_rollouts(make, drop_token):
    agent, env, launch_name, shape, draw = make()
    agent.last_state = env.reset()[0]
    launches = []
    inner = getattr(env, launch_name)
    setattr(env, launch_name, lambda *a, **k: (launches.append(1), inner(*a, **k))[1])
    g = th.Generator(device=DEV).manual_seed(11)
    first, second = (draw(shape, device=DEV, generator=g) for _ in range(2))
    agent._explore_vec_env(env, H, noise=first)
    assert len(launches) == 1 and agent._last_state_token is not None      # the one-launch path ran and left its token
    if drop_token:
        agent._last_state_token = None
        with th.no_grad():
            env.state.add_(1.0)                         # the live buffer no longer holds the agent's last state: a skipped copy would show
    epoch = env.state_epoch
    items = agent._explore_vec_env(env, H, noise=second)
    assert len(launches) == 2
    out = dict(zip(("buf%d" % i for i in range(len(items))), items))
    out.update(last_state=agent.last_state, env_state=env.state, step_count=env.step_count, episode=env.episode)
    if hasattr(env, "phys"):
        out["phys"] = env.phys
    return out, agent.rng_counter, env.state_epoch - epoch


@pytest.mark.parametrize("make", [_ppo_syn, _discrete_cartpole, _discrete_acrobot, _sac_syn], ids=lambda f: f.__name__.strip("_"))
def test_second_rollout_is_bitwise_the_same_with_and_without_the_copy_back(make):
    kept, kept_counter, kept_moves = _two_rollouts(make, drop_token=False)
    copied, copied_counter, copied_moves = _two_rollouts(make, drop_token=True)
    assert kept_moves == 1 and copied_moves == 2           # the launch alone moved the env / the copy-back and the launch did
    assert kept_counter == copied_counter == 2 * H
    assert kept.keys() == copied.keys()
    for name in kept:
        a, b = kept[name], copied[name]
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert th.equal(a, b), f"{name}: {(a != b).sum().item()} elements differ"
    flags = [v for k, v in kept.items() if v.dtype == th.bool]
    assert any((~f).any() for f in flags), "the case is meant to contain resets"
