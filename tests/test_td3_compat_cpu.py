"""The import block of the reference's off-policy demo (examples/demo_DDPG_TD3_SAC.py:13-14 there) resolves to this package, in a fresh
interpreter as tests/test_compat.py does; what that file pins as absent stays absent; the agents' constructor contract without a GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code: str):
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1", ERL_QUIET="1")
    out = subprocess.run([sys.executable, "-c", code], cwd="/", env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


def test_the_demo_import_block_resolves_to_this_package():
    out = _run("""
from elegantrl.agents import AgentDDPG, AgentTD3
from elegantrl.agents import AgentSAC, AgentModSAC
from elegantrl.train.config import Config
import sys
real = sys.modules["elegantrl_amd.agents.AgentDDPG"]                      # (the package attribute of that name is the class)
assert AgentTD3 is real.AgentTD3 and AgentDDPG is real.AgentDDPG and AgentTD3.__module__ == "elegantrl_amd.agents.AgentDDPG"
env_args = {"env_name": "x", "num_envs": 4, "max_step": 10, "state_dim": 3, "action_dim": 1, "if_discrete": False}
for cls in (AgentTD3, AgentDDPG):
    args = Config(cls, None, dict(env_args))
    assert args.if_off_policy and args.batch_size == 64 and args.buffer_init_size == 512
try:
    import elegantrl.agents.AgentTD3                                      # the module path stays unsupported
    raise SystemExit("the module elegantrl.agents.AgentTD3 should not exist")
except ModuleNotFoundError:
    pass
try:
    from elegantrl.agents import AgentDQN                                 # the DQN family stays out of scope
    raise SystemExit("AgentDQN should not exist")
except ImportError:
    pass
print("ok")
""")
    assert out.strip().endswith("ok")


def _args(cls, **extra):
    from elegantrl_amd.train import Config
    args = Config(cls, None, {"env_name": "x", "num_envs": 4, "max_step": 10, "state_dim": 11, "action_dim": 3, "if_discrete": False})
    args.net_dims, args.quiet = [64, 32], True
    for k, v in extra.items():
        setattr(args, k, v)
    return args


def test_defaults_and_the_reference_attribute_names():
    from elegantrl_amd.agents import Actor, AgentDDPG, AgentTD3, Critic, CriticTwin
    td3 = AgentTD3([64, 32], 11, 3, gpu_id=-1, args=_args(AgentTD3))
    assert (td3.num_ensembles, td3.update_freq, td3.policy_noise_std, td3.explore_noise_std) == (8, 2, 0.10, 0.05)
    assert td3.if_off_policy and isinstance(td3.act, Actor) and type(td3.cri) is CriticTwin and type(td3.cri_target) is CriticTwin
    assert isinstance(td3.act_target, Actor) and td3.act_target is not td3.act
    assert td3.save_attr_names == {"act", "act_target", "act_optimizer", "cri", "cri_target", "cri_optimizer"}
    assert td3.update_path is None and td3.rollout_path is None
    assert list(td3.act.state_dict()) == ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias"]
    assert td3.cri.state_dict()["net.4.weight"].shape == (8, 32) and td3.cri.state_dict()["net.0.weight"].shape == (64, 14)
    # the modules are views of the flat blocks, in state_dict order
    assert td3.act.net[0].weight.data_ptr() == td3._actor_flat.data_ptr()
    assert td3.cri_target.net[0].weight.data_ptr() == td3._critic_target_flat.data_ptr()
    assert sum(p.numel() for p in td3.cri.parameters()) == td3._spec.critic_count == 14 * 64 + 64 + 64 * 32 + 32 + 32 * 8 + 8
    tuned = AgentTD3([64, 32], 11, 3, gpu_id=-1, args=_args(AgentTD3, num_ensembles=2, update_freq=3, policy_noise_std=0.2, explore_noise_std=0.3))
    assert (tuned.num_ensembles, tuned.update_freq, tuned.policy_noise_std, tuned.explore_noise_std) == (2, 3, 0.2, 0.3)

    ddpg = AgentDDPG([64, 32], 11, 3, gpu_id=-1, args=_args(AgentDDPG, explore_noise=0.2, explore_noise_std=0.9, num_ensembles=5))
    assert (ddpg.num_ensembles, ddpg.update_freq, ddpg.policy_noise_std, ddpg.explore_noise_std) == (1, 1, 0.0, 0.2)     # `explore_noise`
    assert type(ddpg.cri) is Critic and ddpg.cri.state_dict()["net.4.weight"].shape == (1, 32)


def test_what_the_constructor_refuses():
    import torch as th
    from elegantrl_amd.agents import AgentDDPG, AgentTD3
    for cls in (AgentTD3, AgentDDPG):
        with pytest.raises(NotImplementedError, match="lambda_fit_cum_r"):
            cls([64, 32], 11, 3, gpu_id=-1, args=_args(cls, lambda_fit_cum_r=0.5))
        with pytest.raises(NotImplementedError, match="criterion"):                        # AgentBase's criterion rules
            cls([64, 32], 11, 3, gpu_id=-1, args=_args(cls, criterion=th.nn.L1Loss(reduction="none")))
        with pytest.raises(ValueError, match="reduction"):
            cls([64, 32], 11, 3, gpu_id=-1, args=_args(cls, criterion=th.nn.SmoothL1Loss()))
        assert cls([64, 32], 11, 3, gpu_id=-1, args=_args(cls, criterion=th.nn.HuberLoss(reduction="none", delta=0.5))).criterion_code[1] == 0.5
    with pytest.raises(ValueError, match="update_freq"):
        AgentTD3([64, 32], 11, 3, gpu_id=-1, args=_args(AgentTD3, update_freq=0))


def test_every_kernel_launching_method_pins_its_device_once():
    from elegantrl_amd.agents import AgentDDPG, AgentTD3

    def depth(f):
        n = 0
        while hasattr(f, "__wrapped__"):
            f, n = f.__wrapped__, n + 1
        return n

    for cls in (AgentTD3, AgentDDPG):
        for n in ("explore_env", "explore_action", "_explore_vec_env", "_explore_one_env", "update_objectives", "update_net"):
            assert depth(getattr(cls, n)) == 1, f"{cls.__name__}.{n}: wrapped {depth(getattr(cls, n))} times by _hip.on_device"


def test_actor_and_critic_modules_follow_the_reference_formulas():
    import torch as th
    from elegantrl_amd.agents import Actor, CriticTwin
    th.manual_seed(0)
    act, cri = Actor([16, 8], 5, 2), CriticTwin([16, 8], 5, 2, num_ensembles=4)
    s, eps = th.randn(7, 5), th.randn(7, 2) * 30
    with th.no_grad():
        a = act.get_action(s, 0.1, noise=eps)
        assert th.equal(a, (act(s) + 0.1 * eps).clip(-1, 1)) and a.abs().max() == 1.0       # the action is clipped, the noise is not
        q = cri.get_q_values(s, a)
        assert q.shape == (7, 4) and th.allclose(cri(s, a), q.mean(1, keepdim=True))
