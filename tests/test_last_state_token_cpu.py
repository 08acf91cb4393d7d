"""The rule "the env's live buffer already holds my last state, so skip the copy back" (AgentBase._hand_state_to_env /
_record_last_state, shared by the one-launch rollouts of AgentPPO, AgentDiscretePPO and AgentSAC), driven directly on a stub env with
CPU tensors: after a record nothing is copied, and each of the five things the token watches, changed alone, brings the copy back
exactly once (no GPU)."""
import pytest
import torch as th

N, S = 5, 4


class StubEnv:
    def __init__(self, with_epoch=True):
        self.state = th.zeros((N, S))
        if with_epoch:
            self.state_epoch = 0


def make_agent():
    from elegantrl_amd.agents import AgentDiscretePPO
    from elegantrl_amd.train import Config
    args = Config(AgentDiscretePPO, None, {"env_name": "CartPole-v1", "num_envs": N, "max_step": 5, "state_dim": S, "action_dim": 2,
                                           "if_discrete": True})
    args.net_dims, args.quiet = [64, 32], True
    return AgentDiscretePPO(args.net_dims, S, 2, gpu_id=-1, args=args)


def recorded():
    """an agent and an env right behind a one-launch rollout: the live buffer and the agent's copy hold the same final state"""
    agent, env = make_agent(), StubEnv()
    final = th.arange(N * S, dtype=th.float32).reshape(N, S)
    env.state.copy_(final)
    env.state_epoch += 1                                # (the rollout moved the env)
    agent._record_last_state(env, final.clone())
    return agent, env


def hand(agent, env):
    """what `_hand_state_to_env(env, agent.last_state)` did: (env.state was written, how far state_epoch moved)"""
    buf, version, epoch = env.state, env.state._version, getattr(env, "state_epoch", None)
    agent._hand_state_to_env(env, agent.last_state)
    assert env.state is buf                             # the env owns the live buffer: written in place, never rebound
    return env.state._version - version, None if epoch is None else env.state_epoch - epoch


def test_record_sets_last_state_and_a_five_field_token():
    agent, env = recorded()
    tok = agent._last_state_token
    assert isinstance(tok, tuple) and len(tok) == 5
    assert tok[0] is agent.last_state and tok[1] == agent.last_state._version and tok[2] is env
    assert tok[3] == env.state_epoch and tok[4] == (id(env.state), env.state._version)


def test_after_record_nothing_is_copied():
    agent, env = recorded()
    for _ in range(2):
        assert hand(agent, env) == (0, 0)


def _rebind_last_state(agent, env):
    agent.last_state = agent.last_state.clone()
    return env


def _write_last_state(agent, env):
    agent.last_state.add_(1.0)
    return env


def _other_env(agent, env):
    other = StubEnv()
    other.state_epoch = env.state_epoch
    return other


def _advance_epoch(agent, env):
    env.state_epoch += 1
    return env


def _write_env_state(agent, env):
    env.state.mul_(2.0)
    return env


def _rebind_env_state(agent, env):
    env.state = env.state.clone()
    return env


@pytest.mark.parametrize("invalidate", [_rebind_last_state, _write_last_state, _other_env, _advance_epoch, _write_env_state,
                                        _rebind_env_state], ids=lambda f: f.__name__.strip("_"))
def test_each_invalidation_alone_copies_and_bumps_the_epoch_once(invalidate):
    agent, env = recorded()
    env = invalidate(agent, env)
    assert hand(agent, env) == (1, 1)
    assert th.equal(env.state, agent.last_state)


def test_no_token_copies():
    agent, env = recorded()
    agent._last_state_token = None
    env.state.zero_()
    assert hand(agent, env) == (1, 1)
    assert th.equal(env.state, agent.last_state)


def test_an_env_without_state_epoch_gets_the_copy():
    agent, env = make_agent(), StubEnv(with_epoch=False)
    agent.last_state = th.ones((N, S))
    assert agent._last_state_token is None
    assert hand(agent, env) == (1, None)
    assert th.equal(env.state, agent.last_state) and not hasattr(env, "state_epoch")
    # ... and a record on such an env holds until somebody writes either side
    agent._record_last_state(env, env.state.clone())
    assert agent._last_state_token[3] is None and hand(agent, env) == (0, None)
    env.state.add_(1.0)
    assert hand(agent, env) == (1, None)


def test_the_live_buffer_itself_is_never_copied_onto_itself():
    agent, env = make_agent(), StubEnv()
    agent.last_state = env.state                        # (args.snapshot_last_state = False hands out the live buffer)
    assert hand(agent, env) == (0, 0)
