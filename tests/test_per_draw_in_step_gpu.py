"""The prioritised draw + gather inside the fused SAC step's first launch (args.per_draw_in_step, opt-in: erl_sac_update_per_draw_loop_f32,
erl_sac_update_mod_per_loop_f32 with draw_in_step = 1; csrc/sac_fused.hip actor_fwd_body's PER form on csrc/per_draw.h) against the loop
whose every step starts with a stand-alone erl_per_sample_rows_f32 launch: same seed, equal rings, equal injected uniforms -- everything
the loop writes, the staging block and the sampler's indices and weights of the last step included, must be the same bits."""
import numpy as np
import pytest
import torch as th

from tests.test_modsac_per_loop_gpu import (B, H, N, NETS, RINGS, SKIPPED, STEPS, assert_same_state, make, same_bits, spy, start_counts,
                                            uniforms)

pytestmark = pytest.mark.gpu

DRAW_RINGS = dict(RINGS, **{"ten-level-descent": (1024, 2)})      # a ten-level descent, 32 of its 1024 leaves filled
BATCHES = {"B64": 64, "B72-half-empty-last-tile": 72}               # 72 = 9 draws per sequence, 4.5 tiles of 16 rows


def assert_same_sample(ba, bb):
    """what the last step's draw + gather left: the staging block and the sampler's indices and weights"""
    names = ("state", "action", "reward", "undone", "unmask", "next_state")
    for name, x, y in zip(names, ba._stage.out, bb._stage.out):
        assert same_bits(x, y), name
    assert th.equal(ba._per_stage.is_index, bb._per_stage.is_index) and same_bits(ba._per_stage.is_weight, bb._per_stage.is_weight)
    assert th.equal(ba._per_stage.is_index, ba.ids1 * ba.cur_size + ba.ids0)
    assert int(ba.ids0.min()) >= 0 and int(ba.ids0.max()) <= ba.cur_size - 2
    assert bool(th.isfinite(ba._per_stage.is_weight).all()) and float(ba._per_stage.is_weight.min()) > 0


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("ring", list(DRAW_RINGS))
@pytest.mark.parametrize("net", list(NETS))
def test_sac_loop_with_the_draw_in_the_step_is_bit_identical(net, ring, batch, monkeypatch):
    from elegantrl_amd.agents import AgentSAC
    max_size, rollouts = DRAW_RINGS[ring]
    B_ = BATCHES[batch]
    calls = spy(monkeypatch)
    u = uniforms(STEPS, B_)
    a, ba = make(AgentSAC, NETS[net], max_size, rollouts, batch=B_, per_draw_in_step=True)
    b, bb = make(AgentSAC, NETS[net], max_size, rollouts, batch=B_)
    assert a.per_draw_in_step and not b.per_draw_in_step and ba.cur_size == min(max_size, rollouts * H)
    assert th.equal(ba._ring.block, bb._ring.block) and th.equal(ba.sum_trees.sum, bb.sum_trees.sum)
    sum0 = ba.sum_trees.sum.clone()
    oa = a.update_net(ba, per_uniform=u)
    assert calls["per_draw_loop"] == 1 and calls["per_loop"] == 0 and calls["per_step"] == 0
    assert "erl_sac_update_per_draw_loop_f32" in a.per_path and "draw + gather inside the step's first launch" in a.per_path
    ob = b.update_net(bb, per_uniform=u)
    assert calls["per_draw_loop"] == 1 and calls["per_loop"] == 1 and calls["per_step"] == 0
    assert "erl_sac_update_per_loop_f32" in b.per_path and "per_draw_in_step" not in b.per_path
    assert oa == ob and all(np.isfinite(x) for x in oa)
    assert_same_state(a, ba, b, bb, batch=B_)
    assert_same_sample(ba, bb)
    assert not th.equal(ba.sum_trees.sum, sum0) and a._step == STEPS and bool(th.isfinite(a.objs_all).all())


def test_modsac_loop_with_the_draw_in_the_step_is_bit_identical(monkeypatch):
    from elegantrl_amd.agents import AgentModSAC
    max_size, rollouts = RINGS["full-and-wrapped"]
    calls = spy(monkeypatch)
    u = uniforms()
    a, ba = make(AgentModSAC, (256, 256), max_size, rollouts, mod_per_loop_in_c=True, per_draw_in_step=True)
    b, bb = make(AgentModSAC, (256, 256), max_size, rollouts, mod_per_loop_in_c=True, per_draw_in_step=False)
    start_counts(a, b)
    oa = a.update_net(ba, per_uniform=u)
    ob = b.update_net(bb, per_uniform=u)
    assert calls["mod_per_loop"] == 2 and calls["draw_in_step"] == [True, False] and calls["per_step"] == calls["per_draw_loop"] == 0
    assert "erl_sac_update_mod_per_loop_f32" in a.per_path and "draw + gather inside the step's first launch" in a.per_path
    assert "erl_sac_update_mod_per_loop_f32" in b.per_path and "inside the step's first launch" not in b.per_path
    assert oa == ob and all(np.isfinite(x) for x in oa)
    assert_same_state(a, ba, b, bb)
    assert_same_sample(ba, bb)
    assert th.isnan(a.objs_all[:, 1]).nonzero().flatten().tolist() == SKIPPED and a.update_a == 5


def test_a_layered_net_ignores_the_switch_and_says_why(monkeypatch):
    from elegantrl_amd.agents import AgentSAC
    calls = spy(monkeypatch)
    agent, buf = make(AgentSAC, (64, 48, 32), 64, 2, steps=3, per_draw_in_step=True)
    objs = agent.update_net(buf, per_uniform=uniforms(3))
    assert calls["per_loop"] == 1 and calls["per_draw_loop"] == 0 and calls["per_step"] == 0
    assert "erl_sac_update_per_loop_f32" in agent.per_path and "per_draw_in_step ignored" in agent.per_path
    assert "layered step" in agent.per_path and "stand-alone draw" in agent.per_path
    assert all(np.isfinite(o) for o in objs) and agent._step == 3


@pytest.mark.parametrize("agent_class", ["AgentSAC", "AgentModSAC"])
def test_a_default_agent_never_enters_the_new_wrappers(agent_class, monkeypatch):
    """no switch named, nothing in the environment: the routes are the ones from before the new entries existed"""
    from elegantrl_amd import agents
    from elegantrl_amd.envs import SynVecEnv
    from elegantrl_amd.train import Config, ReplayBuffer
    for name in ("ERL_SAC_PER_DRAW_IN_STEP", "ERL_SAC_MOD_PER_LOOP_IN_C"):
        monkeypatch.delenv(name, raising=False)
    calls = spy(monkeypatch)
    cls = getattr(agents, agent_class)
    args = Config(cls, SynVecEnv, {"env_name": "SynVecEnv", "num_envs": N, "max_step": 50, "state_dim": 11, "action_dim": 3, "if_discrete": False})
    args.net_dims, args.horizon_len, args.batch_size, args.if_use_per, args.quiet = [256, 256], H, B, True, True
    th.manual_seed(5)
    agent = cls(args.net_dims, 11, 3, gpu_id=0, args=args)
    env = SynVecEnv(N, 11, 3, max_step=50, gpu_id=0, seed=1)
    agent.last_state = env.reset()[0]
    buf = ReplayBuffer(max_size=64, state_dim=11, action_dim=3, gpu_id=0, num_seqs=N, if_use_per=True, args=args)
    for _ in range(2):
        buf.update(agent.explore_env(env, H))
    agent.repeat_times = 3 * B / buf.cur_size
    objs = agent.update_net(buf)
    assert calls["mod_per_loop"] == 0 and calls["per_draw_loop"] == 0
    if agent_class == "AgentSAC":
        assert calls["per_loop"] == 1 and calls["per_step"] == 0 and "erl_sac_update_per_loop_f32" in agent.per_path
    else:
        assert calls["per_loop"] == 0 and calls["per_step"] == 3 and "per step" in agent.per_path and "AgentModSAC" in agent.per_path
    assert np.isfinite(objs[0]) and agent._step == 3
