"""AgentModSAC.update_net with prioritised replay as ONE C call (erl_sac_update_mod_per_loop_f32; args.mod_per_loop_in_c, opt-in) against
the per-step route (AgentSAC._per_step on the fused ModSAC step, AgentModSAC._step_options per step): two agents from one seed, equal rings
and equal injected uniforms must end bit-identical in everything the loop writes -- counters, trees and the nan pattern of the skipped
actor steps included.  per_alpha = 0.6, so the priorities move between the steps and step t + 1 draws from the trees step t updated.
No tolerance anywhere: the per-step route is what the fp64 restatement and the reference's recorded runs are pinned to."""
import math

import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

N, S, A, B, H, STEPS = 8, 11, 3, 64, 16, 8
NETS = {"256x256": (256, 256), "64x48": (64, 48)}
RINGS = {"partly-filled": (64, 2), "full-and-wrapped": (32, 3)}          # max_size, rollouts of 16 rows
SKIPPED = [2, 5, 7]        # update_a / (t + 1) < 1 / (2 - exp(-1)) = 0.6127 fails at 2/3, 4/6, 5/8: the loop ends on a skipped step
STEP0, ACTOR_STEP0 = 6, 4  # a run that has updated before: both counts run on


def make(agent_class, net, max_size, rollouts, batch=B, steps=STEPS, **extra):
    """an agent and a prioritised replay ring filled by its own rollouts on SynVecEnv (same seeds: same agent, same ring)"""
    from elegantrl_amd.envs import SynVecEnv
    from elegantrl_amd.train import Config, ReplayBuffer
    args = Config(agent_class, SynVecEnv, {"env_name": "SynVecEnv", "num_envs": N, "max_step": 50, "state_dim": S, "action_dim": A,
                                           "if_discrete": False})
    args.net_dims, args.horizon_len, args.batch_size, args.if_use_per, args.random_seed = list(net), H, batch, True, 3
    args.per_alpha, args.per_beta, args.quiet, args.fused_step = 0.6, 0.4, True, True
    for k, v in extra.items():
        setattr(args, k, v)
    th.manual_seed(5)
    agent = agent_class(args.net_dims, S, A, gpu_id=0, args=args)
    env = SynVecEnv(N, S, A, max_step=50, gpu_id=0, seed=1)
    agent.last_state = env.reset()[0]
    buf = ReplayBuffer(max_size=max_size, state_dim=S, action_dim=A, gpu_id=0, num_seqs=N, if_use_per=True, args=args)
    for _ in range(rollouts):
        buf.update(agent.explore_env(env, H))
    agent.repeat_times = steps * batch / buf.cur_size           # update_times = int(cur_size * repeat_times / batch_size) = steps
    assert int(buf.cur_size * agent.repeat_times / batch) == steps
    return agent, buf


def uniforms(steps=STEPS, batch=B):
    u = th.rand((steps, N, batch // N), device="cuda:0", generator=th.Generator(device="cuda:0").manual_seed(11))
    u[0, 0, 0], u[1, -1, -1] = 0.0, float(1 - 2.0 ** -24)      # both ends of [0, 1)
    return u


def spy(monkeypatch):
    """counts the entries into ops' prioritised-loop wrappers and into the per-step route"""
    from elegantrl_amd import ops
    from elegantrl_amd.agents import AgentSAC
    calls = {"per_loop": 0, "mod_per_loop": 0, "per_draw_loop": 0, "per_step": 0, "draw_in_step": []}

    def counted(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            if name == "mod_per_loop":
                calls["draw_in_step"].append(bool(k.get("draw_in_step", False)))
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(ops, "sac_update_per_loop", counted("per_loop", ops.sac_update_per_loop))
    monkeypatch.setattr(ops, "sac_update_mod_per_loop", counted("mod_per_loop", ops.sac_update_mod_per_loop))
    monkeypatch.setattr(ops, "sac_update_per_draw_loop", counted("per_draw_loop", ops.sac_update_per_draw_loop))
    monkeypatch.setattr(AgentSAC, "_per_step", counted("per_step", AgentSAC._per_step))
    return calls


def same_bits(x: th.Tensor, y: th.Tensor) -> bool:
    """equal as bit patterns: NaN positions included, +0 and -0 apart"""
    return x.shape == y.shape and x.dtype == y.dtype and th.equal(x.contiguous().view(th.int32), y.contiguous().view(th.int32))


def assert_same_state(a, ba, b, bb, batch=B):
    """everything a prioritised update_net writes, agent `a` on buffer `ba` against agent `b` on `bb`, bit for bit"""
    names = ["_actor_flat", "_critic_flat", "_target_flat", "alpha_log"] + (["_actor_target_flat"] if hasattr(a, "_actor_target_flat") else [])
    for name in names:
        assert same_bits(getattr(a, name), getattr(b, name)), name
    for opt in ("act_optimizer", "cri_optimizer", "alpha_optim"):                  # all six Adam moment vectors, the three step counts
        x, y = getattr(a, opt), getattr(b, opt)
        assert same_bits(x.exp_avg, y.exp_avg) and same_bits(x.exp_avg_sq, y.exp_avg_sq), opt
        assert x.step_count == y.step_count, opt
    assert same_bits(ba.sum_trees.sum, bb.sum_trees.sum) and same_bits(ba.sum_trees.min, bb.sum_trees.min)
    assert th.equal(ba.ids0, bb.ids0) and th.equal(ba.ids1, bb.ids1) and ba.ids0.shape == (batch,)
    assert same_bits(a._td_error, b._td_error) and a._td_error.shape == (batch,)
    assert same_bits(a.objs_all, b.objs_all)
    assert a._step == b._step


def start_counts(*agents):
    for x in agents:
        x._step, x._actor_step = STEP0, ACTOR_STEP0


@pytest.mark.parametrize("ring", list(RINGS))
@pytest.mark.parametrize("net", list(NETS))
def test_one_call_loop_is_bit_identical_to_the_per_step_route(net, ring, monkeypatch):
    from elegantrl_amd.agents import AgentModSAC
    max_size, rollouts = RINGS[ring]
    calls = spy(monkeypatch)
    u = uniforms()
    a, ba = make(AgentModSAC, NETS[net], max_size, rollouts, mod_per_loop_in_c=True)
    b, bb = make(AgentModSAC, NETS[net], max_size, rollouts)                    # the switch is not named: the per-step route
    assert a.mod_per_loop_in_c and not b.mod_per_loop_in_c and not a.per_draw_in_step
    assert ba.if_full == (ring == "full-and-wrapped") and ba.cur_size == min(max_size, rollouts * H) and ba.p == bb.p
    assert th.equal(ba._ring.block, bb._ring.block) and th.equal(ba.sum_trees.sum, bb.sum_trees.sum) and th.equal(a._actor_flat, b._actor_flat)
    start_counts(a, b)
    sum0, min0 = ba.sum_trees.sum.clone(), ba.sum_trees.min.clone()
    oa = a.update_net(ba, per_uniform=u)
    assert calls["mod_per_loop"] == 1 and calls["per_step"] == 0 and calls["per_loop"] == 0 and calls["draw_in_step"] == [False]
    assert "one C call" in a.per_path and "erl_sac_update_mod_per_loop_f32" in a.per_path
    assert a.update_path.startswith("per step: ") and "prioritised" in a.update_path
    ob = b.update_net(bb, per_uniform=u)
    assert calls["mod_per_loop"] == 1 and calls["per_step"] == STEPS and calls["per_loop"] == 0
    assert "per step" in b.per_path and "AgentModSAC" in b.per_path and "mod_per_loop_in_c" in b.per_path
    assert oa == ob and all(np.isfinite(x) for x in oa)
    assert_same_state(a, ba, b, bb)
    assert not th.equal(ba.sum_trees.sum, sum0) and not th.equal(ba.sum_trees.min, min0)        # the priorities did move
    for x in (a, b):
        assert th.isnan(x.objs_all[:, 1]).nonzero().flatten().tolist() == SKIPPED and bool(th.isfinite(x.objs_all[:, 0]).all())
        assert x.update_a == 5 and x._actor_step == ACTOR_STEP0 + 5 and x._step == STEP0 + STEPS and not x._last_actor_updated
        assert x.cri_optimizer.step_count == x.alpha_optim.step_count == STEP0 + STEPS and x.act_optimizer.step_count == ACTOR_STEP0 + 5
    assert not th.equal(a._actor_flat, a._actor_target_flat)
    # the trees were updated behind the skipped steps too: the loop ends on one, and its td errors are the leaves of the rows it drew
    # (td.clamp(1e-8, 10) ** per_alpha; a row drawn twice keeps its last entry).  The device's powf against torch's: a few ulp.
    L = ba.sum_trees.leaves
    leaves = ba.sum_trees.sum.view(N, 2 * L)[:, L:].cpu()
    want = a._td_error.clamp(1e-8, 10.0).pow(0.6).cpu()
    last = {(int(q), int(r)): float(w) for q, r, w in zip(ba.ids1.cpu(), ba.ids0.cpu(), want)}
    assert len(last) >= N
    for (q, r), w in last.items():
        assert math.isclose(float(leaves[q, r]), w, rel_tol=1e-5), (q, r, float(leaves[q, r]), w)


@pytest.mark.parametrize("case", ["lambda_fit_cum_r", "three-hidden-layers", "fused_step-off"])
def test_switch_on_but_a_condition_missing_keeps_the_per_step_route(case, monkeypatch):
    from elegantrl_amd.agents import AgentModSAC
    net, extra, word = {"lambda_fit_cum_r": ((256, 256), {"lambda_fit_cum_r": 0.3}, "lambda_fit_cum_r"),
                        "three-hidden-layers": ((64, 48, 32), {}, "outside the fused step's shapes"),
                        "fused_step-off": ((256, 256), {"fused_step": False}, "args.fused_step is off")}[case]
    calls = spy(monkeypatch)
    agent, buf = make(AgentModSAC, net, 64, 2, steps=3, mod_per_loop_in_c=True, **extra)
    assert agent.mod_per_loop_in_c
    objs = agent.update_net(buf)
    assert calls["mod_per_loop"] == 0 and calls["per_loop"] == 0 and calls["per_step"] == 3
    assert "per step" in agent.per_path and word in agent.per_path, agent.per_path
    assert np.isfinite(objs[0]) and agent._step == 3 and agent.update_a == 2
