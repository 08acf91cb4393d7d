"""AgentModSAC on the fused SAC step (csrc/sac_fused.hip with ActorFixSAC as a run-time variant; erl_sac_update_mod_f32 /
erl_sac_update_mod_ring_f32 / erl_sac_update_mod_ring_loop_f32): against oracle/sac_torch.py's ModSacStepper and the reference's own run
(tests/golden/sac_mod_small.npz), the skipped actor step, the one-call update loop against the per-step calls bit for bit, the routes that
stay where they were, and the checkpoint.  Every agent here names `args.fused_step` itself: nothing depends on the default.
Tolerances: those of the layered step against the same oracle (tests/test_sac.py)."""
import numpy as np
import pytest
import torch as th

from tests.helpers import load

pytestmark = pytest.mark.gpu

N, S, A, B, H, STEPS = 8, 11, 3, 64, 16, 8
RINGS = {"partly-filled": (64, 2), "full-and-wrapped": (32, 3)}          # max_size, rollouts of 16 rows
SKIPPED = [2, 5, 7]        # update_a / (t + 1) < 1 / (2 - exp(-1)) = 0.6127 fails at 2/3, 4/6, 5/8


def _spy(monkeypatch):
    """counts the entries into ops' three fused ModSAC wrappers, into the layered step's wrapper and into the per-step PER route"""
    from elegantrl_amd import ops
    from elegantrl_amd.agents import AgentSAC
    calls = {"step": 0, "ring_step": 0, "loop": 0, "layered": 0, "per_step": 0}
    step, ring_step, loop, layered, per_step = (ops.sac_update_mod, ops.sac_update_mod_from_ring, ops.sac_update_mod_ring_loop, ops.sac_update,
                                                AgentSAC._per_step)

    def counted(name, fn):
        def spy(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return spy
    monkeypatch.setattr(ops, "sac_update_mod", counted("step", step))
    monkeypatch.setattr(ops, "sac_update_mod_from_ring", counted("ring_step", ring_step))
    monkeypatch.setattr(ops, "sac_update_mod_ring_loop", counted("loop", loop))
    monkeypatch.setattr(ops, "sac_update", counted("layered", layered))
    monkeypatch.setattr(AgentSAC, "_per_step", counted("per_step", per_step))
    return calls


def _agent(net, S_=S, A_=A, E=8, B_=B, fused=True, **extra):
    from elegantrl_amd.agents import AgentModSAC
    from elegantrl_amd.train import Config
    args = Config(AgentModSAC, None, {"env_name": "x", "num_envs": N, "max_step": 50, "state_dim": S_, "action_dim": A_, "if_discrete": False})
    args.net_dims, args.batch_size, args.learning_rate, args.gamma, args.num_ensembles = list(net), B_, 1e-3, 0.98, E
    args.fused_step, args.quiet, args.random_seed, args.horizon_len = fused, True, 3, H
    for k, v in extra.items():
        setattr(args, k, v)
    return AgentModSAC(args.net_dims, S_, A_, gpu_id=0, args=args), args


def _with_ring(net, max_size, rollouts, steps=STEPS, **extra):
    """an agent and a replay ring filled by its own rollouts on SynVecEnv (same seeds: same agent, same ring)"""
    from elegantrl_amd.envs import SynVecEnv
    from elegantrl_amd.train import ReplayBuffer
    th.manual_seed(5)
    agent, args = _agent(net, **extra)
    env = SynVecEnv(N, S, A, max_step=50, gpu_id=0, seed=1)
    agent.last_state = env.reset()[0]
    buf = ReplayBuffer(max_size=max_size, state_dim=S, action_dim=A, gpu_id=0, num_seqs=N, if_use_per=bool(extra.get("if_use_per", False)), args=args)
    for _ in range(rollouts):
        buf.update(agent.explore_env(env, H))
    agent.repeat_times = steps * B / buf.cur_size               # update_times = int(cur_size * repeat_times / batch_size) = steps
    return agent, buf


STEP_SHAPES = {
    "split-critic-passes": ((256, 256), 8, 64, 11, 3),          # 4 tiles x 8 x 4 <= 256: every critic pass split, actor pair launch
    "unsplit-critic": ((256, 256), 8, 256, 11, 3),              # 16 x 8 x 4 > 256: critic unsplit, actor pair launch
    "ragged-128x64": ((128, 64), 4, 100, 11, 3),                # ragged last tile, unsplit forms, mixed width classes
    "limits-S56-A8": ((64, 32), 8, 17, 56, 8),                  # S + A = 64, A = 8; one row in the last tile
    "narrowest": ((16, 16), 1, 16, 11, 3),                      # the narrowest layers, a single critic
}


@pytest.mark.parametrize("shape", list(STEP_SHAPES))
def test_fused_step_matches_the_torch_restatement(shape, monkeypatch):
    """three steps with injected noise against ModSacStepper; step t = 2 skips the actor"""
    from oracle.sac_torch import ModSacStepper
    net, E, B_, S_, A_ = STEP_SHAPES[shape]
    calls = _spy(monkeypatch)
    dev = th.device("cuda:0")
    g = th.Generator().manual_seed(len(shape) * 100 + E)
    agent, _ = _agent(net, S_, A_, E, B_)
    assert agent.kernel_path.startswith("fused ModSAC step")
    th.set_grad_enabled(True)
    try:
        st = ModSacStepper(list(net), S_, A_, E, 1e-3, 0.98, float(agent.soft_update_tau), float(agent.clip_grad_norm))
        st.act.load_state_dict({k: v.detach().cpu() for k, v in agent.act.state_dict().items()})
        st.act_target.load_state_dict(st.act.state_dict())
        st.cri.load_state_dict({k: v.detach().cpu() for k, v in agent.cri.state_dict().items()})
        st.cri_target.load_state_dict(st.cri.state_dict())
        st.reset_optimizers()
        batch = (th.randn(B_, S_, generator=g), th.randn(B_, A_, generator=g).tanh(), th.randn(B_, generator=g),
                 (th.rand(B_, generator=g) < 0.97).float(), (th.rand(B_, generator=g) < 0.98).float(), th.randn(B_, S_, generator=g))
        dbatch = tuple(x.to(dev).contiguous() for x in batch)
        objs = th.zeros(2, device=dev)
        for t in range(3):
            e_next, e_cur = th.randn(B_, A_, generator=g), th.randn(B_, A_, generator=g)
            oc, oa = st.step(batch, e_next, e_cur, update_t=t)
            agent._update_on_batch(dbatch, objs, noises=(e_next.to(dev), e_cur.to(dev)), update_t=t)
            got = objs.cpu().numpy()
            print(shape, t, "objectives", got, "oracle", (oc, oa))
            assert np.isnan(oa) == np.isnan(got[1]) == (t == 2)
            np.testing.assert_allclose(got, [oc, oa], rtol=3e-4, atol=3e-6, equal_nan=True)
            for name, mine, ref in (("act", agent.act, st.act), ("act_target", agent.act_target, st.act_target), ("cri", agent.cri, st.cri),
                                    ("cri_target", agent.cri_target, st.cri_target)):
                for k, v in ref.state_dict().items():
                    np.testing.assert_allclose(mine.state_dict()[k].cpu().numpy(), v.numpy(), rtol=0, atol=4e-5, err_msg=f"{name}.{k} after step {t}")
            np.testing.assert_allclose(agent.alpha_log.detach().cpu().numpy(), st.alpha_log.detach().numpy(), rtol=0, atol=1e-5)
    finally:
        th.set_grad_enabled(False)
    assert calls["step"] == 3 and calls["layered"] == 0
    assert agent._step == 3 and agent._actor_step == 2 and agent.act_optimizer.step_count == 2 and agent.cri_optimizer.step_count == 3


def test_fused_step_replays_the_reference(monkeypatch):
    """tests/golden/sac_mod_small.npz -- the reference's own AgentModSAC run -- through update_objectives on the fused route: four steps with
    the recorded ids / noise (tolerances of the layered step's replay, tests/test_sac.py)"""
    from elegantrl_amd.train import ReplayBuffer
    from tests.test_sac import _load_nets, _mod_setup
    calls = _spy(monkeypatch)
    g = load("sac_mod_small.npz")
    (N_, S_, A_, rows, B_, n_upd, n_ens, h1, h2), (gamma, lr, max_norm, reward_scale, tau, target_entropy, critic_tau, critic_value) = _mod_setup(g)
    dev = th.device("cuda:0")
    agent, _ = _agent((h1, h2), S_, A_, n_ens, B_, learning_rate=lr, gamma=gamma, reward_scale=reward_scale, soft_update_tau=tau,
                      clip_grad_norm=max_norm, num_envs=N_)
    assert n_upd == 4 and abs(agent.target_entropy - target_entropy) < 1e-12 and agent.critic_value == critic_value
    _load_nets(g, 0, agent.act, agent.cri)
    agent.act_target.load_state_dict(agent.act.state_dict())
    agent.cri_target.load_state_dict(agent.cri.state_dict())
    with th.no_grad():
        agent.alpha_log[:] = th.from_numpy(g["alpha_log0"]).to(dev)
    buf = ReplayBuffer(max_size=rows + 5, state_dim=S_, action_dim=A_, gpu_id=0, num_seqs=N_)
    buf.update(tuple(th.from_numpy(g[n]).to(dev) for n in ("ro_states", "ro_actions", "ro_rewards", "ro_undones", "ro_unmasks")))
    for t in range(n_upd):
        oc, oa = agent.update_objectives(buf, t, ids=th.from_numpy(g["ids"][t]).to(dev),
                                         noises=(th.from_numpy(g["eps_next"][t]).to(dev), th.from_numpy(g["eps_cur"][t]).to(dev)))
        print("golden step", t, (oc, oa), g["objs"][t])
        assert np.isnan(oa) == (g["actor_updated"][t] == 0) and agent._last_actor_updated == bool(g["actor_updated"][t])
        np.testing.assert_allclose([oc, oa], g["objs"][t], rtol=2e-4, atol=2e-6, equal_nan=True)
        for prefix, net in ((f"act{t + 1}", agent.act), (f"actt{t + 1}", agent.act_target), (f"cri{t + 1}", agent.cri),
                            (f"crit{t + 1}", agent.cri_target)):
            for k, v in net.state_dict().items():
                np.testing.assert_allclose(v.cpu().numpy(), g[f"{prefix}.{k}"], rtol=0, atol=3e-5, err_msg=f"{prefix}.{k} after step {t}")
        np.testing.assert_allclose(agent.alpha_log.detach().cpu().numpy(), g[f"alpha_log{t + 1}"], rtol=0, atol=1e-5)
    assert calls["step"] == 4 and calls["layered"] == 0
    assert agent._actor_step == 3 and agent.act_optimizer.step_count == 3 and agent.cri_optimizer.step_count == 4


@pytest.mark.parametrize("net,B_", [((256, 256), 64), ((64, 32), 100)], ids=["split-forms", "unsplit-ragged"])
def test_skipped_step_leaves_the_actor_alone(net, B_, monkeypatch):
    calls = _spy(monkeypatch)
    dev = th.device("cuda:0")
    g = th.Generator().manual_seed(7)
    agent, _ = _agent(net, B_=B_)
    batch = tuple(x.to(dev).contiguous() for x in (
        th.randn(B_, S, generator=g), th.randn(B_, A, generator=g).tanh(), th.randn(B_, generator=g), (th.rand(B_, generator=g) < 0.97).float(),
        (th.rand(B_, generator=g) < 0.98).float(), th.randn(B_, S, generator=g)))
    objs = th.zeros(2, device=dev)
    td = th.full((B_,), -1.0, device=dev)
    agent._update_on_batch(batch, objs, update_t=0)                      # one full step first: the actor's moments are not all zero
    assert agent._last_actor_updated and bool(th.isfinite(objs).all())
    before = [x.clone() for x in (agent._actor_flat, agent._actor_target_flat, agent.act_optimizer.exp_avg, agent.act_optimizer.exp_avg_sq)]
    others = [x.clone() for x in (agent._critic_flat, agent._target_flat, agent.alpha_log)]
    assert float(before[2].abs().max()) > 0
    agent.update_a = 2                                                   # 2 / 3 >= 0.6127: update_t = 2 skips the actor
    agent._update_on_batch(batch, objs, update_t=2, td_error_out=td)
    assert not agent._last_actor_updated and agent._actor_step == 1 and agent._step == 2
    for was, now in zip(before, (agent._actor_flat, agent._actor_target_flat, agent.act_optimizer.exp_avg, agent.act_optimizer.exp_avg_sq)):
        assert th.equal(was, now)
    for was, now in zip(others, (agent._critic_flat, agent._target_flat, agent.alpha_log)):
        assert not th.equal(was, now)
    o = objs.cpu().numpy()
    assert np.isnan(o[1]) and np.isfinite(o[0]) and o[0] > 0
    # the td errors of the skipped step were written, and the critic objective is their mean
    assert float(td.min()) >= 0 and abs(float(td.mean()) - o[0]) <= 1e-5 * max(1.0, abs(o[0]))
    assert calls["step"] == 2 and calls["layered"] == 0


@pytest.mark.parametrize("ring", list(RINGS))
@pytest.mark.parametrize("net", [(256, 256), (64, 32)], ids=["256x256", "64x32"])
def test_one_call_loop_is_bit_identical_to_the_per_step_fused_calls(net, ring, monkeypatch):
    max_size, rollouts = RINGS[ring]
    calls = _spy(monkeypatch)
    a, ba = _with_ring(net, max_size, rollouts, update_loop_in_c=True)
    b, bb = _with_ring(net, max_size, rollouts, update_loop_in_c=False)
    assert ba.if_full == (ring == "full-and-wrapped") and ba.cur_size == min(max_size, rollouts * H) and ba.p == bb.p
    assert th.equal(ba._ring.block, bb._ring.block) and th.equal(a._actor_flat, b._actor_flat) and th.equal(a._critic_flat, b._critic_flat)
    a._actor_step = b._actor_step = 4                                     # (a run that has updated before: the counts run on)
    a._step = b._step = 6
    th.manual_seed(9)
    oa = a.update_net(ba)
    assert calls["loop"] == 1 and calls["ring_step"] == 0 and calls["step"] == 0 and calls["layered"] == 0
    assert a.update_path.startswith("one C call") and "erl_sac_update_mod_ring_loop_f32" in a.update_path
    th.manual_seed(9)                                                     # the same th.randint ids
    ob = b.update_net(bb)
    assert calls["loop"] == 1 and calls["ring_step"] == STEPS and calls["step"] == 0 and calls["layered"] == 0
    assert b.update_path.startswith("per step: ") and "update_loop_in_c is off" in b.update_path
    assert oa == ob and all(np.isfinite(x) for x in oa)
    for name in ("_actor_flat", "_critic_flat", "_target_flat", "_actor_target_flat", "alpha_log"):
        assert th.equal(getattr(a, name), getattr(b, name)), name
    for opt in ("act_optimizer", "cri_optimizer", "alpha_optim"):                  # all six Adam moment vectors
        x, y = getattr(a, opt), getattr(b, opt)
        assert th.equal(x.exp_avg, y.exp_avg) and th.equal(x.exp_avg_sq, y.exp_avg_sq), opt
    assert th.equal(ba.ids0, bb.ids0) and th.equal(ba.ids1, bb.ids1) and ba.ids0.shape == (B,)
    assert a.objs_all.shape == (STEPS, 2) and th.equal(a.objs_all.isnan(), b.objs_all.isnan())
    assert th.equal(a.objs_all.nan_to_num(nan=-7.0), b.objs_all.nan_to_num(nan=-7.0))
    for x in (a, b):
        assert x.update_a == 5 and x._actor_step == 4 + 5 and x._step == 6 + STEPS
        assert x.cri_optimizer.step_count == x.alpha_optim.step_count == 6 + STEPS and x.act_optimizer.step_count == 4 + 5
        assert not x._last_actor_updated
        assert th.isnan(x.objs_all[:, 1]).nonzero().flatten().tolist() == SKIPPED and bool(th.isfinite(x.objs_all[:, 0]).all())
    assert not th.equal(a._actor_flat, a._actor_target_flat)


@pytest.mark.parametrize("case", ["one-hidden-layer", "three-hidden-layers", "lambda_fit_cum_r", "fused_step-off"])
def test_routes_that_stay_layered(case, monkeypatch):
    net, extra, word = {"one-hidden-layer": ((64,), {}, "outside the fused step's shapes"),
                        "three-hidden-layers": ((64, 48, 32), {}, "outside the fused step's shapes"),
                        "lambda_fit_cum_r": ((256, 256), {"lambda_fit_cum_r": 0.3}, "lambda_fit_cum_r"),
                        "fused_step-off": ((256, 256), {"fused": False}, "args.fused_step is off")}[case]
    calls = _spy(monkeypatch)
    agent, buf = _with_ring(net, 64, 2, steps=3, **extra)
    assert agent.kernel_path.startswith("layered ModSAC step") and word in agent.kernel_path
    objs = agent.update_net(buf)
    assert calls["step"] == calls["ring_step"] == calls["loop"] == 0 and calls["layered"] == 3
    assert agent.update_path.startswith("per step: ") and word in agent.update_path
    assert np.isfinite(objs[0]) and agent._step == 3 and agent.update_a == 2


def test_prioritised_modsac_keeps_its_per_step_loop_on_the_fused_step(monkeypatch):
    calls = _spy(monkeypatch)
    agent, buf = _with_ring((256, 256), 64, 2, steps=4, if_use_per=True, per_alpha=0.6, per_beta=0.4)
    trees0 = buf.sum_trees.sum.clone()
    objs = agent.update_net(buf)
    assert calls["per_step"] == 4 and calls["step"] == 4 and calls["layered"] == calls["loop"] == calls["ring_step"] == 0
    assert "per step" in agent.per_path and "AgentModSAC" in agent.per_path
    assert agent.update_path.startswith("per step: ") and "prioritised" in agent.update_path
    assert np.isfinite(objs[0]) and agent._step == 4 and agent.update_a == 3
    assert not th.equal(buf.sum_trees.sum, trees0)                                   # the td errors of every step reached the trees
    assert bool(th.isfinite(agent._td_error).all()) and float(agent._td_error.min()) >= 0


def test_evaluation_keeps_the_evaluators_loop():
    from elegantrl_amd.envs import PendulumVecEnv
    agent, _ = _agent((64, 64), 3, 1, num_envs=64)
    assert agent.kernel_path.startswith("fused ModSAC step")
    env = PendulumVecEnv(64, max_step=20, gpu_id=0, seed=5)
    assert agent.evaluate_env(env) is None and "ActorFixSAC" in agent._fused_eval_reason(env)


def test_checkpoint_after_a_fused_update_net(tmp_path, monkeypatch):
    calls = _spy(monkeypatch)
    agent, buf = _with_ring((64, 32), 64, 2)
    w0 = agent.act.encoder_s[0].weight.detach().clone()
    t0 = agent.act_target.encoder_s[0].weight.detach().clone()
    oc, oa = agent.update_net(buf)
    assert calls["loop"] == 1 and np.isfinite([oc, oa]).all()
    assert agent.update_a == 5 and agent._actor_step == 5 and agent._step == STEPS
    assert not th.equal(agent.act.encoder_s[0].weight, w0) and not th.equal(agent.act_target.encoder_s[0].weight, t0)
    agent.save_or_load_agent(str(tmp_path), if_save=True)
    fresh, _ = _agent((64, 32))
    fresh.save_or_load_agent(str(tmp_path), if_save=False)
    assert fresh._actor_step == agent._actor_step == 5 and fresh._step == agent._step == STEPS
    assert th.equal(fresh.act_target.encoder_s[0].weight, agent.act_target.encoder_s[0].weight)
    assert th.equal(fresh._actor_target_flat, agent._actor_target_flat) and th.equal(fresh._actor_flat, agent._actor_flat)
