"""AgentTD3 / AgentDDPG on the device (csrc/td3.hip) against tests/golden/td3_small.npz (a recorded run of the reference's AgentTD3) and
against tests/td3_ref.py in fp64.

Bounds.  Objectives rtol 2e-4 / atol 2e-6 and weights atol 3e-5: what tests/test_sac.py holds the layered SAC step to against its own
golden.  td errors rtol 3e-4 / atol 1e-6: test_sac.py's bound for the same quantity.  Gradients, read back from Adam's first moment
after the first step (exp_avg = (1 - beta1) g): the project's gradient bound 1e-4 * max|g| + 1e-7 per named tensor
(tests/sac_gradient_cases.py).  Exploration actions rtol 2e-5 / atol 2e-6: test_sac.py's bound on ActorSAC's rollout actions.  The
fp64 shape cases run at learning rate 1e-4 like the golden (tools/record_td3_golden.py says why)."""
import math
import os

import numpy as np
import pytest
import torch as th

from tests.helpers import load
from tests.td3_ref import Td3Ref, gather

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBJ_TOL = dict(rtol=2e-4, atol=2e-6)
W_ATOL = 3e-5
TD_TOL = dict(rtol=3e-4, atol=1e-6)


def _agent(cls, S, A, net, B, N=4, **extra):
    from elegantrl_amd.train import Config
    args = Config(cls, None, {"env_name": "x", "num_envs": N, "max_step": 100, "state_dim": S, "action_dim": A, "if_discrete": False})
    args.net_dims, args.batch_size, args.quiet = list(net), B, True
    for k, v in extra.items():
        setattr(args, k, v)
    return cls(args.net_dims, S, A, gpu_id=0, args=args)


def _load_from_ref(agent, ref):
    f32 = lambda net: {k: v.to(th.float32) for k, v in net.state_dict().items()}  # noqa: E731
    for mod, src in ((agent.act, ref.act), (agent.act_target, ref.act_target), (agent.cri, ref.cri), (agent.cri_target, ref.cri_target)):
        mod.load_state_dict(f32(src))
    agent._sync_modules()
    assert agent.act.net[0].weight.data_ptr() == agent._actor_flat.data_ptr()


def _assert_nets(agent, ref, what):
    for name, mine, want in (("act", agent.act, ref.act), ("act_target", agent.act_target, ref.act_target), ("cri", agent.cri, ref.cri),
                             ("cri_target", agent.cri_target, ref.cri_target)):
        for k, v in want.state_dict().items():
            np.testing.assert_allclose(mine.state_dict()[k].cpu().numpy(), v.numpy(), rtol=0, atol=W_ATOL, err_msg=f"{name}.{k} {what}")


def _state(agent):
    """everything a step may write, as clones"""
    o = (agent._actor_flat, agent._actor_target_flat, agent._critic_flat, agent._critic_target_flat, agent.act_optimizer.exp_avg,
         agent.act_optimizer.exp_avg_sq, agent.cri_optimizer.exp_avg, agent.cri_optimizer.exp_avg_sq)
    return [t.clone() for t in o]


class _ReplayEnv:
    """replays the recorded env transitions of the golden rollout (device tensors, the reference's 5-tuple protocol)"""

    def __init__(self, g, reward_scale):
        self.g, self.t, self.scale = g, 0, reward_scale
        self.num_envs = g["ro_states"].shape[1]

    def step(self, action):
        g, t = self.g, self.t
        nxt = g["ro_states"][t + 1] if t + 1 < g["ro_states"].shape[0] else g["ro_last_state"]
        self.t += 1
        to = lambda a: th.from_numpy(a).to(DEV)  # noqa: E731
        return to(nxt), to(g["ro_rewards"][t] / self.scale), to(~g["ro_undones"][t]), to(~g["ro_unmasks"][t]), {}


# ---- 1. golden replay ---------------------------------------------------------------------------------------------------------
def test_rollout_and_four_updates_replay_the_reference_and_fp64():
    from elegantrl_amd.agents import AgentTD3
    from elegantrl_amd.train import ReplayBuffer
    g = load("td3_small.npz")
    N, S, A, rows, B, n_upd, E, freq, h1, h2 = [int(x) for x in g["dims"]]
    gamma, lr, max_norm, reward_scale, tau, policy_noise, explore_noise = [float(x) for x in g["hyper"]]
    agent = _agent(AgentTD3, S, A, (h1, h2), B, N=N, learning_rate=lr, gamma=gamma, reward_scale=reward_scale, soft_update_tau=tau,
                   clip_grad_norm=max_norm, num_ensembles=E, update_freq=freq, policy_noise_std=policy_noise, explore_noise_std=explore_noise)
    ref = Td3Ref([h1, h2], S, A, E, lr=lr, gamma=gamma, tau=tau, max_norm=max_norm, policy_noise_std=policy_noise)
    ref.load({k[5:]: v for k, v in g.items() if k.startswith("act0.")}, {k[5:]: v for k, v in g.items() if k.startswith("cri0.")})
    _load_from_ref(agent, ref)

    # the off-policy rollout: stored action = the clipped action, rewards scaled, flags inverted
    agent.last_state = th.from_numpy(g["first_state"]).to(DEV)
    items = agent._explore_vec_env(_ReplayEnv(g, reward_scale), rows, noise=th.from_numpy(g["ro_eps"]).to(DEV))
    assert agent.rollout_path.startswith("per-step loop (erl_td3_explore_action_f32")
    for got, name in zip(items, ("ro_states", "ro_actions", "ro_rewards", "ro_undones", "ro_unmasks")):
        if got.dtype == th.bool:
            np.testing.assert_array_equal(got.cpu().numpy(), g[name])
        else:
            np.testing.assert_allclose(got.cpu().numpy(), g[name], rtol=2e-5, atol=2e-6)
    np.testing.assert_array_equal(agent.last_state.cpu().numpy(), g["ro_last_state"])

    buf = ReplayBuffer(max_size=rows + 5, state_dim=S, action_dim=A, gpu_id=0, num_seqs=N)
    buf.update(tuple(th.from_numpy(g[n]).to(DEV) for n in ("ro_states", "ro_actions", "ro_rewards", "ro_undones", "ro_unmasks")))
    ring = {k: g[f"ro_{k}"] for k in ("states", "actions", "rewards", "undones", "unmasks")}
    objs, td = th.zeros(2, device=DEV), th.zeros(B, device=DEV)
    for t in range(n_upd):
        upd = t % freq == 0
        before = _state(agent)
        steps_before = (agent._actor_step, agent.act_optimizer.step_count)
        batch = buf.sample(B, ids=th.from_numpy(g["ids"][t]).to(DEV))
        agent._update_on_batch(batch, objs, agent._update_actor(buf, t), th.from_numpy(g["noise"][t]).to(DEV), td_error_out=td)
        oc, oa = objs.cpu().tolist()
        rc, ra, rtd = ref.step(gather(ring, g["ids"][t], rows - 1)[0], g["noise"][t], upd)
        print(f"step {t}: device ({oc:.8f}, {oa:.8f}) fp64 ({rc:.8f}, {ra:.8f}) recorded {g['objs'][t]}")
        np.testing.assert_allclose(oc, g["objs"][t][0], **OBJ_TOL)
        np.testing.assert_allclose(oc, rc, **OBJ_TOL)
        np.testing.assert_allclose(td.cpu().numpy(), rtd.numpy(), **TD_TOL)
        if upd:
            np.testing.assert_allclose(oa, g["objs"][t][1], **OBJ_TOL)
            np.testing.assert_allclose(oa, ra, **OBJ_TOL)
        else:               # nan, and the actor, its target and its moments bit-unchanged
            assert math.isnan(oa) and math.isnan(g["objs"][t][1])
            after = _state(agent)
            for i in (0, 1, 4, 5):
                assert th.equal(before[i], after[i]), i
            assert (agent._actor_step, agent.act_optimizer.step_count) == steps_before
        for prefix, net in ((f"act{t + 1}", agent.act), (f"actt{t + 1}", agent.act_target), (f"cri{t + 1}", agent.cri), (f"crit{t + 1}", agent.cri_target)):
            for k, v in net.state_dict().items():
                np.testing.assert_allclose(v.cpu().numpy(), g[f"{prefix}.{k}"], rtol=0, atol=W_ATOL, err_msg=f"{prefix}.{k}")
        _assert_nets(agent, ref, f"after step {t}")
    assert (agent._step, agent._actor_step) == (4, 2)


# ---- 2. shapes where the kernels can go wrong, against fp64 -----------------------------------------------------------------------
def _crit(name):
    return {"mse": None, "smooth_l1": th.nn.SmoothL1Loss(reduction="none", beta=0.05), "huber": th.nn.HuberLoss(reduction="none", delta=0.05)}[name]


SHAPES = [  # id, agent, S, A, net, E, B, criterion, is_weight
    ("full-block-plus-tail-E8", "td3", 11, 3, (64, 32), 8, 300, "mse", False),
    ("E2", "td3", 11, 3, (64, 32), 2, 300, "mse", False),
    ("E1", "td3", 11, 3, (64, 32), 1, 300, "mse", False),
    ("ddpg", "ddpg", 11, 3, (64, 32), 1, 300, "mse", False),
    ("pendulum-A1-S3", "td3", 3, 1, (32, 16), 8, 65, "mse", False),
    ("three-layers", "td3", 17, 6, (64, 48, 32), 2, 130, "mse", False),
    ("smooth-l1", "td3", 11, 3, (64, 32), 8, 70, "smooth_l1", False),
    ("huber", "ddpg", 11, 3, (64, 32), 1, 70, "huber", False),
    ("is-weight-with-zeros", "td3", 11, 3, (64, 32), 8, 300, "mse", True),
]


@pytest.mark.parametrize("kind,S,A,net,E,B,crit,weighted", [c[1:] for c in SHAPES], ids=[c[0] for c in SHAPES])
def test_step_matches_fp64(kind, S, A, net, E, B, crit, weighted):
    from elegantrl_amd.agents import AgentDDPG, AgentTD3
    cls = AgentTD3 if kind == "td3" else AgentDDPG
    lr, gamma, tau, max_norm, std = 1e-4, 0.97, 5e-3, 3.0, (0.2 if kind == "td3" else 0.0)
    extra = dict(learning_rate=lr, gamma=gamma, soft_update_tau=tau, clip_grad_norm=max_norm, num_ensembles=E, update_freq=1, policy_noise_std=std)
    if crit != "mse":
        extra["criterion"] = _crit(crit)
    agent = _agent(cls, S, A, net, B, **extra)
    assert agent.num_ensembles == E and agent.policy_noise_std == std
    ref = Td3Ref(list(net), S, A, E, lr=lr, gamma=gamma, tau=tau, max_norm=max_norm, policy_noise_std=std, criterion=_crit(crit), seed=11)
    with th.no_grad():                                    # targets that differ from the current nets
        for tar in (ref.act_target, ref.cri_target):
            for p in tar.parameters():
                p.mul_(0.9)
    _load_from_ref(agent, ref)
    rng = np.random.default_rng(5)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    w = None
    if weighted:
        w = rng.uniform(0.2, 1.0, B).astype(np.float32)
        w[::7] = 0.0
    objs, td = th.zeros(2, device=DEV), th.zeros(B, device=DEV)
    for t in range(2):
        batch = (f(B, S), np.clip(f(B, A), -1, 1), f(B), (rng.random(B) > 0.15).astype(np.float32), (rng.random(B) > 0.15).astype(np.float32),
                 f(B, S))
        if crit != "mse":                                  # both arms of the piecewise losses occur
            batch = (*batch[:2], batch[2] * 0.2, *batch[3:])
        noise = f(B, A) * 3.0                              # some actions leave [-1, 1] before the clip
        agent._update_on_batch(tuple(th.from_numpy(x).to(DEV) for x in batch), objs, True, th.from_numpy(noise).to(DEV),
                               is_weight=None if w is None else th.from_numpy(w).to(DEV), td_error_out=td)
        oc, oa = objs.cpu().tolist()
        rc, ra, rtd = ref.step(batch, noise, True, is_weight=w)
        print(f"step {t}: device ({oc:.8f}, {oa:.8f}) fp64 ({rc:.8f}, {ra:.8f})")
        np.testing.assert_allclose([oc, oa], [rc, ra], **OBJ_TOL)
        np.testing.assert_allclose(td.cpu().numpy(), rtd.numpy(), **TD_TOL)
        if crit != "mse":
            a = np.abs(rtd.numpy())
            assert (a > 0).any()
        if t == 0:                                         # the clipped gradients of the first step, from Adam's first moment
            for name, opt, ropt, rnet, slices in (("actor", agent.act_optimizer, ref.act_opt, ref.act, agent._spec.actor_slices()),
                                                  ("critic", agent.cri_optimizer, ref.cri_opt, ref.cri, agent._spec.critic_slices())):
                named = dict(rnet.named_parameters())
                for pname, off, shape in slices:
                    want = ropt.state[named[pname]]["exp_avg"].numpy() / 0.1
                    got = opt.exp_avg[off:off + want.size].view(shape).cpu().numpy().astype(np.float64) / 0.1
                    scale = np.abs(want).max()
                    assert scale > 0, f"{name}.{pname}: the case exercises no gradient here"
                    err = np.abs(got - want).max()
                    assert err <= 1e-4 * scale + 1e-7, f"{name}.{pname}: gradient off by {err:.3e}, bound {1e-4 * scale + 1e-7:.3e}"
        _assert_nets(agent, ref, f"after step {t}")


# ---- 3. the one-call loop against the per-step route ---------------------------------------------------------------------------
def _filled_buffer(N, S, A, rows, seed=3, **kw):
    from elegantrl_amd.train import ReplayBuffer
    g = th.Generator().manual_seed(seed)
    buf = ReplayBuffer(max_size=rows + 7, state_dim=S, action_dim=A, gpu_id=0, num_seqs=N, **kw)
    buf.update((th.randn(rows, N, S, generator=g).to(DEV), th.rand(rows, N, A, generator=g).mul(2).sub(1).to(DEV),
                th.randn(rows, N, generator=g).to(DEV), (th.rand(rows, N, generator=g) > 0.1).to(DEV), (th.rand(rows, N, generator=g) > 0.1).to(DEV)))
    return buf


def _two_routes(cls, **extra):
    """the same agent twice -- per-step route, one-call loop -- on one buffer, with the same id draws"""
    N, S, A, rows, B = 4, 11, 3, 40, 64
    out = []
    for loop in (False, True):
        th.manual_seed(123)
        agent = _agent(cls, S, A, (64, 32), B, N=N, repeat_times=10.0, td3_loop_in_c=loop, learning_rate=1e-3, **extra)
        buf = _filled_buffer(N, S, A, rows)
        assert int(buf.cur_size * agent.repeat_times / B) == 6
        th.manual_seed(77)
        logs = agent.update_net(buf)
        out.append((agent, buf, logs))
    (a, abuf, alog), (b, bbuf, blog) = out
    assert a.update_path.startswith("per step: args.td3_loop_in_c is off") and b.update_path.startswith("one C call (erl_td3_update_ring_loop_f32")
    for x, y in zip(_state(a), _state(b)):
        assert th.equal(x, y)
    assert (a._step, a._actor_step, a.act_optimizer.step_count, a.cri_optimizer.step_count) == (b._step, b._actor_step, b.act_optimizer.step_count,
                                                                                           b.cri_optimizer.step_count)
    oa, ob = a.objs_all.cpu().numpy(), b.objs_all.cpu().numpy()
    np.testing.assert_array_equal(oa, ob)                                     # (nan rows compare equal here)
    assert th.equal(abuf.ids0, bbuf.ids0) and th.equal(abuf.ids1, bbuf.ids1) and abuf.ids0.numel() == B
    assert alog == blog or (math.isnan(alog[1]) and math.isnan(blog[1]))
    return a, oa


@pytest.mark.parametrize("freq", [2, 3])
def test_td3_loop_is_bit_identical_to_the_per_step_route(freq):
    from elegantrl_amd.agents import AgentTD3
    a, objs = _two_routes(AgentTD3, update_freq=freq)
    assert a._step == 6 and a._actor_step == len(range(0, 6, freq)) == a.act_optimizer.step_count
    np.testing.assert_array_equal(np.isnan(objs[:, 1]), [t % freq != 0 for t in range(6)])
    assert np.isfinite(objs[:, 0]).all()


@pytest.mark.parametrize("init_size,updates", [(40, True), (41, False)], ids=["at-the-threshold", "below-it"])
def test_ddpg_loop_is_bit_identical_on_both_sides_of_buffer_init_size(init_size, updates):
    from elegantrl_amd.agents import AgentDDPG
    a, objs = _two_routes(AgentDDPG, buffer_init_size=init_size)
    assert a._step == 6 and a._actor_step == (6 if updates else 0)
    assert np.isnan(objs[:, 1]).all() != updates and np.isnan(objs[:, 1]).any() != updates
    if not updates:                                                           # the actor never moved, its target neither
        assert th.equal(a._actor_flat, a._actor_target_flat) and not a.act_optimizer.exp_avg.any()


def test_prioritised_and_planar_rings_take_the_per_step_route():
    from elegantrl_amd.agents import AgentTD3
    from elegantrl_amd.train import Config
    N, S, A, rows, B = 4, 11, 3, 40, 64
    agent = _agent(AgentTD3, S, A, (64, 32), B, N=N, repeat_times=4.0, td3_loop_in_c=True, if_use_per=True)
    cfg = Config(AgentTD3, None, None)
    cfg.per_alpha, cfg.per_beta = 0.6, 0.4
    buf = _filled_buffer(N, S, A, rows, if_use_per=True, args=cfg)
    oc, oa = agent.update_net(buf)
    assert agent.update_path.startswith("per step: prioritised replay") and math.isfinite(oc) and math.isfinite(oa)
    assert agent._td_error is not None and bool(th.isfinite(agent._td_error).all()) and agent._step == 2
    cfg.replay_interleaved = False
    agent = _agent(AgentTD3, S, A, (64, 32), B, N=N, repeat_times=4.0, td3_loop_in_c=True)
    oc, oa = agent.update_net(_filled_buffer(N, S, A, rows, args=cfg))
    assert agent.update_path.startswith("per step: planar replay ring") and math.isfinite(oc) and math.isfinite(oa)


# ---- 4. exploration ------------------------------------------------------------------------------------------------------------
def test_explore_action_with_injected_noise_matches_fp64():
    from elegantrl_amd.agents import AgentDDPG, AgentTD3
    for cls, key, S, A, N in ((AgentTD3, "explore_noise_std", 11, 3, 300), (AgentDDPG, "explore_noise", 3, 1, 5)):
        agent = _agent(cls, S, A, (64, 32), 64, N=N, **{key: 0.4})
        ref = Td3Ref([64, 32], S, A, agent.num_ensembles, lr=1e-4, gamma=0.99, tau=5e-3, max_norm=3.0, policy_noise_std=0.0, seed=2)
        _load_from_ref(agent, ref)
        g = th.Generator().manual_seed(9)
        state, noise = th.randn(N, S, generator=g), th.randn(N, A, generator=g) * 3
        out_state = th.zeros(N, S, device=DEV)
        got = agent.explore_action(state.to(DEV), noise.to(DEV), out_state=out_state)
        with th.no_grad():
            want = ref.policy(state, 0.4, noise)
        assert (want.abs() == 1).any() or N < 10                               # the clip is exercised
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-6)
        assert th.equal(out_state.cpu(), state) and agent.rng_counter == 1 and float(got.abs().max()) <= 1.0


def test_philox_draws_are_reproducible_and_independent_of_the_launch_geometry():
    from elegantrl_amd import ops
    from elegantrl_amd.agents import AgentTD3
    S, A = 11, 3
    agent = _agent(AgentTD3, S, A, (64, 32), 64, N=4096, explore_noise_std=0.5)
    g = th.Generator().manual_seed(4)
    state = th.randn(4096, S, generator=g).to(DEV)
    draw = lambda rows, counter, seed=agent.rng_seed: ops.td3_explore_action(agent._spec, agent._actor_flat, state[:rows].contiguous(), 0.5,  # noqa: E731
                                                                             seed=seed, counter=counter)
    big, small, again = draw(4096, 3), draw(5, 3), draw(4096, 3)
    assert th.equal(big, again) and th.equal(big[:5], small)
    other_counter, other_seed, mean = draw(4096, 4), draw(4096, 3, seed=agent.rng_seed + 1), agent.act(state).detach()
    assert not th.equal(big, other_counter) and not th.equal(big, other_seed)
    eps = ((big - mean) / 0.5)[(big.abs() < 1)]                                # where the clip did not act: the draws themselves
    assert abs(float(eps.mean())) < 0.05 and 0.8 < float(eps.std()) < 1.1
    a0 = agent.explore_action(state)                                           # the agent's own counter advances per call
    assert th.equal(a0, draw(4096, 0)) and not th.equal(agent.explore_action(state), a0) and agent.rng_counter == 2


def test_single_numpy_env_rollout():
    from elegantrl_amd.agents import AgentDDPG
    from tests.helpers import ToySingleEnv
    env = ToySingleEnv()
    agent = _agent(AgentDDPG, env.state_dim, env.action_dim, (32, 16), 64, N=1, reward_scale=0.5)
    agent.last_state = th.as_tensor(env.reset()[0], dtype=th.float32, device=DEV).unsqueeze(0)
    states, actions, rewards, undones, unmasks = agent.explore_env(env, 10)
    assert states.shape == (10, 1, 3) and actions.shape == (10, 1, 2) and rewards.shape == undones.shape == unmasks.shape == (10, 1)
    assert "one numpy env" in agent.rollout_path and agent.rng_counter == 10 and float(actions.abs().max()) <= 1.0
    assert bool(undones.all()) and not bool(unmasks.all())                     # the toy env only truncates
    np.testing.assert_allclose(rewards.cpu().numpy(), 0.5 * (1.0 - actions.abs().mean(dim=2).cpu().numpy()), rtol=1e-6)


# ---- 5. training run, checkpoint -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["AgentTD3", "AgentDDPG"])
def test_train_agent_on_pendulum_and_resume(name, tmp_path):
    import elegantrl_amd.agents as agents
    from elegantrl_amd import train_agent
    from elegantrl_amd.envs import PendulumVecEnv
    from elegantrl_amd.train import Config
    cls = getattr(agents, name)
    args = Config(cls, PendulumVecEnv, {"env_name": "Pendulum-v1", "num_envs": 16, "max_step": 200, "state_dim": 3, "action_dim": 1,
                                        "if_discrete": False})
    args.net_dims, args.quiet = [64, 32], True
    args.horizon_len, args.batch_size, args.repeat_times, args.buffer_size, args.buffer_init_size = 24, 64, 8.0, 4096, 40
    args.break_step, args.eval_per_step, args.eval_times = 24 * 2, 24, 2          # three iterations, evaluated
    args.cwd, args.gpu_id, args.random_seed = str(tmp_path / "run"), 0, 0
    train_agent(args, if_single_process=True)
    files = os.listdir(args.cwd)
    for f in ("act.pth", "act_target.pth", "act_optimizer.pth", "cri.pth", "cri_target.pth", "cri_optimizer.pth", "recorder.npy"):
        assert f in files, (f, files)
    rec = np.load(os.path.join(args.cwd, "recorder.npy"))
    assert rec.shape[0] >= 2 and np.isfinite(rec[:, :6]).all(), rec
    actor = th.load(os.path.join(args.cwd, "act.pth"), weights_only=False)
    assert actor(th.zeros((2, 3), device=DEV)).shape == (2, 1)

    # a resumed agent reproduces the next step bit for bit: X goes on, Y is loaded from X's checkpoint and takes the same step
    th.manual_seed(1)
    x = cls(args.net_dims, 3, 1, gpu_id=0, args=args)
    x.save_or_load_agent(args.cwd, if_save=False)
    assert x._step == sum(int(24 * k * 8.0 / 64) for k in (1, 2, 3))            # the run's three update_net loops, from the checkpoint
    buf = _filled_buffer(16, 3, 1, 48)
    th.manual_seed(5)
    x.update_net(buf)                                                           # X moves on from the run's checkpoint ...
    os.makedirs(tmp_path / "ckpt")
    x.save_or_load_agent(str(tmp_path / "ckpt"), if_save=True)                  # ... and is saved mid-way
    y = cls(args.net_dims, 3, 1, gpu_id=0, args=args)
    y.save_or_load_agent(str(tmp_path / "ckpt"), if_save=False)
    assert (y._step, y._actor_step, y.rng_counter) == (x._step, x._actor_step, x.rng_counter) and y._actor_step > 0
    for a, b in zip(_state(x), _state(y)):
        assert th.equal(a, b)
    ids = th.randint((buf.cur_size - 1) * buf.num_seqs, (64,), device=DEV)
    ox, oy = x.update_objectives(buf, 0, ids=ids), y.update_objectives(buf, 0, ids=ids)
    assert ox == oy and all(math.isfinite(v) for v in ox)
    for a, b in zip(_state(x), _state(y)):
        assert th.equal(a, b)
    assert th.equal(x.explore_action(buf.states[0].contiguous()), y.explore_action(buf.states[0].contiguous()))
