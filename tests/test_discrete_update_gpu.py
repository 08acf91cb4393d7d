"""The fused discrete minibatch kernel and its one-call update loop (csrc/ppo_step_discrete.hip): one step's gradients and logged
objectives against the fp64 numpy oracle at the tolerances the layered discrete step is held to (tests/test_discrete_gpu.py), the edges
of the categorical head, the C loop against a Python loop of its own steps (bit for bit), the agents on the fused route against the
reference's recorded run (tests/golden/ppo_discrete_small.npz), routing between the fused and the layered route, and a checkpoint
round trip."""
import numpy as np
import pytest
import torch as th

from oracle import ppo_numpy as O
from tests.helpers import hyper, load
from tests.test_discrete_gpu import discrete_case, spread
from tests.test_kernels_gpu import cu, flat_params
from tests.test_mlpn_gpu import random_net_n

pytestmark = pytest.mark.gpu
DEV = th.device("cuda:0")
# S not a multiple of 4 or 16, A not a multiple of 4, both extremes of width; (4, (64, 32), 2) is CartPole's compile-time instantiation
SHAPES = [(4, (64, 32), 2), (6, (64, 32), 4), (17, (32, 32), 3), (64, (128, 128), 8), (5, (96, 64), 5)]
H, N = 9, 50          # 450 rows: ids repeat from B = 1000 on


@pytest.fixture(scope="module")
def ops():
    from elegantrl_amd import ops as _ops
    return _ops


def run_step(ops, actor, critic, case, S, hidden, A, lam=0.01, clip=0.25):
    """erl_ppo_step_discrete_f32 + erl_grad_reduce_f32 -> (gradient row, slabs) as float64 / float32 numpy"""
    states, actions, um, lp, adv, rs, ids = case
    B = ids.shape[0]
    stride, n_slabs = ops.ppo_discrete_slab_stride(S, *hidden, A), ops.ppo_num_slabs(B)
    slabs = th.full((n_slabs, stride), float("nan"), device=DEV)
    ops.ppo_step_discrete(cu(flat_params(actor), DEV), cu(flat_params(critic), DEV), cu(actor.state_avg, DEV), cu(actor.state_std, DEV),
                          cu(critic.state_avg, DEV), cu(critic.state_std, DEV), S, hidden[0], hidden[1], A, cu(states, DEV),
                          cu(actions, DEV), cu(um, DEV), cu(lp, DEV), cu(adv, DEV), cu(rs, DEV), cu(ids, DEV), clip, lam, 1.0 / B, slabs,
                          n_slabs)
    row = th.full((stride,), float("nan"), device=DEV)
    ops.grad_reduce(slabs, n_slabs, stride, row)
    return row.cpu().numpy().astype(np.float64), slabs.cpu().numpy()


def oracle_step(actor, critic, case, lam=0.01, clip=0.25):
    states, actions, um, lp, adv, rs, ids = case
    dt = np.float64
    i0, i1 = O.split_ids(ids, states.shape[0])
    s = states[i0, i1].astype(dt)
    oc, gw, gb = O.critic_objective(s, rs[i0, i1].astype(dt), um[i0, i1], critic.astype(dt))
    gc = np.concatenate([x.reshape(-1) for pair in zip(gw, gb) for x in pair])
    os_, oe, gw, gb = O.actor_objective_discrete(s, actions[i0, i1], lp[i0, i1].astype(dt), adv[i0, i1].astype(dt), um[i0, i1],
                                                 actor.astype(dt), clip, lam)
    ga = np.concatenate([x.reshape(-1) for pair in zip(gw, gb) for x in pair])
    return ga, gc, (oc, os_, oe)


def check_against_oracle(got, slabs, ref, Pa, Pc):
    ga, gc, logs = ref
    assert np.isfinite(got).all() and np.isfinite(slabs).all()
    assert (slabs[:, Pa + Pc + 4:] == 0).all() and (got[Pa + Pc + 3:] == 0).all()        # the 4th log and the pad of every row
    for name, g, r in (("actor", got[:Pa], ga), ("critic", got[Pa:Pa + Pc], gc)):
        scale, err = np.abs(r).max(), np.abs(g - r).max()
        print(f"{name} grad err {err:.3e} (scale {scale:.3e}, bound {1e-4 * scale + 1e-7:.3e})")
        assert err <= 1e-4 * scale + 1e-7, f"{name} grad err {err:.3e} (scale {scale:.3e})"
    print("logs", got[Pa + Pc:Pa + Pc + 3], logs)
    np.testing.assert_allclose(got[Pa + Pc:Pa + Pc + 3], logs, rtol=1e-4, atol=1e-6)


# ---- 1. gradients of one step against the fp64 oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("S,hidden,A", SHAPES)
@pytest.mark.parametrize("B", [64, 128, 1000, 1300])
def test_step_gradients_match_oracle(ops, S, hidden, A, B):
    rng = np.random.default_rng(S + B + A)
    case = discrete_case(rng, H, N, S, A, B)
    actor, critic = spread(random_net_n(rng, [S, *hidden, A], False), 3.0), random_net_n(rng, [S, *hidden, 1], False)
    Pa, Pc = ops.MlpSpecN([S, *hidden, A], False).count, ops.MlpSpecN([S, *hidden, 1], False).count
    got, slabs = run_step(ops, actor, critic, case, S, hidden, A)
    check_against_oracle(got, slabs, oracle_step(actor, critic, case), Pa, Pc)


# ---- 2. edges of the head ----------------------------------------------------------------------------------------------------------
def test_all_rows_masked_gives_exact_zeros(ops):
    S, hidden, A, B = 6, (64, 32), 4, 200
    rng = np.random.default_rng(11)
    states, actions, um, lp, adv, rs, ids = discrete_case(rng, H, N, S, A, B)
    case = (states, actions, np.zeros_like(um), lp, adv, rs, ids)
    actor, critic = spread(random_net_n(rng, [S, *hidden, A], False), 3.0), random_net_n(rng, [S, *hidden, 1], False)
    Pa, Pc = ops.MlpSpecN([S, *hidden, A], False).count, ops.MlpSpecN([S, *hidden, 1], False).count
    got, slabs = run_step(ops, actor, critic, case, S, hidden, A)
    assert np.isfinite(slabs).all()
    assert (got[:Pa] == 0).all(), "actor gradient of a fully masked minibatch"
    assert got[Pa + Pc + 1] == 0 and got[Pa + Pc + 2] == 0 and got[Pa + Pc] == 0      # surrogate, entropy, critic loss
    assert (got[Pa:Pa + Pc] == 0).all()


def test_probability_under_the_clamp(ops):
    """one action's logit sits 40 below the rest (p ~ 4e-18, far under eps = 2^-23): its log-prob is the clamp's constant, so rows that
    took it pass no gradient through the log-prob, and its entropy term passes none either"""
    S, hidden, A, B = 6, (64, 32), 3, 300
    rng = np.random.default_rng(12)
    case = discrete_case(rng, H, N, S, A, B)
    actor, critic = random_net_n(rng, [S, *hidden, A], False), random_net_n(rng, [S, *hidden, 1], False)
    actor.biases[-1][1] -= np.float32(40.0)
    states, actions, um, lp, adv, rs, ids = case
    i0, i1 = O.split_ids(ids, H)
    p = O.softmax(O.actor_mean(states[i0, i1].astype(np.float64), actor.astype(np.float64)))
    eps = float(np.finfo(np.float32).eps)
    for v in (p, 1.0 - p):          # no probability of any row within a factor 10 of eps or of 1 - eps: no row is ambiguous, none is left out
        assert not ((v > eps / 10) & (v < eps * 10)).any()
    assert (p[:, 1] < eps / 10).all() and (actions[i0, i1] == 1).sum() > 30
    Pa, Pc = ops.MlpSpecN([S, *hidden, A], False).count, ops.MlpSpecN([S, *hidden, 1], False).count
    got, slabs = run_step(ops, actor, critic, case, S, hidden, A)
    check_against_oracle(got, slabs, oracle_step(actor, critic, case), Pa, Pc)
    # every row took the suppressed action and the entropy term is off: nothing reaches the actor, while the surrogate is logged
    only = (states, np.ones_like(actions), um, lp, adv, rs, ids)
    got, slabs = run_step(ops, actor, critic, only, S, hidden, A, lam=0.0)
    assert (got[:Pa] == 0).all() and got[Pa + Pc + 1] != 0
    check_against_oracle(got, slabs, oracle_step(actor, critic, only, lam=0.0), Pa, Pc)


# ---- 3. the loop is the steps ------------------------------------------------------------------------------------------------------
def test_update_loop_is_bitwise_the_python_loop_of_its_steps(ops):
    S, hidden, A, B, K = 4, (64, 32), 2, 200, 3
    rng = np.random.default_rng(13)
    states, actions, um, lp, adv, rs, _ = discrete_case(rng, H, N, S, A, B)
    ids = rng.integers(0, H * N, (K, B)).astype(np.int64)
    actor, critic = spread(random_net_n(rng, [S, *hidden, A], False), 3.0), random_net_n(rng, [S, *hidden, 1], False)
    Pa, Pc = ops.MlpSpecN([S, *hidden, A], False).count, ops.MlpSpecN([S, *hidden, 1], False).count
    stride, n_slabs = ops.ppo_discrete_slab_stride(S, *hidden, A), ops.ppo_num_slabs(B)
    avg, sd = cu(actor.state_avg, DEV), cu(actor.state_std, DEV)
    buf = [cu(x, DEV) for x in (states, actions, um, lp, adv, rs)]
    ids_d = cu(ids, DEV)
    lr, max_norm, first = 1e-3, 0.5, 7          # (a norm bound that clips)
    groups = [(0, Pa), (Pa, Pc)]

    def fresh():
        flat = cu(np.concatenate([flat_params(actor), flat_params(critic)]), DEV)
        m1 = cu(0.01 * rng0.standard_normal(Pa + Pc).astype(np.float32), DEV)
        m2 = cu((1e-4 * rng0.random(Pa + Pc)).astype(np.float32), DEV)
        return flat, m1, m2, th.full((n_slabs, stride), float("nan"), device=DEV), th.full((K, stride), float("nan"), device=DEV)

    rng0 = np.random.default_rng(14)
    flat, m1, m2, slabs, grads = fresh()
    ops.ppo_update_discrete(flat, m1, m2, avg, sd, avg, sd, S, hidden[0], hidden[1], A, *buf, ids_d, 0.25, 0.01, slabs, grads, first, lr,
                            max_norm)
    rng0 = np.random.default_rng(14)
    flat2, m1b, m2b, slabs2, grads2 = fresh()
    for k in range(K):
        ops.ppo_step_discrete(flat2[:Pa], flat2[Pa:], avg, sd, avg, sd, S, hidden[0], hidden[1], A, *buf, ids_d[k], 0.25, 0.01, 1.0 / B,
                              slabs2, n_slabs)
        ops.grad_reduce(slabs2, n_slabs, stride, grads2[k])
        ops.grad_sq_partials(grads2[k], stride, groups, 1.0)
        ops.clip_adam_partials(flat2, grads2[k], m1b, m2b, stride, groups, first + k, lr, max_norm)
    for name, x, y in (("params", flat, flat2), ("exp_avg", m1, m1b), ("exp_avg_sq", m2, m2b), ("grads", grads, grads2)):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=name)
    assert np.isfinite(flat.cpu().numpy()).all() and np.abs(flat.cpu().numpy()[:Pa] - flat_params(actor)).max() > 1e-4


# ---- 4. the agents against the reference's recorded run ----------------------------------------------------------------------------
def make_agent(g, cls, fused=True, **extra):
    from elegantrl_amd.train import Config
    hp = hyper(g)
    n, S, A, h, B, n_upd, _, *net = [int(x) for x in g["dims"]]
    args = Config(cls, None, {"env_name": "golden", "num_envs": n, "max_step": 100, "state_dim": S, "action_dim": A, "if_discrete": True})
    args.net_dims = extra.get("net", net)
    args.horizon_len, args.batch_size, args.repeat_times = h, B, n_upd * B / h
    args.learning_rate, args.gamma, args.reward_scale, args.clip_grad_norm = hp["lr"], hp["gamma"], hp["reward_scale"], hp["max_norm"]
    args.lambda_gae_adv, args.ratio_clip, args.lambda_entropy = hp["lam"], hp["ratio_clip"], hp["lambda_entropy"]
    args.quiet = True
    if fused is not None:
        args.fused_update = fused
    th.manual_seed(0)
    agent = cls(args.net_dims, S, A, gpu_id=0, args=args)
    if "net" not in extra:
        with th.no_grad():
            for net_, prefix in ((agent.act, "act0"), (agent.cri, "cri0")):
                net_.load_state_dict({k[len(prefix) + 1:]: th.from_numpy(v) for k, v in g.items() if k.startswith(prefix + ".")})
    agent.last_state = th.from_numpy(g["last_state"]).to(DEV)
    return agent


def golden_buffer(g):
    return [th.from_numpy(g[k]).to(DEV) for k in ("states", "actions", "logprobs", "rewards", "undones", "unmasks")]


@pytest.mark.parametrize("cls", ["AgentDiscretePPO", "AgentDiscreteA2C"])
def test_agent_fused_update_matches_reference_weights_and_objectives(cls):
    import elegantrl_amd.agents as agents
    g = load("ppo_discrete_small.npz")
    agent = make_agent(g, getattr(agents, cls))
    assert not agent._fused and agent.fused_update_discrete
    objs = agent.update_net(golden_buffer(g), ids=th.from_numpy(g["ids"]).to(DEV))
    assert agent.update_path == "fused"
    np.testing.assert_allclose(np.array(objs), g["objs"], rtol=5e-4, atol=5e-6)
    for net, prefix in ((agent.act, "act1"), (agent.cri, "cri1")):
        for k, v in net.state_dict().items():
            np.testing.assert_allclose(v.cpu().numpy(), g[f"{prefix}.{k}"], rtol=0, atol=3e-5, err_msg=f"{prefix}.{k}")
    assert np.abs(agent.act.net[0].weight.detach().cpu().numpy() - g["act0.net.0.weight"]).max() > 1e-4


# ---- 5. routing --------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def spies(monkeypatch):
    from elegantrl_amd import ops as _ops
    calls = {"layered": 0, "fused": 0}
    lay, fus = _ops.mlpn_ppo_step_discrete, _ops.ppo_update_discrete

    def lay_spy(*a, **k):
        calls["layered"] += 1
        return lay(*a, **k)

    def fus_spy(*a, **k):
        calls["fused"] += 1
        return fus(*a, **k)

    monkeypatch.setattr(_ops, "mlpn_ppo_step_discrete", lay_spy)
    monkeypatch.setattr(_ops, "ppo_update_discrete", fus_spy)
    return calls


def test_routing_between_the_fused_and_the_layered_loop(spies, monkeypatch):
    from elegantrl_amd import parallel
    from elegantrl_amd.agents import AgentDiscretePPO
    g = load("ppo_discrete_small.npz")
    ids = th.from_numpy(g["ids"]).to(DEV)
    n_upd = ids.shape[0]

    def run(agent):
        spies["layered"] = spies["fused"] = 0
        agent.last_state = th.from_numpy(g["last_state"]).to(DEV)
        agent.update_net(golden_buffer(g), ids=ids)
        return agent.update_path, spies["layered"], spies["fused"]

    on = make_agent(g, AgentDiscretePPO, True)
    assert run(on) == ("fused", 0, 1)
    assert run(on) == ("fused", 0, 1)                                            # once per update_net
    assert run(make_agent(g, AgentDiscretePPO, False)) == ("layered", n_upd, 0)
    assert run(make_agent(g, AgentDiscretePPO, True, net=[256, 128])) == ("layered", n_upd, 0)
    monkeypatch.setattr(parallel, "force_dp", lambda: True)                      # the data-parallel code path with one rank ...
    monkeypatch.setattr(parallel, "gradient_comm", lambda count=None: None)      # ... on the torch.distributed route (identity here)
    assert run(on) == ("layered", n_upd, 0)


def test_lazy_logs_on_the_fused_route_equal_the_eager_values():
    from elegantrl_amd.agents import AgentDiscretePPO
    from elegantrl_amd.agents.AgentPPO import PendingLogs
    g = load("ppo_discrete_small.npz")
    ids = th.from_numpy(g["ids"]).to(DEV)
    eager = make_agent(g, AgentDiscretePPO).update_net(golden_buffer(g), ids=ids)
    twin = make_agent(g, AgentDiscretePPO)
    pending = twin.update_net(golden_buffer(g), ids=ids, lazy=True)
    assert isinstance(pending, PendingLogs) and twin.update_path == "fused"
    assert tuple(pending.result()) == tuple(eager)


# ---- 6. checkpoint round trip ------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_on_the_fused_route(tmp_path):
    from elegantrl_amd.agents import AgentDiscretePPO
    g = load("ppo_discrete_small.npz")
    ids = th.from_numpy(g["ids"]).to(DEV)
    first = make_agent(g, AgentDiscretePPO)
    first.update_net(golden_buffer(g), ids=ids)
    first.save_or_load_agent(str(tmp_path), if_save=True)
    second = make_agent(g, AgentDiscretePPO)
    second.save_or_load_agent(str(tmp_path), if_save=False)
    assert second._adam_step == first._adam_step == ids.shape[0]
    for a in (first, second):
        a.last_state = th.from_numpy(g["last_state"]).to(DEV)
        a.update_net(golden_buffer(g), ids=ids)
        assert a.update_path == "fused"
    assert first._adam_step == second._adam_step == 2 * ids.shape[0]
    for x, y in ((first.act, second.act), (first.cri, second.cri)):
        for (k, v), (_, w) in zip(x.state_dict().items(), y.state_dict().items()):
            np.testing.assert_array_equal(v.cpu().numpy(), w.cpu().numpy(), err_msg=k)
    np.testing.assert_array_equal(first._exp_avg.cpu().numpy(), second._exp_avg.cpu().numpy())
    np.testing.assert_array_equal(first._exp_avg_sq.cpu().numpy(), second._exp_avg_sq.cpu().numpy())
