"""The GAE_ form of the one-launch discrete rollout (csrc/rollout_discrete.hip: erl_rollout_discrete_{cartpole,acrobot}_gae_f32) behind
`fused_rollout_discrete(..., epilogue=...)` and AgentDiscretePPO with args.fused_gae = True: the rollout itself is unchanged to the bit,
the critic's values agree with an fp64 restatement on the recorded states, the advantages / reward sums ARE the exact scan on those
values, the launch geometry is invisible, and update_net consumes what the rollout left only while it is valid.

Shapes: the smallest that reach each way the kernel can go wrong -- a ragged last tile with truncations inside the horizon, two waves
per workgroup with one wave wholly past N (257 tiles), the largest LDS image restaged, S = 6 (features on the q = 1 lanes), H = 1; H is
neither a multiple of the steps the value pass takes at once (4) nor always above it."""
import math

import numpy as np
import pytest
import torch as th

from oracle import ppo_numpy as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (env, N, net, H, max_step, reward_scale)
CASES = [("cartpole", 50, (64, 32), 40, 7, 0.25), ("cartpole", 4100, (32, 32), 5, 3, 1.0), ("cartpole", 300, (128, 128), 12, 500, 2.0),
         ("acrobot", 70, (64, 32), 9, 4, 1.0), ("cartpole", 16, (32, 32), 1, 500, 1.0)]


def make(kind, N, net, max_step, reward_scale=1.0, fused_gae=True, vtrace=True, env_seed=5, agent_seed=3, **extra):
    """agent + env on the one-launch route; `fused_gae` None leaves args.fused_gae unset (the default)"""
    from elegantrl_amd.agents import AgentDiscretePPO
    from elegantrl_amd.envs import AcrobotGpuVecEnv, CartPoleGpuVecEnv
    from elegantrl_amd.train import Config
    env_cls, S, A, name = ((CartPoleGpuVecEnv, 4, 2, "CartPole-v1") if kind == "cartpole" else (AcrobotGpuVecEnv, 6, 3, "Acrobot-v1"))
    args = Config(AgentDiscretePPO, env_cls, {"env_name": name, "num_envs": N, "max_step": max_step, "state_dim": S, "action_dim": A,
                                              "if_discrete": True})
    args.net_dims, args.reward_scale, args.random_seed, args.fused_rollout, args.quiet = list(net), reward_scale, 7, True, True
    args.if_use_v_trace = vtrace
    if fused_gae is not None:
        args.fused_gae = fused_gae
    for k, v in extra.items():
        setattr(args, k, v)
    th.manual_seed(agent_seed)
    agent = AgentDiscretePPO(args.net_dims, S, A, gpu_id=0, args=args)
    with th.no_grad():
        g = th.Generator(device=DEV).manual_seed(agent_seed + 1)
        agent.act.state_avg[:] = 0.01 * th.randn(S, device=DEV, generator=g)
        agent.act.state_std[:] = 0.05 + 0.2 * th.rand(S, device=DEV, generator=g)
        agent.act.net[-1].weight.mul_(6.0)
        # the critic's own normalisation, not the actor's; a last layer that takes |values| to order 1
        agent.cri.state_avg[:] = 0.02 * th.randn(S, device=DEV, generator=g)
        agent.cri.state_std[:] = 0.1 + 0.3 * th.rand(S, device=DEV, generator=g)
        agent.cri.net[-1].weight.mul_(8.0)
        agent.cri.net[-1].bias.fill_(0.5)
    env = env_cls(N, max_step=max_step, gpu_id=0, seed=env_seed)
    agent.last_state = env.reset()[0]
    return agent, env, args


def critic64(agent):
    f = lambda t: t.detach().cpu().numpy().astype(np.float64)  # noqa: E731
    lin = [m for m in agent.cri.net if isinstance(m, th.nn.Linear)]
    return O.Mlp([f(m.weight) for m in lin], [f(m.bias) for m in lin], f(agent.cri.state_avg), f(agent.cri.state_std), None)


def env_state(env):
    out = [env.state.clone(), env.step_count.clone(), env.episode.clone()]
    if hasattr(env, "phys"):
        out.append(env.phys.clone())
    return out


def two_rollouts(kind, N, net, H, max_step, rs, vtrace, fused_gae, uniforms):
    agent, env, _ = make(kind, N, net, max_step, rs, fused_gae=fused_gae, vtrace=vtrace)
    out = []
    for u in uniforms:
        items = agent._explore_vec_env(env, H, noise=u)
        assert agent.rollout_path == "one-launch"
        c = agent._rollout_cache
        out.append(dict(items=items, last=agent.last_state, env=env_state(env), cache=c,
                        kept=(items[3].clone(), items[4].clone())))
    return agent, out


@pytest.fixture(scope="module", params=[c + (v,) for c in CASES for v in (True, False)],
                ids=lambda c: f"{c[0]}-N{c[1]}-{c[2][0]}x{c[2][1]}-H{c[3]}-{'vtrace' if c[6] else 'plain'}")
def runs(request):
    """two consecutive rollouts with injected uniforms, with the epilogue (`on`) and on the parent route (`off`), computed once"""
    kind, N, net, H, max_step, rs, vtrace = request.param
    g = th.Generator(device=DEV).manual_seed(N + H)
    uniforms = [th.rand((H, N), device=DEV, generator=g) for _ in range(2)]
    agent, on = two_rollouts(kind, N, net, H, max_step, rs, vtrace, True, uniforms)
    _, off = two_rollouts(kind, N, net, H, max_step, rs, vtrace, False, uniforms)
    return dict(agent=agent, on=on, off=off, N=N, H=H, max_step=max_step, vtrace=vtrace)


def test_the_rollout_is_unchanged(runs):
    for a, b in zip(runs["on"], runs["off"]):
        assert b["cache"] is None or "adv" not in b["cache"]            # switch off: nothing is left behind
        assert a["cache"] is not None and "adv" in a["cache"]
        for x, y in zip(a["items"], b["items"]):
            assert x.dtype == y.dtype and th.equal(x, y)
        assert th.equal(a["last"], b["last"])
        for x, y in zip(a["env"], b["env"]):
            assert th.equal(x, y)


def test_values_against_fp64(runs):
    """tolerance: tests/test_mlpn_gpu.py::test_mlpn_value_forward (the same fp32-MFMA arithmetic against the same fp64 restatement)"""
    agent, N, H = runs["agent"], runs["N"], runs["H"]
    critic = critic64(agent)
    top = 0.0
    for r in runs["on"]:
        c = r["cache"]
        assert c["values"].shape == (H, N) and c["next_value"].shape == (N,) and c["values"].dtype == th.float32
        ref = O.critic_value(r["items"][0].cpu().numpy().astype(np.float64), critic)
        ref_next = O.critic_value(r["last"].cpu().numpy().astype(np.float64), critic)
        got, got_next = c["values"].cpu().numpy(), c["next_value"].cpu().numpy()
        print(f"values: max |err| {np.abs(got - ref).max():.3e} (next: {np.abs(got_next - ref_next).max():.3e}), max |value| {np.abs(ref).max():.3f}")
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(got_next, ref_next, rtol=1e-4, atol=2e-5)
        top = max(top, float(np.abs(ref).max()))
    assert top > 0.3                                                    # the comparison is not one of zeros


def test_the_epilogue_is_the_exact_gae_scan(runs):
    from elegantrl_amd import ops
    agent, N, H, vtrace = runs["agent"], runs["N"], runs["H"], runs["vtrace"]
    n_trunc = 0
    for r in runs["on"]:
        states, actions, logprobs, rewards, undones, unmasks = r["items"]
        c = r["cache"]
        stats = th.zeros(8, dtype=th.float64, device=DEV)
        adv, ret = ops.gae_scan(rewards.clone(), undones.clone(), unmasks, c["values"], c["next_value"], float(agent.gamma),
                                float(agent.lambda_gae_adv), use_v_trace=vtrace, mutate=True, algo="exact", stats=stats)
        assert th.equal(c["adv"], adv), f"advantages differ in {(c['adv'] != adv).sum().item()} elements"
        assert th.equal(c["ret"], ret)
        assert th.equal(rewards, r["kept"][0]) and th.equal(undones, r["kept"][1])       # explore_env's outputs are not mutated
        assert c["n_parts"] == math.ceil(N / 16) and c["parts"].numel() == 3 * c["n_parts"]
        folded = ops.adv_stats_fold(c["parts"], c["n_parts"], H, N, th.full((8,), -1.0, dtype=th.float64, device=DEV))
        np.testing.assert_allclose(folded.cpu().numpy()[:5], stats.cpu().numpy()[:5], rtol=1e-12, atol=1e-9)
        assert folded[5:].abs().sum().item() == 0
        n_trunc += int((~unmasks).sum())
    if runs["max_step"] < H:
        assert n_trunc > 0


def test_the_launch_geometry_is_invisible():
    """4100 envs: 257 tiles, two waves per workgroup, one wave wholly past N; 4096 envs: one wave per workgroup.  Draws and resets are
    keyed by the env, so the first 4096 columns are the same numbers"""
    kind, N, net, H, max_step, rs = CASES[1]
    M = 4096
    g = th.Generator(device=DEV).manual_seed(N + H)
    u = th.rand((H, N), device=DEV, generator=g)
    big, env_big, _ = make(kind, N, net, max_step, rs)
    small, env_small, _ = make(kind, M, net, max_step, rs)
    with th.no_grad():
        env_small.state.copy_(env_big.state[:M])              # (a generator's stream need not agree between two sizes)
    small.last_state = env_small.state.clone()
    a = big._explore_vec_env(env_big, H, noise=u)
    b = small._explore_vec_env(env_small, H, noise=u[:, :M].contiguous())
    for x, y in zip(a, b):
        assert th.equal(x[:, :M], y)
    ca, cb = big._rollout_cache, small._rollout_cache
    for k in ("values", "adv", "ret"):
        assert th.equal(ca[k][:, :M], cb[k]), k
    assert th.equal(ca["next_value"][:M], cb["next_value"])
    assert th.equal(ca["parts"][:3 * cb["n_parts"]], cb["parts"])        # rows are per tile, not per workgroup


# ---- update_net --------------------------------------------------------------------------------------------------------------------
UPD = dict(N=256, net=(64, 32), H=16, max_step=6, B=1024, n_upd=3)


def iteration(fused_gae, edit=None, get_values=None, gae_algo=None, **extra):
    """one explore + update_net from fixed weights, uniforms and minibatch ids -> what it left"""
    N, net, H, B, n_upd = UPD["N"], UPD["net"], UPD["H"], UPD["B"], UPD["n_upd"]
    agent, env, _ = make("cartpole", N, net, UPD["max_step"], 0.5, fused_gae=fused_gae, horizon_len=H, batch_size=B,
                         repeat_times=n_upd * B / H, learning_rate=1e-3, **extra)
    if gae_algo is not None:
        agent.gae_algo = gae_algo
    g = th.Generator(device=DEV).manual_seed(11)
    u = th.rand((H, N), device=DEV, generator=g)
    ids = th.randint(H * N, (n_upd, B), device=DEV, generator=g)
    items = agent._explore_vec_env(env, H, noise=u)
    cache = agent._rollout_cache
    rec = None if cache is None else (cache["values"].clone(), cache["next_value"].clone())
    before = [x.clone() for x in items]
    had_adv = cache is not None and "adv" in cache
    if edit is not None:
        with th.no_grad():
            edit(agent, items)
    if get_values is not None:
        agent.get_values = get_values
    objs = agent.update_net(list(items), ids=ids)
    return dict(agent=agent, items=items, before=before, objs=objs, flat=agent._flat.clone(), rec=rec, had_adv=had_adv,
                paths=(agent.rollout_path, agent.advantage_path, agent.update_path))


def same_result(a, b):
    assert th.equal(a["flat"], b["flat"]) and tuple(a["objs"]) == tuple(b["objs"])
    for x, y in zip(a["items"], b["items"]):
        assert th.equal(x, y)


def test_update_net_consumes_the_cache_only_while_it_is_valid(monkeypatch):
    monkeypatch.delenv("ERL_FUSED_GAE", raising=False)
    monkeypatch.delenv("ERL_FUSED_DISCRETE_GAE", raising=False)
    on = iteration(True)
    assert on["had_adv"] and on["paths"] == ("one-launch", "rollout", "fused")
    assert on["agent"]._rollout_cache is None
    edits = {"critic weight": lambda agent, items: agent.cri.net[0].weight[0, 0].add_(0.01),
             "cri.state_avg": lambda agent, items: agent.cri.state_avg.add_(0.001),
             "rewards": lambda agent, items: items[3][0, 0].add_(0.25)}
    for name, edit in edits.items():
        a, b = iteration(True, edit=edit), iteration(False, edit=edit)
        assert a["had_adv"] and not b["had_adv"], name
        assert a["paths"] == ("one-launch", "scan", "fused") and b["paths"] == ("one-launch", "scan", "fused"), name
        same_result(a, b)                                                # ... as a run that never had the cache
    a, b = iteration(True, fused_update=False), iteration(False, fused_update=False)
    assert a["paths"] == ("one-launch", "scan", "layered")
    same_result(a, b)
    off = iteration(False)
    assert not off["had_adv"] and off["paths"] == ("one-launch", "scan", "fused")
    default = iteration(None)                                            # the continuous agents' default does not reach a discrete agent
    assert not default["agent"].fused_gae and not default["had_adv"] and default["paths"][1] == "scan"
    same_result(default, off)
    monkeypatch.setenv("ERL_FUSED_DISCRETE_GAE", "1")
    assert iteration(None)["paths"] == ("one-launch", "rollout", "fused")
    monkeypatch.setenv("ERL_FUSED_GAE", "1")
    monkeypatch.delenv("ERL_FUSED_DISCRETE_GAE")
    assert iteration(None)["paths"][1] == "scan"


def test_the_route_equals_the_separate_launches_given_the_same_values():
    """tolerances: tests/test_rollout_fused_gpu.py::test_update_net_with_the_rollout_epilogue_matches_the_separate_launches (the same
    effect: the summation order of the normalisation's sums)"""
    N, H = UPD["N"], UPD["H"]
    a = iteration(True)
    assert a["paths"] == ("one-launch", "rollout", "fused")
    values, next_value = a["rec"]

    def recorded(states):
        if tuple(states.shape) == (H, N, 4):
            return values
        assert tuple(states.shape) == (N, 4)
        return next_value
    b = iteration(False, get_values=recorded, gae_algo="exact")
    assert b["paths"] == ("one-launch", "scan", "fused")
    for x, y in zip(a["before"], b["before"]):
        assert th.equal(x, y)
    for x, y in zip(a["items"], b["items"]):
        assert th.equal(x, y)
    rewards, undones, unmasks = a["items"][3:]
    assert (~unmasks).any()
    assert not th.equal(rewards, a["before"][3]) and not th.equal(undones, a["before"][4])     # get_advantages' side effect, applied
    np.testing.assert_allclose(np.array(a["objs"]), np.array(b["objs"]), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(a["flat"].cpu().numpy(), b["flat"].cpu().numpy(), rtol=0, atol=1e-6)
    assert np.isfinite(a["flat"].cpu().numpy()).all()


def test_train_agent_runs_on_the_route(tmp_path, monkeypatch):
    from elegantrl_amd import _hip, train_agent
    from elegantrl_amd.agents import AgentDiscretePPO
    from elegantrl_amd.envs import CartPoleGpuVecEnv
    from elegantrl_amd.train import Config
    seen = []
    inner = AgentDiscretePPO.update_net

    def spy(self, *a, **k):
        out = inner(self, *a, **k)
        seen.append((self.rollout_path, self.advantage_path, self.update_path, tuple(out.result() if hasattr(out, "result") else out)))
        return out
    monkeypatch.setattr(AgentDiscretePPO, "update_net", spy)
    args = Config(AgentDiscretePPO, CartPoleGpuVecEnv, {"env_name": "CartPole-v1", "num_envs": 64, "max_step": 50, "state_dim": 4,
                                                        "action_dim": 2, "if_discrete": True})
    args.net_dims, args.fused_rollout, args.fused_gae = [64, 32], True, True
    args.horizon_len, args.batch_size, args.repeat_times = 32, 512, 2 * 512 / 32
    args.break_step, args.eval_per_step, args.eval_times = 32 * 3, 10 ** 9, 1
    args.cwd, args.gpu_id, args.random_seed = str(tmp_path / "run"), 0, 0
    train_agent(args, if_single_process=True)
    assert len(seen) >= 3
    for rollout, adv, upd, objs in seen:
        assert (rollout, adv, upd) == ("one-launch", "rollout", "fused")
        assert np.isfinite(np.array(objs)).all()
    assert _hip.lib().erl_async_fault_count(0) == 0
