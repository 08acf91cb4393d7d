"""AgentTD3's / AgentDDPG's one-launch rollout and evaluation (csrc/sac_fused.hip sac_rollout_synenv_kernel<.., DET>, det_actor_tile_kernel;
erl_td3_rollout_*, erl_td3_eval_*, erl_td3_explore_action_tile_f32), switch `args.fused_td3_rollout`:
  1. one launch against the per-step loop on the tile action, bit for bit;
  2. the tail: the clip, std = 0, a teacher-forced fp64 check that can see a missing activation on the second layer, the reference's golden;
  3. the evaluation kernel against the training rollout at std = 0, bit for bit;
  4. the tile action against the layered action;
  5. agent.evaluate_env against the Evaluator's loop;
  6. the routes the agent and the Evaluator take, and a checkpoint in the middle of a Philox run;
  7. train_agent end to end."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch as th

from tests.eval_helpers import oracle_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACT_TOL = dict(rtol=2e-5, atol=2e-6)          # tests/test_td3_gpu.py's bound on exploration actions

# Test 5's bounds.  Measured between two sides that exist without this feature and that it leaves as they were (the torch module and
# erl_pendulum_step_f32): the Evaluator's loop with the fp32 Actor module against the same loop with the module in fp64 and its actions
# cast to fp32 for the env; Pendulum 256 envs x 200 steps, net (128, 64), weight seeds 0..4 (tools/td3_rollout_ab.py --case gap;
# profiles/td3_rollout_ab.txt).  Per seed, largest per-episode |return gap| / |gap of the mean return|:
#   0: 0.0461426 / 0.000183105    1: 0.00756836 / 0    2: 0.00552368 / 0    3: 0.0712585 / 0.000244141    4: 0.00125122 / 0
# (returns are about -600 .. -1500: one float32 ulp there is 6.1e-05 .. 1.2e-04; AgentDDPG builds the same Actor from the same seed).
# Allowed: three times the largest value seen (five seeds under-sample the tail; the margin of tests/test_eval_fused_gpu.py and
# tests/test_modsac_rollout_gpu.py).
TD3_GAP_MEASURED_EPISODE, TD3_GAP_MEASURED_MEAN = 0.071258544921875, 0.000244140625
TD3_EP_BOUND, TD3_MEAN_BOUND = 3 * TD3_GAP_MEASURED_EPISODE, 3 * TD3_GAP_MEASURED_MEAN

AGENTS = ("AgentTD3", "AgentDDPG")


def _cls(name):
    from elegantrl_amd import agents
    return getattr(agents, name)


def _env(kind, N, S, A, max_step, env_seed):
    from elegantrl_amd.envs import PendulumVecEnv, PointChasingVecEnv, SynVecEnv
    return (PendulumVecEnv(N, max_step=max_step, gpu_id=0, seed=env_seed) if kind == "pendulum" else
            PointChasingVecEnv(A, N, max_step=max_step, gpu_id=0, seed=env_seed) if kind == "point" else
            SynVecEnv(N, S, A, max_step=max_step, gpu_id=0, seed=env_seed))


def _make(name, kind, N, S, A, net, max_step, scale=1.0, fused_rollout=True, on=True, std=None, seed=5, env_seed=1, **extra):
    from elegantrl_amd.train import Config
    cls = _cls(name)
    args = Config(cls, None, {"env_name": kind, "num_envs": N, "max_step": max_step, "state_dim": S, "action_dim": A, "if_discrete": False})
    args.net_dims, args.random_seed, args.reward_scale, args.fused_rollout, args.fused_td3_rollout = list(net), 3, scale, fused_rollout, on
    args.quiet = True
    if std is not None:
        args.explore_noise_std = args.explore_noise = std          # (AgentTD3 reads the first spelling, AgentDDPG the second)
    for k, v in extra.items():
        setattr(args, k, v)
    th.manual_seed(seed)
    agent = cls(args.net_dims, S, A, gpu_id=0, args=args)
    env = _env(kind, N, S, A, max_step, env_seed)
    agent.last_state = env.reset()[0]
    return agent, env, args


def _count(env, name):
    """counts the calls of env.<name>"""
    calls = []
    inner = getattr(env, name)
    setattr(env, name, lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    return calls


def _phys(env):
    return getattr(env, "phys", getattr(env, "distance", None))


# ---- 1. one launch against the per-step loop on the tile action ---------------------------------------------------------------------------
# (N, S, A, net, max_step, H, reward_scale)
SYN_CASES = [(64, 11, 3, (256, 256), 5, 9, 1.0), (50, 17, 6, (64, 48), 4, 7, 0.25), (100, 56, 8, (128, 256), 1000, 6, 1.0),
             (16, 3, 1, (256, 64), 3, 12, 1.0),          # the head is one column wide
             (4, 11, 3, (64, 32), 5, 8, 1.0)]            # the golden's shape: fewer rows than a tile
PEN_CASES = [(64, (256, 256), 7, 20, 1.0), (50, (64, 48), 200, 9, 1.0), (4096, (128, 64), 5, 6, 1.0)]
POINT_CASES = [(dim, N) for dim in (1, 2, 4) for N in (50, 64)]


def _bit_identity(name, kind, N, S, A, net, max_step, H, scale, inject):
    (fa, fe, _), (pa, pe, _) = (_make(name, kind, N, S, A, net, max_step, scale, fused_rollout=f, std=0.3) for f in (True, False))
    assert fa.fused_td3_rollout and pa.fused_td3_rollout and fa.fused_rollout and not pa.fused_rollout
    assert fa.explore_noise_std == pa.explore_noise_std == 0.3
    assert th.equal(fa._actor_flat, pa._actor_flat) and th.equal(fe.state, pe.state)
    f_launches, p_launches = _count(fe, "fused_rollout_offpolicy"), _count(pe, "fused_rollout_offpolicy")
    p_steps = _count(pe, "step_into")
    g = th.Generator(device=DEV).manual_seed(2)
    for it in range(2):
        noise = th.randn((H, N, A), device=DEV, generator=g) if inject else None
        f_items = fa._explore_vec_env(fe, H, noise=noise)
        p_items = pa._explore_vec_env(pe, H, noise=noise)
        assert len(f_launches) == it + 1 and len(p_launches) == 0 and len(p_steps) == (it + 1) * H      # the launch counter moved on one side only
        assert fa.rollout_path == f"one launch (erl_td3_rollout_*_f32 through {type(fe).__name__}.fused_rollout_offpolicy)"
        assert pa.rollout_path.startswith("per-step loop (tile action erl_td3_explore_action_tile_f32") and "fused_rollout is off" in pa.rollout_path
        for nm, x, y in zip(("states", "actions", "rewards", "undones", "unmasks"), f_items, p_items):
            assert x.dtype == y.dtype and x.shape == y.shape, nm
            assert th.equal(x, y), f"{nm} differs at rollout {it}: {(x != y).sum().item()} elements"
        assert float(f_items[1].abs().max()) <= 1.0 and bool((f_items[1].abs() == 1.0).any()) == bool((p_items[1].abs() == 1.0).any())
        assert th.equal(fa.last_state, pa.last_state) and th.equal(fe.state, pe.state)
        if _phys(fe) is not None:
            assert th.equal(_phys(fe), _phys(pe))
        assert th.equal(fe.step_count, pe.step_count) and th.equal(fe.episode, pe.episode)
        assert fa.rng_counter == pa.rng_counter == (it + 1) * H
        if max_step < H:
            assert (~f_items[4]).any(), "the case is meant to contain truncations"


@pytest.mark.parametrize("name", AGENTS)
@pytest.mark.parametrize("N,S,A,net,max_step,H,scale", SYN_CASES)
@pytest.mark.parametrize("inject", [True, False], ids=["injected-noise", "philox"])
def test_one_launch_rollout_is_bit_identical_to_the_loop_on_the_tile_action(name, N, S, A, net, max_step, H, scale, inject):
    """erl_td3_rollout_synenv_f32 against erl_td3_explore_action_tile_f32 + erl_synenv_step_f32 per step, two consecutive rollouts"""
    _bit_identity(name, "syn", N, S, A, net, max_step, H, scale, inject)


@pytest.mark.parametrize("name", AGENTS)
@pytest.mark.parametrize("N,net,max_step,H,scale", PEN_CASES)
@pytest.mark.parametrize("inject", [True, False], ids=["injected-noise", "philox"])
def test_one_launch_rollout_on_pendulum_is_bit_identical_to_the_loop_on_the_tile_action(name, N, net, max_step, H, scale, inject):
    _bit_identity(name, "pendulum", N, 3, 1, net, max_step, H, scale, inject)


@pytest.mark.parametrize("name", AGENTS)
@pytest.mark.parametrize("dim,N", POINT_CASES)
@pytest.mark.parametrize("inject", [True, False], ids=["injected-noise", "philox"])
def test_one_launch_rollout_on_pointchasing_is_bit_identical_to_the_loop_on_the_tile_action(name, dim, N, inject):
    _bit_identity(name, "point", N, 4 * dim, dim, (64, 48), 5, 8, 1.0, inject)


# ---- 2. the tail ----------------------------------------------------------------------------------------------------------------------------
CLIP_N, CLIP_A, CLIP_H, CLIP_STD, CLIP_SEED = 50, 5, 2, 1.5, 4
CLIP_BIAS = (-2.0, -0.3, 0.0, 0.3, 2.0)


def _clip_case():
    """the injected noise (H, N, A) float32 on the CPU, clip(tanh(b) + 1.5 eps, -1, 1) in fp64 and the unclipped sum.  The draws are
    th.randn of a CPU generator (seed 4), except that a draw whose unclipped sum lies within 0.1 of zero is moved 0.2 away from it: the
    bound below is relative, and a sum that cancels keeps the absolute error of its terms (about 2e-7: tanhf's few ulp below 1 and one
    rounding of 1.5 eps), which rtol 1e-5 only covers from 0.02 up.  The reference formula alone decides all of this."""
    eps = th.randn((CLIP_H, CLIP_N, CLIP_A), generator=th.Generator().manual_seed(CLIP_SEED)).numpy()
    tb = np.tanh(np.array(CLIP_BIAS))[None, None, :]
    raw = tb + CLIP_STD * eps.astype(np.float64)
    eps = np.where(np.abs(raw) < 0.1, eps + np.where(raw >= 0, 0.2, -0.2), eps).astype(np.float32)
    raw = tb + CLIP_STD * eps.astype(np.float64)
    return eps, np.clip(raw, -1.0, 1.0), raw


@pytest.mark.parametrize("name", AGENTS)
@pytest.mark.parametrize("net", [(256, 256), (64, 48)])
def test_the_action_is_clipped_after_the_noise(name, net):
    """(a) head weight 0, head bias on the cycle (-2, -0.3, 0, 0.3, 2), std 1.5: the head output is the bias exactly, so action =
    clip(tanh(b) + 1.5 eps, -1, 1).  rtol 1e-5 without an absolute term (_clip_case says why it can hold); the elements on the clip are
    +-1 exactly.  With eps ~ N(0, 1) and std 1.5 about half the elements leave [-1, 1]: at least 10 % is asserted, on the reference
    formula alone (tests/test_td3_rollout_abi_cpu.py::test_the_clip_case_holds_what_it_is_meant_to runs it without a GPU)."""
    agent, env, _ = _make(name, "syn", CLIP_N, 11, CLIP_A, net, 100, std=CLIP_STD)
    with th.no_grad():
        agent.act.net[4].weight.zero_()
        agent.act.net[4].bias.copy_(th.tensor(CLIP_BIAS, dtype=th.float32))
    agent._sync_modules()
    assert th.equal(agent._actor_flat[-CLIP_A:].cpu(), th.tensor(CLIP_BIAS, dtype=th.float32))       # the module's tensors ARE the flat block
    eps, want, raw = _clip_case()
    noise = th.from_numpy(eps).to(DEV)
    on_clip = np.abs(want) == 1.0
    print(f"[{name} {net}] elements on the clip: {on_clip.mean():.3f}")
    assert on_clip.mean() >= 0.10                                               # decided by the reference formula alone
    assert (np.abs(raw[on_clip]) > 1.0).all()                                   # unclipped, they would leave [-1, 1]
    tile = agent.explore_action(agent.last_state, noise[0])                     # the per-step action on the tile kernel
    agent.rng_counter = 0
    launches = _count(env, "fused_rollout_offpolicy")
    actions = agent._explore_vec_env(env, CLIP_H, noise=noise)[1]
    assert len(launches) == 1 and th.equal(actions[0], tile)
    got = actions.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0.0)
    assert (got[on_clip] == want[on_clip]).all()                                # exactly +-1
    assert np.abs(got).max() <= 1.0
    # Where the sum cancels (what _clip_case keeps out of the relative bound above): eps = -tanh(b) / 1.5 + d, d from -2e-3 to 2e-3 over
    # the envs (step 1: ten times that), so tanh(b) + 1.5 eps = 1.5 d up to the rounding of eps.  The absolute term is the error of the
    # terms, from the formats alone: tanhf within 5 ulp of a value below 1 (the device math library's stated bound: 5 x 6.0e-8), 1.5 eps
    # rounded once where it is not fused (half an ulp of a value below 1: 3.0e-8), the sum rounded once (below 1e-8 here) -- 3.4e-7, taken
    # as 4e-7; rtol 1e-5 as above.
    d = np.linspace(-2e-3, 2e-3, CLIP_N)[None, :, None] * np.array([1.0, 10.0])[:, None, None]
    eps_c = (-np.tanh(np.array(CLIP_BIAS))[None, None, :] / CLIP_STD + d).astype(np.float32)
    want_c = np.tanh(np.array(CLIP_BIAS))[None, None, :] + CLIP_STD * eps_c.astype(np.float64)
    assert np.abs(want_c).max() < 0.05 and (np.abs(want_c) < 1e-4).any()
    agent.last_state = env.reset()[0]
    got_c = agent._explore_vec_env(env, CLIP_H, noise=th.from_numpy(eps_c).to(DEV))[1].cpu().numpy().astype(np.float64)
    print(f"[{name} {net}] near cancellation: max |action - fp64| {np.abs(got_c - want_c).max():.3g}")
    np.testing.assert_allclose(got_c, want_c, rtol=1e-5, atol=4e-7)


@pytest.mark.parametrize("name", AGENTS)
@pytest.mark.parametrize("net", [(256, 256), (64, 48)])
def test_zero_std_is_plain_tanh(name, net):
    """(b) explore_noise_std = 0: the rollout's actions are the tile action's without noise, bit for bit, whatever noise is injected, and
    tanh(net(state)) of the fp64 module within tests/test_td3_gpu.py's bound on exploration actions"""
    N, S, A, H = 50, 17, 6, 3
    agent, env, _ = _make(name, "syn", N, S, A, net, 100, std=0.0)
    assert agent.explore_noise_std == 0.0
    state0 = agent.last_state.clone()
    tile = agent.explore_action(state0, None)
    agent.rng_counter = 0
    g = th.Generator(device=DEV).manual_seed(8)
    noise = 5.0 * th.randn((H, N, A), device=DEV, generator=g)                  # must not be read
    launches = _count(env, "fused_rollout_offpolicy")
    states, actions = agent._explore_vec_env(env, H, noise=noise)[:2]
    assert len(launches) == 1 and th.equal(states[0], state0) and th.equal(actions[0], tile)
    act64 = deepcopy(agent.act).double().cpu()
    with th.no_grad():
        ref = act64.net(states.reshape(H * N, S).double().cpu()).tanh()
        assert th.equal(ref, act64(states.reshape(H * N, S).double().cpu()))
    np.testing.assert_allclose(actions.reshape(H * N, A).cpu().numpy(), ref.numpy(), **ACT_TOL)


def _det_actions_fp64(act64, states, std, noise, activate_layer_2=True):
    """Actor.get_action in fp64; with activate_layer_2 = False, what a kernel that left the second hidden layer raw would compute"""
    lin1, act1, lin2, act2, head = act64.net
    z2 = lin2(act1(lin1(states)))
    y = head(act2(z2) if activate_layer_2 else z2)
    return (y.tanh() + std * noise).clip(-1.0, 1.0), z2


@pytest.mark.parametrize("name", AGENTS)
@pytest.mark.parametrize("net", [(256, 256), (64, 48)])
def test_both_hidden_layers_are_activated_teacher_forced_against_fp64(name, net):
    """(c) every step of a 9-step one-launch rollout: the recorded states[t] and noise[t] through the fp64 Actor module give actions[t]
    within rtol 2e-5 / atol 2e-6.  The run must be able to see a missing activation on the second layer (the mistake opposite to the one
    tests/test_modsac_rollout_gpu.py::test_the_second_layer_is_raw_teacher_forced_against_fp64 looks for): a quarter of the second-layer
    pre-activations negative, and a raw second layer moving the fp64 action beyond the tolerance on at least half the rows.  std 0.05 keeps the
    clip away from most elements."""
    N, S, A, H, std = 50, 17, 6, 9, 0.05
    agent, env, _ = _make(name, "syn", N, S, A, net, 4, std=std)
    assert len(agent.act.net) == 5
    g = th.Generator(device=DEV).manual_seed(6)
    noise = th.randn((H, N, A), device=DEV, generator=g)
    launches = _count(env, "fused_rollout_offpolicy")
    states, actions = agent._explore_vec_env(env, H, noise=noise)[:2]
    assert len(launches) == 1
    act64 = deepcopy(agent.act).double().cpu()
    x, e, got = states.reshape(H * N, S).double().cpu(), noise.reshape(H * N, A).double().cpu(), actions.reshape(H * N, A).double().cpu()
    with th.no_grad():
        ref, z2 = _det_actions_fp64(act64, x, std, e)
        assert th.equal(ref, act64.get_action(x, std, e))
        raw, _ = _det_actions_fp64(act64, x, std, e, activate_layer_2=False)
    negative = float((z2 < 0).double().mean())
    moved = float((((raw - ref).abs() > 2e-6 + 2e-5 * ref.abs()).any(dim=1)).double().mean())
    err = (got - ref).abs()
    print(f"[{name} net {net}] negative second-layer pre-activations {negative:.3f}; rows a raw second layer would move {moved:.3f}; "
          f"max |action - fp64| {float(err.max()):.3g}, max ratio to the bound {float((err / (2e-6 + 2e-5 * ref.abs())).max()):.3f}")
    assert negative >= 0.25 and moved >= 0.5
    np.testing.assert_allclose(got.numpy(), ref.numpy(), **ACT_TOL)
    for t in (0, H - 1):                                                         # per t, the module's own method
        with th.no_grad():
            a_t = act64.get_action(states[t].double().cpu(), std, noise[t].double().cpu())
        np.testing.assert_allclose(actions[t].cpu().numpy(), a_t.numpy(), **ACT_TOL)


def test_the_golden_rollout_replays_with_the_switch_on():
    """(d) the rollout part of tests/test_td3_gpu.py::test_rollout_and_four_updates_replay_the_reference_and_fp64 on the tile action (the
    scripted env has no one-launch method: the loop runs, on erl_td3_explore_action_tile_f32), same bounds"""
    from tests.helpers import load
    from tests.td3_ref import Td3Ref
    from tests.test_td3_gpu import _ReplayEnv, _agent, _load_from_ref
    g = load("td3_small.npz")
    N, S, A, rows, B, n_upd, E, freq, h1, h2 = [int(x) for x in g["dims"]]
    gamma, lr, max_norm, reward_scale, tau, policy_noise, explore_noise = [float(x) for x in g["hyper"]]
    agent = _agent(_cls("AgentTD3"), S, A, (h1, h2), B, N=N, learning_rate=lr, gamma=gamma, reward_scale=reward_scale, soft_update_tau=tau,
                   clip_grad_norm=max_norm, num_ensembles=E, update_freq=freq, policy_noise_std=policy_noise, explore_noise_std=explore_noise,
                   fused_td3_rollout=True)
    ref = Td3Ref([h1, h2], S, A, E, lr=lr, gamma=gamma, tau=tau, max_norm=max_norm, policy_noise_std=policy_noise)
    ref.load({k[5:]: v for k, v in g.items() if k.startswith("act0.")}, {k[5:]: v for k, v in g.items() if k.startswith("cri0.")})
    _load_from_ref(agent, ref)
    agent.last_state = th.from_numpy(g["first_state"]).to(DEV)
    items = agent._explore_vec_env(_ReplayEnv(g, reward_scale), rows, noise=th.from_numpy(g["ro_eps"]).to(DEV))
    assert agent.rollout_path.startswith("per-step loop (tile action erl_td3_explore_action_tile_f32") and "_ReplayEnv has no" in agent.rollout_path
    for got, nm in zip(items, ("ro_states", "ro_actions", "ro_rewards", "ro_undones", "ro_unmasks")):
        if got.dtype == th.bool:
            np.testing.assert_array_equal(got.cpu().numpy(), g[nm])
        else:
            np.testing.assert_allclose(got.cpu().numpy(), g[nm], rtol=2e-5, atol=2e-6)
    np.testing.assert_array_equal(agent.last_state.cpu().numpy(), g["ro_last_state"])


# ---- 3. the evaluation kernel against the training rollout at std = 0 ---------------------------------------------------------------------------
def _kernel_table(agent, env, H):
    """the erl_td3_eval_* entry with horizon H (no reset), then the compaction"""
    from elegantrl_amd import _hip
    from elegantrl_amd.envs.vec_envs import compact_episodes
    N = env.num_envs
    nbytes = _hip.lib().erl_eval_workspace_bytes(N, H)
    ws = th.full((nbytes,), 0xAB, dtype=th.uint8, device=DEV)          # garbage: the launch must write every element it later reads
    rows = th.full((N * H, 2), -7.0, dtype=th.float32, device=DEV)
    count = th.full((1,), -1, dtype=th.int32, device=DEV)
    agent._sync_modules()
    env.fused_evaluate_offpolicy(agent, H, ws)
    compact_episodes(ws, N, H, rows, count)
    n = int(count.item())
    assert 0 <= n <= N * H and (rows[n:] == -7.0).all()
    return rows[:n].cpu().numpy()


# (kind, N ragged, S, A, max_step, H)
EVAL_ENVS = [("syn", 50, 17, 3, 4, 9), ("pendulum", 70, 3, 1, 5, 12), ("point", 50, 8, 2, 4, 9)]


@pytest.mark.parametrize("name", AGENTS)
@pytest.mark.parametrize("kind,N,S,A,max_step,H", EVAL_ENVS)
@pytest.mark.parametrize("net", [(256, 256), (128, 64)])
def test_eval_kernel_is_the_training_rollout_at_zero_std(name, kind, N, S, A, max_step, H, net):
    """the method of tests/test_eval_fused_gpu.py::_check_against_training_rollout: the episode table, the env state and the counters, two
    passes without a reset"""
    a_agent, a_env, _ = _make(name, kind, N, S, A, net, max_step, std=0.0, env_seed=5)
    b_agent, b_env, _ = _make(name, kind, N, S, A, net, max_step, std=0.0, env_seed=5)
    assert th.equal(a_env.state, b_env.state) and th.equal(a_agent._actor_flat, b_agent._actor_flat)
    launches = _count(b_env, "fused_rollout_offpolicy")
    for it in range(2):
        rewards, undones, unmasks = b_agent._explore_vec_env(b_env, H)[-3:]
        assert len(launches) == it + 1
        ref = oracle_table(rewards, undones, unmasks)
        got = _kernel_table(a_agent, a_env, H)
        done = ~(undones & unmasks)
        assert len(ref) >= 1 and int(done.sum(0).max()) >= 2, "the case is meant to contain an env with two or more episodes"
        assert bool((~done[-1]).any()), "the case is meant to contain an open tail"
        assert th.equal(a_env.state, b_env.state), f"env state differs at pass {it}"
        assert th.equal(a_env.step_count, b_env.step_count) and th.equal(a_env.episode, b_env.episode)
        if _phys(a_env) is not None:
            assert th.equal(_phys(a_env), _phys(b_env))
        assert got.shape == ref.shape, f"{got.shape[0]} episodes from the kernels, {ref.shape[0]} from the rollout"
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"episode table differs at pass {it}"


# ---- 4. the tile action against the layered action ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,A,net,max_step,H,scale", SYN_CASES)
@pytest.mark.parametrize("inject", [True, False], ids=["injected-noise", "philox"])
def test_tile_action_agrees_with_the_layered_action(N, S, A, net, max_step, H, scale, inject):
    """erl_td3_explore_action_tile_f32 against erl_td3_explore_action_f32 on the same states, noise / Philox keys and std: the layers are
    summed in another order, so rtol 2e-5 / atol 2e-6 (tests/test_td3_gpu.py's bound on exploration actions), not bits; an element the
    clip holds on one side is held on the other or within the bound of it"""
    from elegantrl_amd import ops
    agent, env, _ = _make("AgentTD3", "syn", N, S, A, net, max_step, std=0.3)
    g = th.Generator(device=DEV).manual_seed(9)
    state = th.randn((N, S), device=DEV, generator=g)
    noise = th.randn((N, A), device=DEV, generator=g) if inject else None
    out_t, out_l = (th.full((N, A), 7.0, device=DEV) for _ in range(2))
    st_t, st_l = (th.full((N, S), 7.0, device=DEV) for _ in range(2))
    for tile, out, st in ((True, out_t, st_t), (False, out_l, st_l)):
        got = ops.td3_explore_action(agent._spec, agent._actor_flat, state, 0.3, noise=noise, seed=11, counter=5, out=out, out_state=st, tile=tile)
        assert got is out
    assert th.equal(st_t, state) and th.equal(st_l, state)
    assert float(out_t.abs().max()) <= 1.0
    np.testing.assert_allclose(out_t.cpu().numpy(), out_l.cpu().numpy(), **ACT_TOL)


# ---- 5. agent.evaluate_env against the Evaluator's loop ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AGENTS)
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_evaluate_env_agrees_with_the_evaluator_loop_on_pendulum(name, seed):
    """Bounds: 3 x the largest gap of five seeds between the Evaluator's loop on the fp32 module and on the fp64 module
    (TD3_GAP_MEASURED_* above: 0.0712585 per episode, 0.000244141 of the mean return; profiles/td3_rollout_ab.txt) = 0.213776 and
    0.000732422.  Episode counts and lengths are equal exactly."""
    from elegantrl_amd.train.evaluator import get_cumulative_rewards_and_step_from_vec_env
    agent, env, _ = _make(name, "pendulum", 256, 3, 1, (128, 64), 200, seed=seed, env_seed=5)
    fused = agent.evaluate_env(env)
    assert fused is not None and fused.dtype == th.float32 and fused.device.type == "cpu"
    loop = get_cumulative_rewards_and_step_from_vec_env(env, agent.act)
    ep = float((fused[:, 0] - loop[:, 0]).abs().max()) if fused.shape == loop.shape else float("nan")
    mean = abs(float(fused[:, 0].mean()) - float(loop[:, 0].mean()))
    print(f"[{name} pendulum seed {seed}] per-episode gap {ep:.6g} (bound {TD3_EP_BOUND:.6g}), mean gap {mean:.6g} (bound {TD3_MEAN_BOUND:.6g})")
    assert fused.shape == loop.shape == (256, 2)
    assert th.equal(fused[:, 1], loop[:, 1]) and bool((fused[:, 1] == 200).all())
    assert ep <= TD3_EP_BOUND and mean <= TD3_MEAN_BOUND


# ---- 6. routes ----------------------------------------------------------------------------------------------------------------------------------
def _evaluator(tmp_path, env, args, **kw):
    from elegantrl_amd.train.evaluator import Evaluator
    args.cwd, args.eval_times = str(tmp_path), 3
    os.makedirs(args.cwd, exist_ok=True)
    return Evaluator(args.cwd, env, args, **kw)


class _PlainEnv:
    """a device env of the vector protocol without the one-launch methods"""

    def __init__(self, env):
        self._env = env
        self.num_envs, self.state_dim, self.action_dim, self.device, self.max_step = env.num_envs, env.state_dim, env.action_dim, env.device, env.max_step

    def step_into(self, *a):
        return self._env.step_into(*a)


@pytest.mark.parametrize("name", AGENTS)
def test_rollout_path_names_the_route(name):
    N, S, A, H = 50, 17, 6, 3
    for on, fused, net, plain, words, n_launch in (
            (False, True, (64, 48), False, ("per-step loop (erl_td3_explore_action_f32", "fused_td3_rollout is off", "ERL_FUSED_TD3_ROLLOUT"), 0),
            (True, False, (64, 48), False, ("per-step loop (tile action erl_td3_explore_action_tile_f32", "fused_rollout is off"), 0),
            (True, True, (100, 100), False, ("per-step loop (erl_td3_explore_action_f32", "[100, 100]", "outside"), 0),
            (True, True, (64, 48), True, ("per-step loop (tile action erl_td3_explore_action_tile_f32", "_PlainEnv has no fused_rollout_offpolicy"), 0),
            (True, True, (64, 48), False, ("one launch (erl_td3_rollout_*_f32 through SynVecEnv.fused_rollout_offpolicy)",), 1)):
        agent, env, _ = _make(name, "syn", N, S, A, net, 4, fused_rollout=fused, on=on)
        assert agent.rollout_path is None
        launches = _count(env, "fused_rollout_offpolicy")
        steps = _count(env, "step_into")
        items = agent.explore_env(_PlainEnv(env) if plain else env, H)
        assert agent.rollout_path.startswith(words[0]) and all(w in agent.rollout_path for w in words), agent.rollout_path
        assert "out of scope" not in agent.rollout_path
        assert len(launches) == n_launch and len(steps) == (0 if n_launch else H) and agent.rng_counter == H
        assert items[0].shape == (H, N, S) and float(items[1].abs().max()) <= 1.0


@pytest.mark.parametrize("name", AGENTS)
def test_the_evaluator_takes_the_fused_path_only_with_the_switches_on(name, tmp_path):
    def spy(agent):
        calls, inner = [], agent.evaluate_env
        agent.evaluate_env = lambda env: (calls.append(env), inner(env))[1]
        return calls

    agent, env, args = _make(name, "pendulum", 64, 3, 1, (256, 256), 25)
    assert agent._fused_eval_reason(env) is None
    calls = spy(agent)
    ev = _evaluator(tmp_path, env, args, agent=agent)
    rs = ev.get_cumulative_rewards_and_step(agent.act)
    assert len(calls) == 1 and calls[0] is env and rs.shape == (64, 2) and bool((rs[:, 1] == 25).all()) and "fused evaluation" in ev.eval_path
    # an actor that is not agent.act: the loop
    ev = _evaluator(tmp_path, env, args, agent=agent)
    ev.get_cumulative_rewards_and_step(deepcopy(agent.act))
    assert ev.eval_path.startswith("loop evaluation") and "not agent.act" in ev.eval_path and len(calls) == 1
    # the switch off: the loop, with the reason naming the switch
    agent, env, args = _make(name, "pendulum", 64, 3, 1, (256, 256), 25, on=False)
    assert agent.evaluate_env(env) is None and "fused_td3_rollout is off" in agent._fused_eval_reason(env)
    ev = _evaluator(tmp_path, env, args, agent=agent)
    rs = ev.get_cumulative_rewards_and_step(agent.act)
    assert rs.shape == (64, 2) and ev.eval_path.startswith("loop evaluation") and "fused_td3_rollout is off" in ev.eval_path
    # the persistent rollout off: its evaluation form goes with it
    agent, env, args = _make(name, "pendulum", 64, 3, 1, (256, 256), 25)
    assert agent.evaluate_env(env) is not None
    agent.fused_rollout = False
    assert agent.evaluate_env(env) is None
    ev = _evaluator(tmp_path, env, args, agent=agent)
    ev.get_cumulative_rewards_and_step(agent.act)
    assert ev.eval_path.startswith("loop evaluation") and "fused_rollout is off" in ev.eval_path
    # a net outside the shapes
    agent, env, args = _make(name, "pendulum", 64, 3, 1, (100, 100), 25)
    assert agent.evaluate_env(env) is None and "outside" in agent._fused_eval_reason(env) and "[100, 100]" in agent._fused_eval_reason(env)


@pytest.mark.parametrize("name", AGENTS)
def test_a_checkpoint_continues_the_philox_rollout(name, tmp_path):
    """save after a one-launch rollout, load into a fresh agent (the checkpoint carries the Philox counter), hand over what it does not
    hold (the env and the last state): the next rollout is the original's, bit for bit"""
    N, S, A, H, net = 50, 17, 6, 5, (64, 48)
    a, ea, _ = _make(name, "syn", N, S, A, net, 4, std=0.3)
    a._explore_vec_env(ea, H)
    assert a.rollout_path.startswith("one launch")
    os.makedirs(tmp_path, exist_ok=True)
    a.save_or_load_agent(str(tmp_path), if_save=True)
    b, eb, _ = _make(name, "syn", N, S, A, net, 4, std=0.3, seed=99)
    assert not th.equal(a._actor_flat, b._actor_flat)
    b.save_or_load_agent(str(tmp_path), if_save=False)
    assert th.equal(a._actor_flat, b._actor_flat)
    eb.state.copy_(ea.state)
    eb.step_count.copy_(ea.step_count)
    eb.episode.copy_(ea.episode)
    assert b.rng_counter == a.rng_counter == H
    b.last_state = a.last_state.clone()
    launches = _count(eb, "fused_rollout_offpolicy")
    want, got = a._explore_vec_env(ea, H), b._explore_vec_env(eb, H)
    assert len(launches) == 1 and b.rollout_path.startswith("one launch")
    for x, y in zip(want, got):
        assert th.equal(x, y)
    assert th.equal(ea.state, eb.state) and th.equal(a.last_state, b.last_state) and a.rng_counter == b.rng_counter == 2 * H


# ---- 7. train_agent end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AGENTS)
def test_train_agent_on_pendulum_with_the_switch_on(name, tmp_path, capsys):
    from elegantrl_amd import train_agent
    from elegantrl_amd.envs import PendulumVecEnv
    from elegantrl_amd.train import Config
    made = []

    class Watched(_cls(name)):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    args = Config(Watched, PendulumVecEnv, {"env_name": "Pendulum-v1", "num_envs": 16, "max_step": 20, "state_dim": 3, "action_dim": 1,
                                            "if_discrete": False})
    assert args.if_off_policy
    args.net_dims = [128, 64]
    args.horizon_len, args.batch_size, args.repeat_times, args.buffer_size = 16, 64, 1.0, 4096       # 16 x 16 = 256 steps a rollout
    args.break_step, args.eval_per_step, args.eval_times = 256 * 3, 256 * 2, 16                       # evaluations at steps 256 and 768: two
    args.cwd, args.gpu_id, args.random_seed = str(tmp_path / "run"), 0, 0
    args.fused_td3_rollout = True
    train_agent(args, if_single_process=True)
    th.set_grad_enabled(True)                                                           # (train_agent leaves autograd switched off)
    out = capsys.readouterr().out
    agent, = made
    assert agent.fused_td3_rollout and agent.rollout_path == "one launch (erl_td3_rollout_*_f32 through PendulumVecEnv.fused_rollout_offpolicy)"
    assert "| Evaluator: fused evaluation" in out and "loop evaluation" not in out
    files = os.listdir(args.cwd)
    assert "act.pth" in files and "recorder.npy" in files
    rec = np.load(os.path.join(args.cwd, "recorder.npy"))
    assert rec.shape[0] >= 1 and np.isfinite(rec[:, :4]).all(), rec
    actor = th.load(os.path.join(args.cwd, "act.pth"), weights_only=False)
    assert all(bool(th.isfinite(p).all()) for p in actor.parameters())
    assert actor(th.zeros((2, 3), device=DEV)).shape == (2, 1)
