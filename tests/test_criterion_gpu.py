"""args.criterion on the device (csrc/critic_loss.h): Smooth-L1 and Huber critic losses through every PPO kernel family and through the
layered and fused SAC steps against the fp64 restatements of tests/criterion_cases.py, under the bounds the same family's MSE test uses;
all rows masked; the one-call PPO and SAC loops against the loop of their steps; all six agents on every update route they have, with
spies on the library's entries; AgentPPO and AgentSAC end to end against the oracle.  Thresholds are the float32 median of
|prediction - target| over the unmasked elements, so both arms of each loss are exercised (asserted per case; a one-row case sits on the
boundary itself)."""
import numpy as np
import pytest
import torch as th

from oracle import ppo_numpy as O
from tests import criterion_cases as K
from tests import sac_gradient_cases as C

pytestmark = pytest.mark.gpu
KINDS = [K.SMOOTH_L1, K.HUBER]
KIND_IDS = ["smooth_l1", "huber"]


@pytest.fixture(scope="module")
def dev():
    return th.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from elegantrl_amd import ops as _ops
    return _ops


def cu(a, dev, dtype=None):
    t = th.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def random_net_n(rng, dims, with_std):
    ws, bs = [], []
    for i, o in zip(dims[:-1], dims[1:]):
        ws.append((rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32))
        bs.append((0.1 * rng.standard_normal(o)).astype(np.float32))
    S, out = dims[0], dims[-1]
    return O.Mlp(ws, bs, (0.1 * rng.standard_normal(S)).astype(np.float32), (1.0 + 0.2 * rng.random(S)).astype(np.float32),
                 (-0.3 + 0.1 * rng.standard_normal(out)).astype(np.float32) if with_std else None)


def flat_params(net):
    return np.concatenate([p.reshape(-1) for p in net.trainable()]).astype(np.float32)


def ppo_case(rng, H, N, S, A, B, discrete=False, masked=False):
    """tests/test_kernels_gpu.py:ppo_case with about one row in eight masked (`masked`: every row) and, for B = 1, an unmasked row"""
    states = rng.standard_normal((H, N, S), dtype=np.float32)
    actions = rng.integers(0, A, size=(H, N)).astype(np.int32) if discrete else rng.standard_normal((H, N, A), dtype=np.float32) * 0.7
    um = rng.random((H, N)) > 0.125
    lp = ((-0.7 if discrete else -1.0 * A) + 0.3 * rng.standard_normal((H, N))).astype(np.float32)
    adv = rng.standard_normal((H, N), dtype=np.float32)
    rs = rng.standard_normal((H, N), dtype=np.float32)
    ids = rng.integers(0, H * N, size=B).astype(np.int64)
    if masked:
        um[:] = False
    elif B == 1:
        i0, i1 = O.split_ids(ids, H)
        um[i0, i1] = True
    return (states, actions, um, lp, adv, rs), ids


def block_errors(got, ref, dims, with_std):
    """the largest of tests/test_ppo_wide_gpu.py:block_errors' values: max |got - ref| per parameter block relative to the WHOLE gradient's
    scale -- over all blocks that is max |got - ref| / max |ref|"""
    assert got.size == ref.size == sum(n for i, o in zip(dims[:-1], dims[1:]) for n in (i * o, o)) + (dims[-1] if with_std else 0)
    return np.abs(got - ref).max() / max(1e-30, np.abs(ref).max())


# ---- one launch of each PPO family: returns the summed gradient row [actor | critic | 3 objectives ...] --------------------------------
def run_fused(ops, dev, dims, buf, ids, actor, critic, crit, arith=None, objective=0):
    S, h1, h2, A = dims
    B = ids.size
    n_slabs, stride = ops.ppo_num_slabs(B), ops.ppo_slab_stride(S, h1, h2, A)
    slabs, flat = th.full((n_slabs, stride), float("nan"), device=dev), th.zeros(stride, device=dev)
    prev = ops.ppo_set_arith(arith) if arith else None
    try:
        if arith:
            assert ops.ppo_arith_in_use(S, h1, h2, A) == arith
        pa = flat_params(actor)
        both = cu(np.concatenate([pa, flat_params(critic)]), dev)           # [actor | critic], as the wide kernels need them
        ops.ppo_step(both[:pa.size], both[pa.size:], cu(actor.state_avg, dev), cu(actor.state_std, dev),
                     cu(critic.state_avg, dev), cu(critic.state_std, dev), S, h1, h2, A, *[cu(x, dev) for x in buf], cu(ids, dev), 0.25, 0.001,
                     1.0 / B, slabs, n_slabs, objective, criterion=crit)
    finally:
        if arith:
            ops.ppo_set_arith(prev)
    ops.grad_reduce(slabs, n_slabs, stride, flat)
    return flat.cpu().numpy().astype(np.float64)


def run_layered(ops, dev, dims, buf, ids, actor, critic, crit, discrete=False, objective=0):
    spec = ops.MlpSpecN(list(dims), not discrete)
    Pa, Pc = spec.count, ops.MlpSpecN(list(dims[:-1]) + [1], False).count
    flat = th.full((Pa + Pc + 4,), float("nan"), device=dev)
    args = (cu(flat_params(actor), dev), cu(flat_params(critic), dev), cu(actor.state_avg, dev), cu(actor.state_std, dev), cu(critic.state_avg, dev),
            cu(critic.state_std, dev), spec, *[cu(x, dev) for x in buf], cu(ids, dev), 0.25, 0.001, 1.0 / ids.size, flat)
    if discrete:
        ops.mlpn_ppo_step_discrete(*args, criterion=crit)
    else:
        ops.mlpn_ppo_step(*args, objective=objective, criterion=crit)
    return flat.cpu().numpy().astype(np.float64)


def run_fused_discrete(ops, dev, dims, buf, ids, actor, critic, crit):
    S, h1, h2, A = dims
    B = ids.size
    n_slabs, stride = ops.ppo_num_slabs(B), ops.ppo_discrete_slab_stride(S, h1, h2, A)
    slabs, flat = th.full((n_slabs, stride), float("nan"), device=dev), th.zeros(stride, device=dev)
    ops.ppo_step_discrete(cu(flat_params(actor), dev), cu(flat_params(critic), dev), cu(actor.state_avg, dev), cu(actor.state_std, dev),
                          cu(critic.state_avg, dev), cu(critic.state_std, dev), S, h1, h2, A, *[cu(x, dev) for x in buf], cu(ids, dev), 0.25, 0.001,
                          1.0 / B, slabs, n_slabs, criterion=crit)
    ops.grad_reduce(slabs, n_slabs, stride, flat)
    return flat.cpu().numpy().astype(np.float64)


#            id                 dims                       how it is launched                                   the family's MSE bound
FAMILIES = {"generic-fp32": ((5, 32, 96, 2), "fused", None, "kernels"),            # ppo_step.hip
            "w4": ((3, 64, 64, 1), "fused", "f32", "kernels"),
            "s3": ((3, 64, 64, 1), "fused", "split", "split"),
            "s3-tightest": ((64, 128, 128, 8), "fused", "split", "split"),          # the register-tightest instantiation
            "wd": ((3, 256, 64, 1), "fused", None, "wide"),
            "wd3": ((3, 256, 128, 64, 1), "layered", None, "wide"),                 # through ops.mlpn_ppo_step
            "mlpn-one-hidden": ((3, 24, 1), "layered", None, "kernels"),
            "mlpn-three-hidden": ((5, 48, 40, 24, 2), "layered", None, "kernels"),
            "discrete-fused": ((4, 64, 32, 2), "fused-discrete", None, "kernels"),    # CartPole
            "discrete-layered": ((4, 64, 32, 2), "layered-discrete", None, "kernels")}


def launch(ops, dev, how, arith, dims, buf, ids, actor, critic, crit, objective=0):
    if how == "fused":
        return run_fused(ops, dev, dims, buf, ids, actor, critic, crit, arith, objective)
    if how == "fused-discrete":
        return run_fused_discrete(ops, dev, dims, buf, ids, actor, critic, crit)
    return run_layered(ops, dev, dims, buf, ids, actor, critic, crit, discrete=how == "layered-discrete", objective=objective)


def check_ppo(ops, dev, family, kind, B, objective=0, seed=0):
    dims, how, arith, bound = FAMILIES[family]
    discrete = "discrete" in how
    S, A = dims[0], dims[-1]
    rng = np.random.default_rng(1000 * seed + 7 * S + B + kind)
    H, N = 9, 50
    buf, ids = ppo_case(rng, H, N, S, A, B, discrete)
    actor, critic = random_net_n(rng, list(dims), not discrete), random_net_n(rng, list(dims[:-1]) + [1], False)
    name = {0: "reference", 1: "canonical", 2: "a2c"}[objective]
    *_, diff = K.ppo_flat_grads(buf, ids, actor, critic, 0.25, 0.001, K.module(K.MSE, 1.0), name, discrete)
    thr = K.median_threshold(np.abs(diff))
    K.assert_both_arms(np.abs(diff), thr)
    ga, gc, objs, _ = K.ppo_flat_grads(buf, ids, actor, critic, 0.25, 0.001, K.module(kind, thr), name, discrete)
    Pa, Pc = ga.size, gc.size
    got = launch(ops, dev, how, arith, dims, buf, ids, actor, critic, (kind, thr), objective)
    assert np.isfinite(got).all(), "a slab slot was left unwritten"
    errs = {"actor": np.abs(got[:Pa] - ga).max(), "critic": np.abs(got[Pa:Pa + Pc] - gc).max()}
    scales = {"actor": np.abs(ga).max(), "critic": np.abs(gc).max()}
    print(f"{family} kind {kind} B={B} threshold {thr:.6g}: error / scale", {k: errs[k] / max(scales[k], 1e-30) for k in errs},
          "objectives", got[Pa + Pc:Pa + Pc + 3], "fp64", objs)
    if bound == "kernels":           # tests/test_kernels_gpu.py::test_ppo_step_gradients, tests/test_mlpn_gpu.py::test_mlpn_ppo_step_gradients
        for k in errs:
            assert errs[k] <= 1e-4 * scales[k] + 1e-7, f"{k} grad err {errs[k]:.3e} (scale {scales[k]:.3e})"
        np.testing.assert_allclose(got[Pa + Pc:Pa + Pc + 3], objs, rtol=1e-4, atol=1e-6)
    elif bound == "split":           # tests/test_kernels_gpu.py::test_ppo_step_split_arith: at most twice the fp32 kernel's error, floor 1e-6
        g32 = launch(ops, dev, how, "f32", dims, buf, ids, actor, critic, (kind, thr), objective)
        for lo, hi, ref in ((0, Pa, ga), (Pa, Pa + Pc, gc), (Pa + Pc, Pa + Pc + 3, objs)):
            scale = max(1e-30, np.abs(ref).max())
            es, e32 = np.abs(got[lo:hi] - ref).max() / scale, np.abs(g32[lo:hi] - ref).max() / scale
            assert es <= max(2.0 * e32, 1e-6), f"split arithmetic error {es:.3e} against the fp32 kernel's {e32:.3e}"
    else:                            # tests/test_ppo_wide_gpu.py::test_wide_step_objective_forms / test_wide3_step_objective_forms
        assert block_errors(got[:Pa], ga, dims, True) <= 2e-6 and block_errors(got[Pa:Pa + Pc], gc, list(dims[:-1]) + [1], False) <= 2e-6
        np.testing.assert_allclose(got[Pa + Pc:Pa + Pc + 3], objs, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("B", [165, 1])                     # one full 128-sample workgroup plus a 37-row tail; one row
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_ppo_critic_loss_in_every_kernel_family(ops, dev, family, kind, B):
    check_ppo(ops, dev, family, kind, B)


@pytest.mark.parametrize("family", ["generic-fp32", "s3", "wd", "mlpn-three-hidden"])
def test_ppo_critic_loss_under_the_a2c_objective(ops, dev, family):
    check_ppo(ops, dev, family, K.SMOOTH_L1, 165, objective=2, seed=1)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_ppo_all_rows_masked_gives_exact_zeros(ops, dev, family, kind):
    dims, how, arith, _ = FAMILIES[family]
    discrete = "discrete" in how
    rng = np.random.default_rng(5)
    buf, ids = ppo_case(rng, 9, 50, dims[0], dims[-1], 165, discrete, masked=True)
    actor, critic = random_net_n(rng, list(dims), not discrete), random_net_n(rng, list(dims[:-1]) + [1], False)
    got = launch(ops, dev, how, arith, dims, buf, ids, actor, critic, (kind, 0.5))
    Pa = flat_params(actor).size
    Pc = flat_params(critic).size
    assert not got[Pa:Pa + Pc].any() and got[Pa + Pc] == 0.0, "critic gradient / obj_critic of a fully masked minibatch"
    assert not got[:Pa - (0 if discrete else dims[-1])].any() and got[Pa + Pc + 1] == 0.0      # (dL/dstd_log keeps no masked term either)


# ---- SAC ---------------------------------------------------------------------------------------------------------------------------
SAC_CASES = ["layered-one-hidden", "layered-lambda-fit", "layered-is-weight", "fused-narrowest-one-row", "fused-32x48", "fused-is-weight",
             "fused-actor-split-critic-unsplit", "fused-nothing-split", "mod-128x64"]


def _flat(module, slices):
    sd = dict(module.named_parameters())
    return th.cat([sd[n].detach().reshape(-1) for n, _, _ in slices]).contiguous()


def _named(flat, slices):
    flat = flat.cpu().double().numpy()
    return {n: flat[o:o + int(np.prod(shape))].reshape(shape) for n, o, shape in slices}


def sac_device_step(case, x, crit, unmask=None):
    """tests/test_sac_gradients_gpu.py:_device_step under `crit`: one step from zero moments with lr = 0, raw gradients in the first moments"""
    from elegantrl_amd import _hip, ops
    dev = th.device("cuda:0")
    st = x.stepper
    spec = ops.SacSpec(case.S, case.A, case.hidden, case.E, actor_variant=_hip.SAC_ACTOR_FIX if C.is_mod(case) else _hip.SAC_ACTOR_SAC)
    sa, sc = spec.actor_slices(), spec.critic_slices()
    pa, pc, pt = (_flat(m, s).to(dev) for m, s in ((st.act, sa), (st.cri, sc), (st.cri_target, sc)))
    pat = pa.clone() + 0.125 if (case.entry == "mod" or case.actor_target) else None
    alpha = st.alpha_log.detach().clone().to(dev)
    mom = [th.zeros_like(pa), th.zeros_like(pa), th.zeros_like(pc), th.zeros_like(pc), th.zeros(1, device=dev), th.zeros(1, device=dev)]
    objs, td = th.full((2,), -7.0, device=dev), th.full((case.B,), -7.0, device=dev)
    put = lambda t: None if t is None else t.to(dev).contiguous()  # noqa: E731
    common = dict(gamma=C.GAMMA, target_entropy=st.target_entropy, tau=C.TAU, lr=0.0, max_norm=C.RAW, objs_out=objs, betas=C.BETAS,
                  noises=(put(x.eps_next), put(x.eps_cur)), is_weight=put(x.is_weight), td_error_out=td, criterion=crit)
    batch = [put(t) for t in x.batch]
    if unmask is not None:
        batch[4] = put(unmask)
    if case.entry == "mod":
        ops.sac_update_mod(spec, pa, pc, pt, alpha, mom, batch, 1, update_actor=case.update_actor, actor_step=1, actor_target=pat, **common)
    else:
        ops.sac_update(spec, pa, pc, pt, alpha, mom, batch, 1, cum_reward=put(x.cum_reward), lambda_fit_cum_r=case.lambda_fit,
                       actor_target=pat, **common)
    th.cuda.synchronize()
    _hip.check_async_faults()
    return dict(sc=sc, mom=[m.cpu() for m in mom], pt=pt.cpu(), pat=None if pat is None else pat.cpu(), objs=objs.cpu(), td=td.cpu())


def _sac_inputs(name):
    prev = th.is_grad_enabled()
    th.set_grad_enabled(True)
    try:
        case = C.CASES[name]
        x = C.make_inputs(case)
        (_, i_mse), _ = K.sac_references(case, x, K.module(K.MSE, 1.0))
        thr = K.median_threshold(np.abs(i_mse["diff"]))
        K.assert_both_arms(np.abs(i_mse["diff"]), thr)
        return case, x, thr, K.sac_references(case, x, K.module(K.HUBER, thr))
    finally:
        th.set_grad_enabled(prev)


@pytest.mark.parametrize("name", SAC_CASES)
def test_sac_huber_critic_gradients_match_fp64(name):
    """the Huber twin of a tests/sac_gradient_cases.py case: critic gradients under its regime-A bound, obj_critic and td_error_out under
    tests/test_sac_gradients_gpu.py's bookkeeping tolerances; everything the criterion cannot reach (lr = 0: the actor's and the
    temperature's gradients, the targets, obj_actor) bit-identical to the same call under MSE"""
    case, x, thr, ((r64, i64), (r32, _)) = _sac_inputs(name)
    out = sac_device_step(case, x, (K.HUBER, thr))
    critic = C.groups_of(r64)["critic"]
    C.compare(name + " huber", "A", _named(out["mom"][2], out["sc"]), {k: r64[k] for k in critic}, {k: r32[k] for k in critic})
    got_obj, got_td, ref_td = float(out["objs"][0]), out["td"].double().numpy(), i64["td_error"].numpy()
    assert abs(got_obj - i64["obj_critic"]) <= 3e-4 * abs(i64["obj_critic"]) + 3e-6, (got_obj, i64["obj_critic"])
    assert np.abs(got_td - ref_td).max() <= 3e-4 * np.abs(ref_td).max() + 1e-6
    mse = sac_device_step(case, x, (K.MSE, 1.0))
    for i in (0, 1, 4, 5):
        assert th.equal(out["mom"][i], mse["mom"][i]), f"moment block {i} depends on the criterion"
    assert th.equal(out["pt"], mse["pt"]) and th.equal(out["objs"][1:], mse["objs"][1:])
    assert out["pat"] is None or th.equal(out["pat"], mse["pat"])
    assert not th.equal(out["mom"][2], mse["mom"][2]), "the critic's gradient ignores the criterion"


@pytest.mark.parametrize("name", ["layered-lambda-fit", "fused-32x48", "mod-128x64"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_sac_all_rows_masked_gives_exact_zeros(name, kind):
    case = C.CASES[name]._replace(lambda_fit=0.0)
    x = C.make_inputs(case)
    x = x._replace(cum_reward=None)
    out = sac_device_step(case, x, (kind, 0.5), unmask=th.zeros(case.B))
    assert not out["mom"][2].any() and not out["mom"][3].any() and float(out["objs"][0]) == 0.0 and not out["td"].any()


# ---- the one-call loops carry the criterion --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("discrete", [False, True], ids=["ppo_update", "ppo_update_discrete"])
def test_ppo_update_loops_are_bitwise_the_loop_of_their_steps_under_smooth_l1(ops, dev, discrete):
    dims = (4, 64, 32, 2) if discrete else (6, 64, 64, 2)
    S, h1, h2, A = dims
    rng = np.random.default_rng(11)
    H, N, B, T = 9, 50, 165, 3
    buf, _ = ppo_case(rng, H, N, S, A, B, discrete)
    ids = cu(rng.integers(0, H * N, size=(T, B)).astype(np.int64), dev)
    actor, critic = random_net_n(rng, list(dims), not discrete), random_net_n(rng, [S, h1, h2, 1], False)
    crit = (K.SMOOTH_L1, 0.5)
    Pa, Pc = flat_params(actor).size, flat_params(critic).size
    stride = ops.ppo_discrete_slab_stride(*dims) if discrete else ops.ppo_slab_stride(*dims)
    n_slabs = ops.ppo_num_slabs(B)
    norms = [cu(x, dev) for x in (actor.state_avg, actor.state_std, critic.state_avg, critic.state_std)]
    dbuf = [cu(x, dev) for x in buf]
    groups = [(0, Pa), (Pa, Pc)]
    results = []
    for one_call in (True, False):
        flat = cu(np.concatenate([flat_params(actor), flat_params(critic)]), dev)
        m1, m2 = th.zeros_like(flat), th.zeros_like(flat)
        slabs, grads = th.zeros((n_slabs, stride), device=dev), th.zeros((T, stride), device=dev)
        if one_call:
            (ops.ppo_update_discrete if discrete else ops.ppo_update)(flat, m1, m2, *norms, S, h1, h2, A, *dbuf, ids, 0.25, 0.001, slabs, grads, 1,
                                                                    1e-3, 3.0, criterion=crit)
        else:
            for k in range(T):
                (ops.ppo_step_discrete if discrete else ops.ppo_step)(flat[:Pa], flat[Pa:], *norms, S, h1, h2, A, *dbuf, ids[k], 0.25, 0.001,
                                                                      float(np.float32(1.0 / B)), slabs, n_slabs, criterion=crit)
                ops.grad_reduce(slabs, n_slabs, stride, grads[k])
                ops.grad_sq_partials(grads[k], stride, groups, 1.0)
                ops.clip_adam_partials(flat, grads[k], m1, m2, stride, groups, 1 + k, 1e-3, 3.0)
        results.append((flat.cpu(), m1.cpu(), grads.cpu()))
    for a, b in zip(*results):
        assert th.equal(a, b)
    # and the criterion reached the loop: under MSE the same call leaves other weights
    flat = cu(np.concatenate([flat_params(actor), flat_params(critic)]), dev)
    m1, m2 = th.zeros_like(flat), th.zeros_like(flat)
    slabs, grads = th.zeros((n_slabs, stride), device=dev), th.zeros((T, stride), device=dev)
    (ops.ppo_update_discrete if discrete else ops.ppo_update)(flat, m1, m2, *norms, S, h1, h2, A, *dbuf, ids, 0.25, 0.001, slabs, grads, 1, 1e-3, 3.0)
    assert not th.equal(flat.cpu()[Pa:], results[0][0][Pa:]) and th.equal(grads.cpu()[0, :Pa], results[0][2][0, :Pa])


# ---- agents ------------------------------------------------------------------------------------------------------------------------
def _ppo_agent(criterion, seed=0):
    from elegantrl_amd.agents import AgentPPO
    from elegantrl_amd.envs import SynVecEnv
    from elegantrl_amd.train import Config
    N, S, A, H, B = 128, 24, 4, 8, 96
    args = Config(AgentPPO, SynVecEnv, {"env_name": "SynVecEnv", "num_envs": N, "max_step": 4, "state_dim": S, "action_dim": A, "if_discrete": False})
    args.net_dims = [64, 64]
    args.horizon_len, args.batch_size, args.repeat_times, args.learning_rate = H, B, 2 * B / H, 1e-3
    if criterion is not None:
        args.criterion = criterion
    th.manual_seed(seed)
    agent = AgentPPO(args.net_dims, S, A, gpu_id=0, args=args)
    env = SynVecEnv(N, S, A, max_step=4, gpu_id=0, seed=1)
    agent.last_state = env.reset()[0]
    g = th.Generator(device="cuda:0").manual_seed(2)
    noise = th.randn((H, N, A), device="cuda:0", generator=g)
    items = agent._explore_vec_env(env, H, noise=noise)
    ids = th.randint(H * N, (2, B), device="cuda:0", generator=g)
    return agent, args, [x.clone() for x in items], noise, ids


@pytest.mark.parametrize("crit", [th.nn.SmoothL1Loss(reduction="none"), th.nn.HuberLoss(reduction="none"), th.nn.MSELoss(reduction="none")],
                         ids=["smooth_l1", "huber", "mse-control"])
def test_agent_ppo_update_net_under_a_criterion_matches_the_oracle(monkeypatch, crit):
    """one AgentPPO.update_net at net (64, 64), B = 96 under the criterion (torch's default beta / delta) against the oracle's minibatch
    step with the helper's critic objective swapped in; tolerances of tests/test_mlpn_gpu.py's agent test.  MSE runs the same set-up as
    the control."""
    agent, args, items, noise, ids = _ppo_agent(crit)
    assert agent.criterion is crit and agent.criterion_code[1] == 1.0
    states, actions, logprobs, rewards, undones, unmasks = [x.clone() for x in items]      # (update_net applies get_advantages' fix-up in place)
    f = lambda t: t.detach().cpu().numpy().astype(np.float64)  # noqa: E731

    def to_mlp(net, with_std):
        return O.Mlp([f(net.net[i].weight) for i in (0, 2, 4)], [f(net.net[i].bias) for i in (0, 2, 4)], f(net.state_avg), f(net.state_std),
                     f(net.action_std_log).reshape(-1) if with_std else None)

    actor, critic = to_mlp(agent.act, True), to_mlp(agent.cri, False)
    objs = agent.update_net(list(items), ids=ids)
    v = O.critic_value(f(states), critic)
    nv = O.critic_value(f(agent.last_state), critic)
    adv, _, _ = O.gae_scan(f(rewards), undones.cpu().numpy(), unmasks.cpu().numpy(), v, nv, args.gamma, 0.95)
    buf = (f(states), f(actions), unmasks.cpu().numpy(), f(logprobs), O.adv_normalize(adv), O.reward_sums(adv, v))
    monkeypatch.setattr(O, "critic_objective", K.ppo_critic_objective(crit))
    sa, sc = O.AdamState(), O.AdamState()
    ref = np.mean([O.ppo_minibatch_step(buf, i.cpu().numpy(), actor, critic, sa, sc, lr=args.learning_rate, max_norm=3.0, ratio_clip=0.25,
                                        lambda_entropy=0.001) for i in ids], axis=0)
    print("objectives", objs, "oracle", ref)
    np.testing.assert_allclose(np.array(objs), ref, rtol=5e-4, atol=5e-6)
    np.testing.assert_allclose(agent.act.net[0].weight.detach().cpu().numpy(), actor.weights[0], rtol=0, atol=2e-5)
    np.testing.assert_allclose(agent.cri.net[4].weight.detach().cpu().numpy(), critic.weights[2], rtol=0, atol=2e-5)
    # it is not what MSE leaves, and the route is MSE's
    mse_agent, _, mse_items, _, mse_ids = _ppo_agent(None)
    mse_agent.update_net(list(mse_items), ids=mse_ids)
    assert th.equal(mse_agent.cri.net[4].weight, agent.cri.net[4].weight) == (agent.criterion_code[0] == K.MSE)
    assert mse_agent.kernel_path == agent.kernel_path and getattr(mse_agent, "update_path", None) == getattr(agent, "update_path", None)


def test_an_explicit_mse_criterion_ends_bit_identical_to_none():
    ends = []
    for crit in (None, th.nn.MSELoss(reduction="none")):
        agent, _, items, _, ids = _ppo_agent(crit)
        objs = agent.update_net(list(items), ids=ids)
        ends.append((objs, agent._flat.clone(), (agent.kernel_path, getattr(agent, "update_path", None))))
    assert ends[0][0] == ends[1][0] and th.equal(ends[0][1], ends[1][1]) and ends[0][2] == ends[1][2]


# ---- every route of every agent hands the criterion to its library entry ---------------------------------------------------------------
@pytest.fixture
def entry_log(monkeypatch):
    """spies on the library's own entries (the ctypes handle): every erl_criterion_next_call and every update entry, in call order"""
    from elegantrl_amd import _hip
    L, log = _hip.lib(), []

    def spy(name, fn):
        def call(*a):
            log.append((name, a[:2]) if name == "erl_criterion_next_call" else (name, None))
            return fn(*a)
        return call
    for name in K.UPDATE_ENTRIES + ("erl_criterion_next_call",):
        monkeypatch.setattr(L, name, spy(name, getattr(L, name)))
    return log


def handed(log):
    """[(update entry, the criterion named for it)]: what the last erl_criterion_next_call before the entry said, MSE when nothing did"""
    out, pending = [], (K.MSE, 1.0)
    for name, crit in log:
        if name == "erl_criterion_next_call":
            pending = (int(crit[0]), float(crit[1]))
        else:
            out.append((name, pending))
            pending = (K.MSE, 1.0)
    return out


SMOOTH = lambda: th.nn.SmoothL1Loss(reduction="none", beta=0.5)  # noqa: E731


def ppo_family_update(cls_name, crit, net, **flags):
    """one update_net (two minibatches) of a PPO-family agent on a synthetic rollout; returns the agent"""
    import elegantrl_amd.agents as agents
    from elegantrl_amd.train import Config
    cls, discrete, a2c = getattr(agents, cls_name), "Discrete" in cls_name, cls_name == "AgentA2C"
    S, A = 6, 2
    N, H, B = (1, 64, 32) if a2c else (24, 8, 96)
    args = Config(cls, None, {"env_name": "synthetic", "num_envs": N, "max_step": 100, "state_dim": S, "action_dim": A, "if_discrete": discrete})
    args.net_dims, args.quiet = list(net), True
    args.horizon_len, args.batch_size, args.repeat_times = H, B, 2 * B / H
    if crit is not None:
        args.criterion = crit
    for k, v in flags.items():
        setattr(args, k, v)
    th.manual_seed(0)
    agent = cls(args.net_dims, S, A, gpu_id=0, args=args)
    g = th.Generator(device="cuda:0").manual_seed(3)
    rn = lambda *shape: th.randn(shape, device="cuda:0", generator=g)  # noqa: E731
    ru = lambda *shape: th.rand(shape, device="cuda:0", generator=g)  # noqa: E731
    actions = th.randint(A, (H, N), device="cuda:0", generator=g).to(th.int32) if discrete else 0.7 * rn(H, N, A)
    buf = [rn(H, N, S), actions, (-0.7 if discrete else -1.0 * A) + 0.3 * rn(H, N), rn(H, N), ru(H, N) > 0.05, ru(H, N) > 0.125]
    agent.last_state = rn(N, S)
    ids = th.randint(H * N, (2, B), device="cuda:0", generator=g)
    agent.update_net(buf, ids=ids)
    return agent


#              agent               net           flags                      the entry the route calls
PPO_ROUTES = [("AgentPPO", (64, 64), {}, "erl_ppo_update_dp_f32"),                          # the one-call loop on the fused kernel
              ("AgentPPO", (48, 40, 24), {}, "erl_mlpn_ppo_step_f32"),                      # the layered loop
              ("AgentPPO", (64, 64), {"dp": True}, "erl_ppo_step_f32"),                     # the data-parallel loop through torch.distributed
              ("AgentA2C", (64, 64), {}, "erl_ppo_update_dp_f32"),
              ("AgentA2C", (24,), {}, "erl_mlpn_ppo_step_f32"),
              ("AgentDiscretePPO", (64, 32), {"fused_update": True}, "erl_ppo_update_discrete_f32"),
              ("AgentDiscretePPO", (64, 32), {"fused_update": False}, "erl_mlpn_ppo_step_discrete_f32"),
              ("AgentDiscreteA2C", (64, 32), {"fused_update": True}, "erl_ppo_update_discrete_f32"),
              ("AgentDiscreteA2C", (64, 32), {"fused_update": False}, "erl_mlpn_ppo_step_discrete_f32")]


@pytest.mark.parametrize("cls_name,net,flags,entry", PPO_ROUTES, ids=[f"{r[0]}-{r[3]}" for r in PPO_ROUTES])
def test_ppo_family_routes_hand_the_criterion_to_their_entry(entry_log, monkeypatch, cls_name, net, flags, entry):
    flags = dict(flags)
    if flags.pop("dp", False):
        from elegantrl_amd import parallel
        monkeypatch.setattr(parallel, "force_dp", lambda: True)                      # the data-parallel code path with one rank ...
        monkeypatch.setattr(parallel, "gradient_comm", lambda count=None: None)      # ... on the torch.distributed route (identity here)
    agent = ppo_family_update(cls_name, SMOOTH(), net, **flags)
    got = handed(entry_log)
    assert got and {n for n, _ in got} == {entry}, got
    assert all(c == (K.SMOOTH_L1, 0.5) for _, c in got), got
    del entry_log[:]
    mse = ppo_family_update(cls_name, None, net, **flags)
    assert [n for n, _ in handed(entry_log)] == [n for n, _ in got] and all(c == (K.MSE, 1.0) for _, c in handed(entry_log))
    assert getattr(mse, "update_path", None) == getattr(agent, "update_path", None) and mse.kernel_path == agent.kernel_path
    assert not th.equal(mse._flat, agent._flat)


def sac_update(cls_name, crit, per=False, loops=1, **flags):
    """AgentSAC / AgentModSAC at net (64, 48), batch 96, 16 envs: a rollout of 40 steps into a ring of 80 rows, then `loops` x [update_net of
    three steps]; the sample ids (or the prioritised sampler's uniforms) are the same for every caller.  Returns (agent, buffer, objectives)"""
    import elegantrl_amd.agents as agents
    from elegantrl_amd.envs import SynVecEnv
    from elegantrl_amd.train import Config, ReplayBuffer
    cls = getattr(agents, cls_name)
    N, S, A, H, B = 16, 11, 3, 40, 96
    args = Config(cls, SynVecEnv, {"env_name": "SynVecEnv", "num_envs": N, "max_step": 50, "state_dim": S, "action_dim": A, "if_discrete": False})
    args.net_dims, args.horizon_len, args.batch_size, args.random_seed, args.quiet = [64, 48], H, B, 3, True
    args.repeat_times = 3.1 * B / H                                 # update_times = int(cur_size * repeat_times / batch_size) = 3
    args.if_use_per = per
    if crit is not None:
        args.criterion = crit
    for k, v in flags.items():
        setattr(args, k, v)
    th.manual_seed(5)
    agent = cls(args.net_dims, S, A, gpu_id=0, args=args)
    env = SynVecEnv(N, S, A, max_step=50, gpu_id=0, seed=1)
    agent.last_state = env.reset()[0]
    buf = ReplayBuffer(max_size=2 * H, state_dim=S, action_dim=A, gpu_id=0, num_seqs=N, if_use_per=per, args=args)
    prev = th.is_grad_enabled()
    th.set_grad_enabled(False)
    try:
        buf.update(agent.explore_env(env, H))
        g = th.Generator(device="cuda:0").manual_seed(9)
        out = []
        for _ in range(loops):
            th.manual_seed(9)
            uni = th.rand((3, N, B // N), device="cuda:0", generator=g) if per else None
            out.append(agent.update_net(buf, per_uniform=uni) if per else agent.update_net(buf))
    finally:
        th.set_grad_enabled(prev)
    return agent, buf, out


#              agent          per    flags                                              the entry the route calls
SAC_ROUTES = [("AgentSAC", False, {}, "erl_sac_update_ring_loop_f32"),
              ("AgentSAC", False, {"update_loop_in_c": False}, "erl_sac_update_ring_f32"),
              ("AgentSAC", False, {"sample_in_step": False}, "erl_sac_update_f32"),
              ("AgentSAC", False, {"lambda_fit_cum_r": 0.5}, "erl_sac_update_f32"),             # the layered step with the fit term
              ("AgentSAC", True, {}, "erl_sac_update_per_loop_f32"),
              ("AgentSAC", True, {"per_draw_in_step": True}, "erl_sac_update_per_draw_loop_f32"),
              ("AgentSAC", True, {"per_loop_in_c": False}, "erl_sac_update_f32"),
              ("AgentModSAC", False, {}, "erl_sac_update_opt_f32"),                             # the layered step
              ("AgentModSAC", False, {"fused_step": True}, "erl_sac_update_mod_ring_loop_f32"),
              ("AgentModSAC", False, {"fused_step": True, "update_loop_in_c": False}, "erl_sac_update_mod_ring_f32"),
              ("AgentModSAC", False, {"fused_step": True, "sample_in_step": False}, "erl_sac_update_mod_f32"),
              ("AgentModSAC", True, {"fused_step": True, "mod_per_loop_in_c": True}, "erl_sac_update_mod_per_loop_f32")]


@pytest.mark.parametrize("cls_name,per,flags,entry", SAC_ROUTES, ids=[f"{r[0]}-{'per-' if r[1] else ''}{r[3]}-{len(r[2])}" for r in SAC_ROUTES])
def test_sac_routes_hand_the_criterion_to_their_entry(entry_log, cls_name, per, flags, entry):
    agent, _, _ = sac_update(cls_name, SMOOTH(), per, **flags)
    got = handed(entry_log)
    assert got and {n for n, _ in got} == {entry}, got
    assert all(c == (K.SMOOTH_L1, 0.5) for _, c in got), got
    del entry_log[:]
    mse, _, _ = sac_update(cls_name, None, per, **flags)
    assert [n for n, _ in handed(entry_log)] == [n for n, _ in got] and all(c == (K.MSE, 1.0) for _, c in handed(entry_log))
    assert mse.update_path == agent.update_path and mse.per_path == agent.per_path and mse.kernel_path == agent.kernel_path
    assert not th.equal(mse._critic_flat, agent._critic_flat)


SAC_LOOPS = [("AgentSAC", False, {}, {"update_loop_in_c": False}),                                  # ops.sac_update_ring_loop against sac_update_from_ring
             ("AgentModSAC", False, {"fused_step": True}, {"fused_step": True, "update_loop_in_c": False}),      # ops.sac_update_mod_ring_loop
             ("AgentSAC", True, {}, {"per_loop_in_c": False})]                                      # ops.sac_update_per_loop against the per-step route


@pytest.mark.parametrize("cls_name,per,loop_flags,step_flags", SAC_LOOPS, ids=["sac_update_ring_loop", "sac_update_mod_ring_loop", "sac_update_per_loop"])
def test_sac_one_call_loops_are_bitwise_the_loop_of_their_steps_under_smooth_l1(cls_name, per, loop_flags, step_flags):
    """three steps from one C call against the same three steps one call each, Smooth-L1 (beta 0.5), two update_net in a row: weights,
    moments, temperature, objectives per step and, prioritised, the td errors and the trees (the second update_net draws from the
    priorities the first one wrote: they are the criterion's values)"""
    (a, ba, oa), (b, bb, ob) = sac_update(cls_name, SMOOTH(), per, loops=2, **loop_flags), sac_update(cls_name, SMOOTH(), per, loops=2, **step_flags)
    assert a.update_path != b.update_path or a.per_path != b.per_path
    assert oa == ob and all(np.isfinite(x) for pair in oa for x in pair)
    for name in ("_actor_flat", "_critic_flat", "_target_flat", "alpha_log", "objs_all"):       # (bit patterns: a skipped actor step logs nan)
        assert th.equal(getattr(a, name).view(th.int32), getattr(b, name).view(th.int32)), name
    for x, y in zip(a._moments(), b._moments()):
        assert th.equal(x, y)
    if per:
        assert th.equal(a._td_error, b._td_error) and th.equal(ba.sum_trees.sum, bb.sum_trees.sum) and th.equal(ba.sum_trees.min, bb.sum_trees.min)
        m, bm, _ = sac_update(cls_name, None, per, loops=2, **loop_flags)
        assert not th.equal(m._td_error, a._td_error) and not th.equal(bm.sum_trees.sum, ba.sum_trees.sum)


def test_agent_sac_step_under_smooth_l1_matches_the_oracle():
    """one AgentSAC step at net (64, 48), B = 96 under SmoothL1Loss(reduction='none') (torch's default beta) against the oracle's step
    with the criterion in it (tests/criterion_cases.py:sac_stepper_under); tolerances of tests/test_sac.py's step test"""
    from oracle.sac_torch import SacStepper
    crit = th.nn.SmoothL1Loss(reduction="none")
    agent, buf, _ = sac_update("AgentSAC", crit, loops=0, learning_rate=1e-3)
    assert agent.criterion_code == (K.SMOOTH_L1, 1.0)
    B, S, A = agent.batch_size, agent.state_dim, agent.action_dim
    prev = th.is_grad_enabled()
    th.set_grad_enabled(True)
    try:
        th.manual_seed(21)
        st = K.sac_stepper_under(crit, SacStepper)([64, 48], S, A, agent.num_ensembles, lr=1e-3, gamma=float(agent.gamma),
                                                   tau=float(agent.soft_update_tau), max_norm=float(agent.clip_grad_norm))
        with th.no_grad():
            for p in st.cri_target.parameters():
                p.add_(0.05 * th.randn_like(p))
            for mine, theirs in ((agent.act, st.act), (agent.cri, st.cri), (agent.cri_target, st.cri_target)):
                mine.load_state_dict(theirs.state_dict())
        g = th.Generator(device="cuda:0").manual_seed(4)
        ids = th.randint((buf.cur_size - 1) * buf.num_seqs, (B,), device="cuda:0", generator=g)
        e_next, e_cur = th.randn((B, A), device="cuda:0", generator=g), th.randn((B, A), device="cuda:0", generator=g)
        batch = tuple(x.clone().cpu() for x in buf.sample(B, ids=ids))
        with th.no_grad():
            objs = agent.update_objectives(buf, 0, ids=ids, noises=(e_next, e_cur))
        ref = st.step(batch, e_next.cpu(), e_cur.cpu())
    finally:
        th.set_grad_enabled(prev)
    print("objectives", objs, "oracle", ref)
    np.testing.assert_allclose(np.array(objs), ref, rtol=3e-4, atol=3e-6)
    for mine, theirs in ((agent.act, st.act), (agent.cri, st.cri), (agent.cri_target, st.cri_target)):
        sd = theirs.state_dict()
        diff = np.concatenate([(v.detach().cpu() - sd[k]).abs().numpy().reshape(-1) for k, v in mine.state_dict().items()])
        assert (diff <= 5e-5).mean() >= 0.995, f"{(diff > 5e-5).mean():.4%} of the block is off"
        assert diff.max() <= 2.2 * 1e-3
    np.testing.assert_allclose(agent.alpha_log.cpu().numpy(), st.alpha_log.detach().numpy(), rtol=0, atol=1e-5)
