"""Raw gradients of every kernel form of the SAC step (csrc/sac.hip's layered step, csrc/sac_fused.hip's fused step for AgentSAC and
AgentModSAC) against the fp64 restatement oracle/sac_torch.py:step_gradients, tensor by tensor.  The other SAC tests look at the backward
pass through Adam, which hides a gradient's size, the clip norm and a few wrong elements; here one step from zero moments with
betas = (0, 0.999), lr = 0, step = 1 leaves the (clipped) gradients themselves in the first moments (tests/sac_gradient_cases.py: the cases,
the two regimes and their bounds; tests/test_sac_gradients_cpu.py: the comparison catches what it is meant to catch)."""
import numpy as np
import pytest
import torch as th

from tests import sac_gradient_cases as C

pytestmark = pytest.mark.gpu

def _reference(name):
    """inputs and both restatements of a case"""
    prev = th.is_grad_enabled()
    th.set_grad_enabled(True)               # (train_agent() in an earlier test leaves autograd switched off)
    try:
        case = C.CASES[name]
        x = C.make_inputs(case)
        return (x, *C.references(case, x))
    finally:
        th.set_grad_enabled(prev)


def _flat(module, slices):
    sd = dict(module.named_parameters())
    return th.cat([sd[n].detach().reshape(-1) for n, _, _ in slices]).contiguous()


def _named(flat, slices):
    flat = flat.cpu().double().numpy()
    return {n: flat[o:o + int(np.prod(shape))].reshape(shape) for n, o, shape in slices}


def _device_step(case, x, max_norm):
    """one step of the case's entry from zero moments; returns every block before and after, on the host"""
    from elegantrl_amd import _hip, ops
    dev = th.device("cuda:0")
    st = x.stepper
    spec = ops.SacSpec(case.S, case.A, case.hidden, case.E, actor_variant=_hip.SAC_ACTOR_FIX if C.is_mod(case) else _hip.SAC_ACTOR_SAC)
    sa, sc = spec.actor_slices(), spec.critic_slices()
    pa0, pc0, pt0 = _flat(st.act, sa), _flat(st.cri, sc), _flat(st.cri_target, sc)
    assert pa0.numel() == spec.actor_count and pc0.numel() == spec.critic_count
    pa, pc, pt = pa0.to(dev), pc0.to(dev), pt0.to(dev)
    with_target = case.entry == "mod" or case.actor_target
    pat = pa.clone() + 0.125 if with_target else None                     # (an actor target that differs from the actor)
    alpha = st.alpha_log.detach().clone().to(dev)
    mom = [th.zeros_like(pa), th.zeros_like(pa), th.zeros_like(pc), th.zeros_like(pc), th.zeros(1, device=dev), th.zeros(1, device=dev)]
    objs, td = th.full((2,), -7.0, device=dev), th.full((case.B,), -7.0, device=dev)
    put = lambda t: None if t is None else t.to(dev).contiguous()  # noqa: E731
    common = dict(gamma=C.GAMMA, target_entropy=st.target_entropy, tau=C.TAU, lr=0.0, max_norm=max_norm, objs_out=objs, betas=C.BETAS,
                  noises=(put(x.eps_next), put(x.eps_cur)), is_weight=put(x.is_weight), td_error_out=td)
    batch = [put(t) for t in x.batch]
    if case.entry == "mod":
        assert ops.sac_mod_fused_supported(spec, case.B)
        ops.sac_update_mod(spec, pa, pc, pt, alpha, mom, batch, 1, update_actor=case.update_actor, actor_step=1, actor_target=pat, **common)
    else:
        ops.sac_update(spec, pa, pc, pt, alpha, mom, batch, 1, cum_reward=put(x.cum_reward), lambda_fit_cum_r=case.lambda_fit,
                       actor_target=pat, **common)
    th.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu()  # noqa: E731
    return dict(sa=sa, sc=sc, pa0=pa0, pc0=pc0, pt0=pt0, pa=host(pa), pc=host(pc), pt=host(pt), pat=host(pat), alpha=host(alpha),
                mom=[host(m) for m in mom], objs=objs.cpu().numpy(), td=td.cpu().numpy())


def _moments(case, out):
    """the first moments as named gradients, in the reference's names"""
    got = _named(out["mom"][2], out["sc"])
    if case.update_actor:
        got.update(_named(out["mom"][0], out["sa"]))
    got["alpha_log"] = out["mom"][4].double().numpy()
    return got


def _check_bookkeeping(case, x, out, info64, info32):
    """what the step has to leave besides the gradients"""
    st, tau = x.stepper, C.TAU
    one_minus_beta2 = np.float32(1.0) - np.float32(C.BETAS[1])
    for m, v in ((out["mom"][0], out["mom"][1]), (out["mom"][2], out["mom"][3]), (out["mom"][4], out["mom"][5])):
        m, v = m.numpy(), v.numpy()
        want = one_minus_beta2 * (m * m)                                  # erl_adam_update's two fp32 roundings
        # 2 ulp; below the smallest normal number a product may have been flushed to zero
        assert (np.abs(v - want) <= 2 * np.spacing(np.abs(want)) + np.finfo(np.float32).tiny).all(), "second moment != (1 - beta2) g^2"
    assert th.equal(out["pa"], out["pa0"]) and th.equal(out["pc"], out["pc0"]), "lr = 0 moved a parameter"
    assert th.equal(out["alpha"], st.alpha_log.detach()), "lr = 0 moved alpha_log"
    if not case.update_actor:
        assert not out["mom"][0].any() and not out["mom"][1].any() and np.isnan(out["objs"][1])
    c, t = out["pc0"].double().numpy(), out["pt0"].double().numpy()
    # rtol 1e-6 of the result, plus one fp32 rounding of each product (their sum may cancel where critic and target differ in sign)
    slack = 2.0 ** -23 * (np.abs(tau * c) + np.abs((1 - tau) * t))
    want = tau * c + (1 - tau) * t
    assert (np.abs(out["pt"].double().numpy() - want) <= 1e-6 * np.abs(want) + slack).all(), "critic target soft update"
    if out["pat"] is not None:
        a, at = out["pa0"].double().numpy(), out["pa0"].double().numpy() + 0.125
        if case.update_actor:
            want = tau * a + (1 - tau) * at
            slack = 2.0 ** -23 * (np.abs(tau * a) + np.abs((1 - tau) * at))
            assert (np.abs(out["pat"].double().numpy() - want) <= 1e-6 * np.abs(want) + slack).all(), "actor target soft update"
        else:
            assert th.equal(out["pat"], out["pa0"] + 0.125), "a skipped actor step moved the actor target"
    # objectives and td errors: tests/test_sac.py's tolerances, taken at the largest element; where fp32 itself is further than that from
    # fp64 (regime B), 8 x the fp32 restatement's own error, as for the gradients
    for what, got, r64, r32, atol in (("objectives", out["objs"], [info64["obj_critic"], info64["obj_actor"]], [info32["obj_critic"], info32["obj_actor"]], 3e-6),
                                      ("td_error", out["td"], info64["td_error"].numpy(), info32["td_error"].double().numpy(), 1e-6)):
        got, r64, r32 = (np.asarray(v, np.float64) for v in (got, r64, r32))
        assert np.array_equal(np.isnan(got), np.isnan(r64)), what
        err, err32 = np.nanmax(np.abs(got - r64)), np.nanmax(np.abs(r32 - r64))
        allowed = 3e-4 * np.nanmax(np.abs(r64)) + atol
        assert err <= (max(allowed, 8.0 * err32) if case.regime == "B" else allowed), f"{what}: {err:.3e} from fp64, fp32 restatement {err32:.3e}"


@pytest.mark.parametrize("name", list(C.CASES))
def test_sac_step_gradients_match_fp64(name):
    """Per case (tests/sac_gradient_cases.py CASES: which launch each reaches): raw gradients per named tensor of the actor, the critic and
    alpha_log under the regime's bound, with the fp32 restatement's own error printed next to the device's; second moments, untouched
    parameters, the soft-updated targets; then a second step on fresh moments with max_norm = a quarter of the smaller fp64 block norm --
    the only place where the extent of the clip norm shows."""
    from elegantrl_amd import _hip
    case = C.CASES[name]
    x, (r64, i64), (r32, i32) = _reference(name)
    edge = C.edge_distance(case, i64)
    assert edge > C.EDGE, f"a pre-clamp log_std lies {edge:.2e} from a clamp edge: choose another seed"
    assert float(x.batch[3].sum()) >= 1 and float(x.batch[4].sum()) >= 1
    out = _device_step(case, x, C.RAW)
    _hip.check_async_faults()                   # a timed-out exchange fails the case instead of passing on stale shares
    C.compare(name + " raw", case.regime, _moments(case, out), r64, r32)
    _check_bookkeeping(case, x, out, i64, i32)
    mn = C.clip_max_norm(r64)
    groups = C.groups_of(r64)
    assert all(C.norm(r64, groups[k]) > 2 * mn for k in ("actor", "critic") if k in groups)              # both blocks really clip
    out = _device_step(case, x, mn)
    _hip.check_async_faults()
    C.compare(name + " clipped", case.regime, _moments(case, out), C.clipped(r64, mn), C.clipped(r32, mn))
