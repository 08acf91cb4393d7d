"""oracle/sac_torch.py:step_gradients pinned to the restatement the golden files pin (SacStepper.step / ModSacStepper.step), and the
comparison of tests/test_sac_gradients_gpu.py run on the CPU with the fp32 restatement standing in for the device: it passes as it is and
fails for four mutations that the Adam-filtered SAC tests cannot see."""
import numpy as np
import pytest
import torch as th

from tests import sac_gradient_cases as C


@pytest.fixture(autouse=True)
def _autograd_on():
    prev = th.is_grad_enabled()
    th.set_grad_enabled(True)
    yield
    th.set_grad_enabled(prev)


PINNED = {
    "SacStepper-64x48": C.Case("sac", (64, 48), 2, 100),
    "SacStepper-64x48x32": C.Case("sac", (64, 48, 32), 2, 130, S=17, A=6),
    "SacStepper-is-weight-lambda-fit": C.Case("sac", (64, 48), 4, 96, is_weight=True, lambda_fit=0.5),
    "SacStepper-saturating": C.Case("sac", (64, 48), 2, 100, regime="B"),
    "ModSacStepper-64x32": C.Case("mod", (64, 32), 8, 64),
    "ModSacStepper-saturating": C.Case("mod", (128, 64), 4, 100, regime="B"),
}


@pytest.mark.parametrize("name", list(PINNED))
def test_step_gradients_reproduce_the_steppers_grad_fields(name):
    """run in fp32, step_gradients gives the .grad fields step() leaves behind on the same inputs: lr = 0 (nothing moves, as on the
    device), max_norm = 1e9 (clip_grad_norm_'s coefficient is clamped to exactly 1), to 1e-6 of each tensor's scale; objectives and td
    errors too.  The stepper itself is not touched by step_gradients."""
    case = PINNED[name]
    x = C.make_inputs(case)
    st = x.stepper
    nets = {"act": st.act, "cri": st.cri, "cri_target": st.cri_target}
    before = {(n, k): v.clone() for n, m in nets.items() for k, v in m.state_dict().items()}
    grads, info = C.references(case, x)[1]
    for n, m in nets.items():
        for k, v in m.state_dict().items():
            assert th.equal(v, before[n, k]), (n, k)
    assert all(p.grad is None for p in st.act.parameters()) and st.alpha_log.grad is None
    if C.is_mod(case):
        oc, oa = st.step(x.batch, x.eps_next, x.eps_cur)
    else:
        oc, oa = st.step(x.batch, x.eps_next, x.eps_cur, is_weight=x.is_weight, cum_reward=x.cum_reward, lambda_fit_cum_r=case.lambda_fit)
        np.testing.assert_allclose(info["td_error"].numpy(), st.td_error.numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose([info["obj_critic"], info["obj_actor"]], [oc, oa], rtol=1e-6, atol=1e-7)
    left = {k: p.grad for m in (st.act, st.cri) for k, p in m.named_parameters()}
    left["alpha_log"] = st.alpha_log.grad
    assert set(left) == set(grads)
    for k, g in left.items():
        g = g.double().numpy()
        assert np.abs(grads[k].reshape(g.shape) - g).max() <= 1e-6 * np.abs(g).max(), k
    for k, v in st.cri_target.state_dict().items():              # the soft-updated target the actor's gradient was taken against
        np.testing.assert_allclose(info["target"][k].numpy(), v.numpy(), rtol=1e-6, atol=0)


def test_an_actor_that_is_not_updated_has_no_gradients():
    case = C.CASES["mod-128x64-actor-skipped"]
    (r64, i64), _ = C.references(case, C.make_inputs(case))
    assert list(C.groups_of(r64)) == ["critic", "alpha"] and np.isnan(i64["obj_actor"]) and np.isfinite(i64["obj_critic"])


# ---- the comparison has teeth ------------------------------------------------------------------------------------------------------------
TEETH = ["fused-64x128", "layered-three-hidden", "mod-128x64"]


def _standin(name):
    case = C.CASES[name]
    x = C.make_inputs(case)
    (r64, i64), (r32, _) = C.references(case, x)
    assert C.edge_distance(case, i64) > C.EDGE
    return case, x, r64, r32


@pytest.mark.parametrize("name", TEETH)
def test_comparison_passes_on_the_fp32_restatement(name):
    case, _, r64, r32 = _standin(name)
    C.compare(name, "A", r32, r64, r32)
    mn = C.clip_max_norm(r64)
    assert all(C.norm(r64, names) > mn for k, names in C.groups_of(r64).items() if k != "alpha")         # both blocks really clip
    C.compare(name + " clipped", "A", C.clipped(r32, mn), C.clipped(r64, mn), C.clipped(r32, mn))


@pytest.mark.parametrize("name", TEETH)
def test_comparison_catches_a_dropped_batch_row(name):
    """one batch row missing from the actor's first-layer weight gradient, as a ragged last tile that loses a row would leave it"""
    case, x, r64, r32 = _standin(name)
    first = next(k for k in r64 if k.endswith(".0.weight") and not k.startswith(("encoder_sa", "decoder_")))
    share = _first_layer_row_share(x.stepper, x, case, case.B - 1).double().numpy()
    assert np.abs(share).max() > 0
    mutated = dict(r32)
    mutated[first] = r32[first] - share
    with pytest.raises(AssertionError, match=first.replace(".", r"\.")):
        C.compare(name, "A", mutated, r64, r32)


def _first_layer_row_share(st, x, case, row):
    """(dL/dz1)[row] (x) state[row] of the actor objective, fp32: the actor's first layer applied as z1 = z1_detached_rows + the one row's
    live product, so that only that row reaches the weight's gradient"""
    from copy import deepcopy
    from oracle.sac_torch import ActorFixSAC
    act, tar, cri = deepcopy(st.act), deepcopy(st.cri_target), st.cri
    with th.no_grad():
        for t, c in zip(tar.parameters(), cri.parameters()):
            t.copy_(c * st.tau + t * (1.0 - st.tau))
    enc = act.encoder_s if isinstance(act, ActorFixSAC) else act.net_s
    lin = enc[0]
    mask = th.zeros(case.B, 1)
    mask[row] = 1.0
    state = x.batch[0]

    class OneRow(th.nn.Module):
        def forward(self, s):
            live = th.nn.functional.linear(s, lin.weight, lin.bias)
            return live * mask + live.detach() * (1.0 - mask)
    enc[0] = OneRow()
    action_pg, logprob = act.get_action_logprob(state, x.eps_cur)
    obj = (tar(state, action_pg).mean() - logprob * st.alpha_log.exp().detach()).mean()
    (-obj).backward()
    return lin.weight.grad.detach().clone()


@pytest.mark.parametrize("name", TEETH)
def test_comparison_catches_a_decoder_scaled_by_1_002(name):
    case, _, r64, r32 = _standin(name)
    last = f"decoder_q{case.E - 1:02}."
    mutated = {k: v * 1.002 if k.startswith(last) else v for k, v in r32.items()}
    with pytest.raises(AssertionError, match="decoder_q"):
        C.compare(name, "A", mutated, r64, r32)


@pytest.mark.parametrize("name", TEETH)
def test_comparison_catches_a_zeroed_head_bias(name):
    case, _, r64, r32 = _standin(name)
    heads = [k for k in r64 if k in ("net_a.0.bias", "decoder_a_avg.0.bias", "decoder_a_std.0.bias")]
    assert heads
    mutated = {k: np.zeros_like(v) if k in heads else v for k, v in r32.items()}
    with pytest.raises(AssertionError, match=heads[0].replace(".", r"\.")):
        C.compare(name, "A", mutated, r64, r32)


@pytest.mark.parametrize("name", TEETH)
def test_comparison_catches_a_clip_norm_without_the_last_tensor(name):
    case, _, r64, r32 = _standin(name)
    mn = C.clip_max_norm(r64)
    with pytest.raises(AssertionError):
        C.compare(name + " clipped", "A", C.clipped(r32, mn, skip_last_tensor=True), C.clipped(r64, mn), C.clipped(r32, mn))
