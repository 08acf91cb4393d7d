"""tests/td3_ref.py (fp64, CPU) replays tests/golden/td3_small.npz -- a run of the reference's own AgentTD3 recorded by
tools/record_td3_golden.py with every draw logged -- within the bounds tests/test_sac.py applies to sac_small.npz for the same
quantities (objectives rtol 1e-5 / atol 1e-7, weights atol 2e-6, rollout actions rtol 1e-5 / atol 1e-6); the two nan slots are exact.
With E = 1 and no policy noise the same restatement is the DDPG oracle under D1: checked against the per-sample
formula written out in numpy."""
import math

import numpy as np
import torch as th

from tests.helpers import load
from tests.td3_ref import Td3Ref, gather


def _setup(g, dtype=th.float64):
    N, S, A, rows, B, n_upd, E, freq, h1, h2 = [int(x) for x in g["dims"]]
    gamma, lr, max_norm, reward_scale, tau, policy_noise, explore_noise = [float(x) for x in g["hyper"]]
    ref = Td3Ref([h1, h2], S, A, E, lr=lr, gamma=gamma, tau=tau, max_norm=max_norm, policy_noise_std=policy_noise, dtype=dtype)
    ref.load({k[5:]: v for k, v in g.items() if k.startswith("act0.")}, {k[5:]: v for k, v in g.items() if k.startswith("cri0.")})
    return ref, (N, S, A, rows, B, n_upd, E, freq), explore_noise


def test_restatement_replays_the_reference_rollout():
    g = load("td3_small.npz")
    ref, (N, S, A, rows, *_), explore_noise = _setup(g)
    with th.no_grad():
        for t in (0, 1, rows - 1):
            a = ref.policy(th.from_numpy(g["ro_states"][t]), explore_noise, th.from_numpy(g["ro_eps"][t]))
            np.testing.assert_allclose(a.numpy(), g["ro_actions"][t], rtol=1e-5, atol=1e-6)
    assert g["ro_actions"].min() >= -1.0 and g["ro_actions"].max() <= 1.0


def test_restatement_replays_the_reference_updates():
    g = load("td3_small.npz")
    ref, (N, S, A, rows, B, n_upd, E, freq), _ = _setup(g)
    assert (n_upd, freq, E) == (4, 2, 8)
    ring = {k: g[f"ro_{k}"] for k in ("states", "actions", "rewards", "undones", "unmasks")}
    for t in range(n_upd):
        batch, _ = gather(ring, g["ids"][t], rows - 1)
        upd = t % freq == 0
        oc, oa, td = ref.step(batch, g["noise"][t], upd)
        assert td.shape == (B,)
        np.testing.assert_allclose(oc, g["objs"][t][0], rtol=1e-5, atol=1e-7)
        if upd:
            np.testing.assert_allclose(oa, g["objs"][t][1], rtol=1e-5, atol=1e-7)
        else:                                                              # the two nan slots are exact
            assert math.isnan(oa) and math.isnan(g["objs"][t][1])
        for prefix, net in ((f"act{t + 1}", ref.act), (f"actt{t + 1}", ref.act_target), (f"cri{t + 1}", ref.cri), (f"crit{t + 1}", ref.cri_target)):
            for k, v in net.state_dict().items():
                np.testing.assert_allclose(v.numpy(), g[f"{prefix}.{k}"], rtol=0, atol=2e-6, err_msg=f"{prefix}.{k}")
        if not upd:                                                        # a skipped step leaves the actor and its target where they were
            for k in ref.act.state_dict():
                np.testing.assert_array_equal(g[f"act{t + 1}.{k}"], g[f"act{t}.{k}"])
                np.testing.assert_array_equal(g[f"actt{t + 1}.{k}"], g[f"actt{t}.{k}" if t else f"act0.{k}"])


def _gelu(x):
    return 0.5 * x * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))


def _mlp(sd, x):
    n = len(sd) // 2
    for i in range(n):
        x = x @ sd[f"net.{2 * i}.weight"].T + sd[f"net.{2 * i}.bias"]
        if i + 1 < n:
            x = _gelu(x)
    return x


def test_restatement_with_one_head_is_the_per_sample_ddpg_objective():
    """D1: criterion(q_i, label_i) * unmask_i, one label per sample; the first step's objectives from numpy alone"""
    rng = np.random.default_rng(7)
    S, A, B, gamma = 5, 2, 37, 0.97
    ref = Td3Ref([16, 8], S, A, 1, lr=1e-3, gamma=gamma, tau=5e-3, max_norm=3.0, policy_noise_std=0.0, seed=3)
    f = lambda net: {k: v.numpy().copy() for k, v in net.state_dict().items()}  # noqa: E731
    act, cri = f(ref.act), f(ref.cri)
    state, nxt, action = rng.standard_normal((B, S)), rng.standard_normal((B, S)), rng.uniform(-1, 1, (B, A))
    reward, undone, unmask = rng.standard_normal(B), (rng.random(B) > 0.2) * 1.0, (rng.random(B) > 0.2) * 1.0
    label = reward + undone * gamma * _mlp(cri, np.concatenate([nxt, np.tanh(_mlp(act, nxt))], 1))[:, 0]
    q = _mlp(cri, np.concatenate([state, action], 1))[:, 0]
    td_np = (q - label) ** 2 * unmask
    assert 0 < unmask.sum() < B
    oc, oa, td = ref.step((state, action, reward, undone, unmask, nxt), None, True)
    np.testing.assert_allclose(td.numpy(), td_np, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(oc, td_np.mean(), rtol=1e-12)
    assert td.shape == (B,) and math.isfinite(oa)
    # the actor objective is evaluated on the critic AFTER its step
    cri1 = f(ref.cri)
    assert any(np.abs(cri1[k] - cri[k]).max() > 0 for k in cri)
    np.testing.assert_allclose(oa, _mlp(cri1, np.concatenate([state, np.tanh(_mlp(act, state))], 1)).mean(), rtol=1e-12)
