"""Shared by tests/test_sac_gradients_cpu.py and tests/test_sac_gradients_gpu.py: the cases (one per kernel form of the SAC step), their
inputs, the fp64 / fp32 references (oracle/sac_torch.py:step_gradients) and the comparison itself.

How a gradient is read without touching the library: every update entry takes betas, lr and max_norm, and the library's one Adam
(csrc/erl_common.h erl_adam_update) computes m1 = m1 * beta1 + (1 - beta1) * g.  From zero moments with betas = (0, 0.999), lr = 0 and
step = 1 the first moments ARE the clipped gradients (the raw ones with max_norm = 1e9), the second moments are (1 - beta2) g^2, the
parameters do not move and the target becomes tau * critic + (1 - tau) * target.

Regime A (well-conditioned): head weights times 3, log_std bias linspace(-1.5, 0, A); no pre-clamp log_std within 1e-4 of a clamp edge.
The project's gradient bound 1e-4 * scale + 1e-7 holds per named tensor, and the fp32 restatement has to stay within a tenth of it (the
inputs' condition, not a measurement of the kernel).
Regime B (saturating): log_std bias linspace(-18, 3, A): both clamp edges, log(1 - a^2 + 1e-6) at a -> +-1.  fp32 itself is up to ~1e-3 of
scale from fp64 there, so the device may be at most 8 x the fp32 restatement's own error per tensor, floor 1e-6 of scale (the factor of
tests/test_acrobot_env_gpu.py's self-calibrating regime)."""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch as th

GAMMA, TAU, BETAS = 0.97, 5e-3, (0.0, 0.999)
RAW = 1e9                          # max_norm of the call that reads raw gradients
EDGE = 1e-4                        # no pre-clamp log_std this close to a clamp edge


class Case(NamedTuple):
    entry: str                     # "sac": ops.sac_update, "mod": ops.sac_update_mod (AgentModSAC's fused step)
    hidden: Tuple[int, ...]
    E: int
    B: int
    S: int = 11
    A: int = 3
    regime: str = "A"
    seed: int = 0
    actor_target: bool = False     # "sac" only: a copy of the actor as actor_target keeps a fused-capable shape on the layered step
    lambda_fit: float = 0.0
    is_weight: bool = False
    fix: bool = False              # "sac" only: SacSpec(..., actor_variant=SAC_ACTOR_FIX) on the layered step
    alpha0: float = -1.0
    update_actor: bool = True


# Seeds: the first from 0 at which the case's own conditions hold (asserted in every run: log_std away from the clamp edges, at least one
# unmasked row, regime A's fp32 restatement within a tenth of the bound on every tensor) -- searched on the CPU, see seed_ok.
CASES: Dict[str, Case] = {
    # ---- the layered step (csrc/sac.hip sac_step_layered)
    "layered-one-hidden": Case("sac", (32,), 1, 37, S=5, A=1),
    "layered-three-hidden": Case("sac", (64, 48, 32), 2, 130, S=17, A=6),
    "layered-40x24-per-decoder": Case("sac", (40, 24), 2, 1030, S=5, A=2),                # above kBatchedRows = 1024
    "layered-40x24-batched": Case("sac", (40, 24), 2, 100, S=5, A=2),
    "layered-actor-target": Case("sac", (64, 48), 2, 100, actor_target=True),
    "layered-lambda-fit": Case("sac", (64, 48), 2, 100, lambda_fit=0.5),
    "layered-is-weight": Case("sac", (64, 48), 2, 96, is_weight=True, actor_target=True),
    "layered-actor-fix": Case("sac", (64, 48, 32), 2, 64, fix=True, actor_target=True),
    # ---- the fused step (csrc/sac_fused.hip), one case per width-class pair: E = 2, B = 100 is seven tiles with four rows in the last
    **{f"fused-{h0}x{h1}": Case("sac", (h0, h1), 2, 100) for h0, h1 in
       ((32, 48), (64, 128), (48, 256), (96, 64), (128, 112), (80, 256), (256, 32), (192, 128), (256, 256))},
    "fused-pair-unsplit-backward": Case("sac", (192, 256), 2, 64),
    "fused-actor-split-critic-unsplit": Case("sac", (256, 256), 8, 256),                  # 16 tiles x 8 x 4 > 256
    "fused-nothing-split": Case("sac", (256, 256), 1, 1040),                              # 65 tiles
    "fused-narrowest": Case("sac", (16, 16), 1, 16, seed=1),
    "fused-narrowest-one-row": Case("sac", (16, 16), 1, 1),
    "fused-S56-A8": Case("sac", (64, 32), 8, 17, S=56, A=8),
    "fused-is-weight": Case("sac", (128, 64), 4, 96, is_weight=True),
    "fused-alpha-1.9": Case("sac", (64, 48), 2, 100, alpha0=1.9),
    # ---- AgentModSAC's fused step
    "mod-256x256": Case("mod", (256, 256), 8, 64, seed=1),
    "mod-128x64": Case("mod", (128, 64), 4, 100),
    "mod-S56-A8": Case("mod", (64, 32), 8, 17, S=56, A=8),
    "mod-128x64-actor-skipped": Case("mod", (128, 64), 4, 100, update_actor=False),
    # ---- regime B
    "saturating-layered-actor-target": Case("sac", (64, 48), 2, 100, regime="B", actor_target=True),
    "saturating-fused-64x48": Case("sac", (64, 48), 2, 100, regime="B"),
    "saturating-fused-256x256": Case("sac", (256, 256), 4, 64, regime="B"),
    "saturating-mod-128x64": Case("mod", (128, 64), 4, 100, regime="B"),
}


def is_mod(case: Case) -> bool:
    return case.entry == "mod" or case.fix


class Inputs(NamedTuple):
    stepper: object
    batch: tuple
    eps_next: th.Tensor
    eps_cur: th.Tensor
    is_weight: Optional[th.Tensor]
    cum_reward: Optional[th.Tensor]


def make_inputs(case: Case, seed: Optional[int] = None) -> Inputs:
    """the stepper (fp32, as the device holds it) and one batch with injected noise; the global generator is left as it was"""
    from oracle.sac_torch import ModSacStepper, SacStepper
    S, A, E, B = case.S, case.A, case.E, case.B
    with th.random.fork_rng(devices=[]):
        th.manual_seed(case.seed if seed is None else seed)
        st = (ModSacStepper if is_mod(case) else SacStepper)(list(case.hidden), S, A, E, lr=0.0, gamma=GAMMA, tau=TAU, max_norm=RAW)
        lo, hi, gain = (-1.5, 0.0, 3.0) if case.regime == "A" else (-18.0, 3.0, 1.0)
        with th.no_grad():
            for p in st.cri_target.parameters():                    # target != critic
                p.add_(0.05 * th.randn_like(p))
            bias = th.linspace(lo, hi, A) if (A > 1 or case.regime == "A") else th.tensor([0.3])
            if is_mod(case):
                st.act.decoder_a_avg[0].weight.mul_(gain)
                st.act.decoder_a_std[0].weight.mul_(gain)
                st.act.decoder_a_std[0].bias.copy_(bias)
                st.act_target.load_state_dict(st.act.state_dict())
            else:
                st.act.net_a[0].weight.mul_(gain)
                st.act.net_a[0].bias[A:] = bias
            st.alpha_log[:] = case.alpha0
        batch = (th.randn(B, S), th.randn(B, A).tanh(), th.randn(B), (th.rand(B) > 0.1).float(), (th.rand(B) > 0.1).float(), th.randn(B, S))
        eps_next, eps_cur = th.randn(B, A), th.randn(B, A)
        w = th.rand(B) * 0.9 + 0.1 if case.is_weight else None
        cum = th.randn(B) if case.lambda_fit else None
    return Inputs(st, batch, eps_next, eps_cur, w, cum)


def references(case: Case, x: Inputs):
    """(grads, info) of oracle/sac_torch.py:step_gradients in fp64 and in fp32, gradients as float64 numpy arrays"""
    from oracle.sac_torch import step_gradients
    out = []
    for dtype in (th.float64, th.float32):
        grads, info = step_gradients(x.stepper, x.batch, x.eps_next, x.eps_cur, dtype=dtype, is_weight=x.is_weight, cum_reward=x.cum_reward,
                                     lambda_fit_cum_r=case.lambda_fit, update_actor=case.update_actor)
        out.append(({k: v.double().numpy() for k, v in grads.items()}, info))
    return out


def clamp_edges(case: Case) -> Tuple[float, float]:
    return (-20.0, 2.0) if is_mod(case) else (-16.0, 2.0)


def edge_distance(case: Case, info64) -> float:
    """how close the closest pre-clamp log_std (both actor passes, fp64) comes to a clamp edge"""
    ls = th.cat([info64["log_std"], info64["log_std_next"]]).double()
    return min(float((ls - e).abs().min()) for e in clamp_edges(case))


def bound(scale: float) -> float:
    """the project's gradient bound (tests/test_kernels_gpu.py::test_ppo_step_gradients), here per named tensor"""
    return 1e-4 * scale + 1e-7


def compare(label: str, regime: str, got: Dict[str, np.ndarray], ref64: Dict[str, np.ndarray], ref32: Dict[str, np.ndarray]):
    """`got` (the device's first moments, or a stand-in) against the fp64 reference, tensor by tensor.  Regime A: max|got - ref| <=
    1e-4 * max|ref over that tensor| + 1e-7, and the fp32 restatement within a tenth of that.  Regime B: at most 8 x the fp32
    restatement's error on the same tensor, floor 1e-6 of its scale.  Prints the worst tensor and returns (name, error / scale, fp32
    restatement's error / scale, error / allowed) of it; raises AssertionError with every tensor that misses."""
    assert set(got) == set(ref64) == set(ref32), (sorted(set(got) ^ set(ref64)), sorted(set(ref32) ^ set(ref64)))
    misses, worst, ratio = [], None, 0.0
    for name, r in ref64.items():
        g, r32 = np.asarray(got[name], np.float64).reshape(r.shape), ref32[name].reshape(r.shape)
        assert np.isfinite(g).all(), f"{label}: {name} is not finite"
        scale = float(np.abs(r).max())
        err, err32 = float(np.abs(g - r).max()), float(np.abs(r32 - r).max())
        if regime == "A":
            allowed = bound(scale)
            if err32 > 0.1 * allowed:
                misses.append(f"{name}: the fp32 restatement is {err32:.3e} from fp64, more than a tenth of the bound {allowed:.3e} "
                              f"(scale {scale:.3e}): these inputs are not well-conditioned")
        else:
            allowed = max(8.0 * err32, 1e-6 * scale)
            if err > 1e-6 * scale:
                ratio = max(ratio, err / max(err32, 1e-30))
        if err > allowed:
            misses.append(f"{name}: error {err:.3e} > allowed {allowed:.3e} (scale {scale:.3e}, fp32 restatement {err32:.3e})")
        row = (name, err / max(scale, 1e-30), err32 / max(scale, 1e-30), err / allowed)
        if worst is None or row[3] > worst[3]:
            worst = row
    print(f"{label} [regime {regime}]: worst tensor {worst[0]}: device error / scale {worst[1]:.3e}, fp32 restatement {worst[2]:.3e}, "
          f"error / allowed {worst[3]:.3f}" + (f"; largest device / fp32 ratio over the tensors above the floor {ratio:.2f}" if regime == "B" else ""))
    assert not misses, f"{label}:\n  " + "\n  ".join(misses)
    return worst


def groups_of(grads: Dict[str, np.ndarray]) -> Dict[str, list]:
    """the three optimisers' tensors, in flat order: critic, actor (if it was updated), temperature"""
    critic = [k for k in grads if k.startswith(("encoder_sa.", "decoder_q"))]
    actor = [k for k in grads if k != "alpha_log" and k not in critic]
    return {k: v for k, v in (("critic", critic), ("actor", actor), ("alpha", ["alpha_log"])) if v}


def norm(grads: Dict[str, np.ndarray], names) -> float:
    return math.sqrt(sum(float((grads[k].astype(np.float64) ** 2).sum()) for k in names))


def clip_max_norm(ref64: Dict[str, np.ndarray]) -> float:
    """one max_norm for the clipped call: a quarter of the smaller of the actor's and the critic's fp64 norms, as the fp32 value the entry
    receives"""
    g = groups_of(ref64)
    return float(np.float32(0.25 * min(norm(ref64, g[k]) for k in ("critic", "actor") if k in g)))


def clipped(grads: Dict[str, np.ndarray], max_norm: float, skip_last_tensor: bool = False) -> Dict[str, np.ndarray]:
    """clip_grad_norm_ per optimiser: g * min(1, max_norm / (||g|| + 1e-6)).  skip_last_tensor: the mutation of
    tests/test_sac_gradients_cpu.py -- a norm that misses the block's last tensor."""
    out = {}
    for names in groups_of(grads).values():
        total = norm(grads, names[:-1] if skip_last_tensor and len(names) > 1 else names)
        coef = min(1.0, max_norm / (total + 1e-6))
        out.update({k: grads[k] * coef for k in names})
    return out


def seed_ok(case: Case, seed: int, margin: float = 0.5) -> bool:
    """the conditions a case's seed has to meet (searched once on the CPU with half the allowance, so that another machine's fp32
    summation order does not break them; every run asserts them again at the full allowance)"""
    x = make_inputs(case, seed)
    (r64, i64), (r32, _) = references(case, x)
    if edge_distance(case, i64) <= EDGE / margin or float(x.batch[4].sum()) < 1 or float(x.batch[3].sum()) < 1:
        return False
    if case.regime == "A":
        for variant in ((r64, r32), (clipped(r64, clip_max_norm(r64)), clipped(r32, clip_max_norm(r64)))):
            for k, r in variant[0].items():
                if np.abs(variant[1][k] - r).max() > margin * 0.1 * bound(np.abs(r).max()):
                    return False
    return True
