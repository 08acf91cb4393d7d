"""The actor-only code of the split-arithmetic PPO minibatch kernel (csrc/ppo_step_s3_impl.h, the ACTOR branch of ppo_block_s3: the 8-row
output layer with its A operands broadcast by the MFMA, exp(-2 std_log) and the logged entropy's terms formed ahead of their use, the
objective, dY / dstd, dW3 / db3) at the instantiation the benchmark runs -- S = 64, net [128, 128] -- and the smallest batches where that
code can go wrong: head rows below, across and at the 8-row pad (A = 1, 3, 8), one full workgroup (B = 128) and a ragged second one (B =
200: its 56 padding samples must add nothing to dW3, db3, dstd or the logged sums), all three objective forms, ~10 % of the samples masked.

The fp64 restatement, the inputs and the tolerance are those of tests/test_kernels_gpu.py::test_ppo_step_split_arith: the split kernel's
distance to fp64 may not exceed twice the fp32-MFMA kernel's on the same inputs, floor 1e-6 of the gradient's scale."""
import functools

import numpy as np
import pytest
import torch as th

from tests.test_kernels_gpu import cu, flat_params, oracle_flat_grads, ppo_case, random_net

pytestmark = pytest.mark.gpu

S, H1, H2 = 64, 128, 128
H, N = 9, 50
CLIP, LAM_ENT = 0.25, 0.001
OBJECTIVES = {"reference": 0, "canonical": 1, "a2c": 2}


@pytest.fixture(scope="module")
def ops():
    from elegantrl_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def dev():
    return th.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(A, B, objective):
    """inputs and the fp64 restatement of one (A, B, objective), built once and shared by the tests below (nobody writes to them)"""
    rng = np.random.default_rng(1000 * A + B + len(objective))
    buf_ids = ppo_case(rng, H, N, S, A, B)
    buf, ids = list(buf_ids[:6]), buf_ids[6]
    buf[3] = (buf[3] + 0.5 * rng.standard_normal(buf[3].shape)).astype(np.float32)      # ratios on both sides of the clip
    assert not buf[2][ids % H, ids // H].all(), "the case needs masked samples"      # (ids -> (t, n) = (ids % H, ids // H): AgentPPO.py:179-187)
    actor, critic = random_net(rng, S, H1, H2, A, True), random_net(rng, S, H1, H2, 1, False)
    ga, gc, objs = oracle_flat_grads(buf, ids, actor, critic, CLIP, LAM_ENT, np.float64, objective)
    return tuple(buf), ids, actor, critic, ga, gc, objs


def run_step(ops, dev, A, B, objective, arith):
    buf, ids, actor, critic = case(A, B, objective)[:4]
    n_slabs, stride = ops.ppo_num_slabs(B), ops.ppo_slab_stride(S, H1, H2, A)
    prev = ops.ppo_set_arith(arith)
    try:
        assert ops.ppo_arith_in_use(S, H1, H2, A) == arith
        slabs = th.full((n_slabs, stride), float("nan"), device=dev)
        ops.ppo_step(cu(flat_params(actor), dev), cu(flat_params(critic), dev), cu(actor.state_avg, dev), cu(actor.state_std, dev),
                     cu(critic.state_avg, dev), cu(critic.state_std, dev), S, H1, H2, A, *[cu(x, dev) for x in buf], cu(ids, dev),
                     CLIP, LAM_ENT, 1.0 / B, slabs, n_slabs, objective=OBJECTIVES[objective])
        th.cuda.synchronize()
    finally:
        ops.ppo_set_arith(prev)
    return slabs


@pytest.mark.parametrize("objective", list(OBJECTIVES))
@pytest.mark.parametrize("B", [128, 200])
@pytest.mark.parametrize("A", [1, 3, 8])
def test_actor_slab_sum_and_logged_sums_against_fp64(ops, dev, A, B, objective):
    """dW1..dW3, db1..db3, dstd of the actor (the slab sum) and the three logged sums against fp64, next to the fp32-MFMA kernel"""
    ga, gc, objs = case(A, B, objective)[4:]
    Pa, Pc = ops.MlpSpec(S, H1, H2, A, True).count, ops.MlpSpec(S, H1, H2, 1, False).count
    n_slabs, stride = ops.ppo_num_slabs(B), ops.ppo_slab_stride(S, H1, H2, A)
    errs = {}
    for arith in ("f32", "split"):
        slabs = run_step(ops, dev, A, B, objective, arith)
        flat = th.zeros(stride, device=dev)
        ops.grad_reduce(slabs, n_slabs, stride, flat)
        got = flat.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), f"{arith}: a slab slot was left unwritten"
        assert not np.any(got[Pa + Pc + 4:])
        errs[arith] = [np.abs(got[:Pa] - ga).max() / max(1e-30, np.abs(ga).max()),
                       np.abs(got[Pa + Pc:Pa + Pc + 3] - objs).max() / max(1e-30, np.abs(objs).max()),
                       np.abs(got[Pa:Pa + Pc] - gc).max() / max(1e-30, np.abs(gc).max())]
    print(f"A={A} B={B} {objective}: max error / scale vs fp64 (actor grad, logged sums, critic grad): f32 MFMA {errs['f32']}, split bf16 {errs['split']}")
    for name, e32, es in zip(("actor grad", "logged sums", "critic grad"), errs["f32"], errs["split"]):
        assert es <= max(2.0 * e32, 1e-6), f"{name}: split arithmetic error {es:.3e} against the fp32 kernel's {e32:.3e}"


@pytest.mark.parametrize("objective", list(OBJECTIVES))
@pytest.mark.parametrize("A", [1, 3, 8])
def test_two_calls_give_the_same_bits(ops, dev, A, objective):
    a = run_step(ops, dev, A, 200, objective, "split").cpu().numpy()
    b = run_step(ops, dev, A, 200, objective, "split").cpu().numpy()
    assert np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("A", [1, 3, 8])
def test_workgroup_maps_give_the_same_actor_slabs(ops, dev, A, monkeypatch):
    """which workgroup computes a slab must not show in it: maps 0, 1, 2 (csrc/ppo_step.h k6_wg_map) at a ragged two-slab batch"""
    Pa = ops.MlpSpec(S, H1, H2, A, True).count
    got = {}
    for wg_map in ("0", "1", "2"):
        monkeypatch.setenv("ERL_K6_WG_MAP", wg_map)               # read per launch
        got[wg_map] = run_step(ops, dev, A, 200, "reference", "split").cpu().numpy()
        assert np.isfinite(got[wg_map]).all(), f"map {wg_map}: a slab slot was left unwritten"
    for wg_map in ("1", "2"):
        assert np.array_equal(got["0"][:, :Pa].view(np.uint32), got[wg_map][:, :Pa].view(np.uint32)), f"actor slabs of map {wg_map} differ from map 0's"
        assert np.array_equal(got["0"].view(np.uint32), got[wg_map].view(np.uint32))
