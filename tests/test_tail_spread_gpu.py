"""The second launch of the optimiser tail (csrc/grad_tail.hip, clip_adam_partials_kernel) called directly on synthetic gradients through
the library-owned partial-norm table: erl_grad_sq_partials_f32 writes the table, erl_clip_adam_partials_f32 sums it, clips and steps.

What is pinned is the ASSOCIATION of the norm.  The table holds one fp64 value per 64-element chunk and parameter group (the xor-butterfly
32, 16, 8, 4, 2, 1 over the chunk's squares).  The kernel's thread T adds partials[T + 1024 j] in increasing j, every wave of 64 threads takes
the same butterfly, and the 16 wave results are added in wave order.  `host_norm` restates that in numpy float64; the kernel's norm is not
exported, so it is observed through everything that depends on it: the clip coefficient and with it both moments and the parameters,
restated in numpy float32 with every product and sum rounded separately (erl_adam_update) and compared BIT FOR BIT.  The second reference is a
route that shares no summation code with the kernel: the single-launch tail (tail_fused_kernel), which keeps the 1024-thread block sum.

Rows: 192 floats (3 chunks: less than a wave, the group seam inside chunk 1, no remainder behind the groups), 4 160 (65 chunks: a second
wave with one lane), 70 016 (1 094 chunks: the `+ 1024 j` accumulation), config 4's own row (25 872 + 24 961 parameters + 4 logged sums,
padded to whole lines) and a 51 756 + 4 float row.  Each with the clip active and inactive, two steps (so the moments are not zero).
SHAPE_CASES (further down) are the group shapes beside "two contiguous groups from 0": 1, 3 and 4 groups, gaps, an empty group, groups
shorter than a chunk and several seams in one chunk, other betas / eps / step -- the same assertions, plus gaps and padding bit-unchanged.
The restatements live in tests/adam_ref.py (checked on the CPU by tests/test_adam_ref_cpu.py).
The bf16 weight images are library-owned and exist only inside the update loop; their refresh is held bit for bit by the update-loop tests
(tests/test_kernels_gpu.py, tests/test_agent_gpu.py: the loop against the Python loop of its steps, which rebuilds the images from fp32)."""
import numpy as np
import pytest
import torch as th

from tests.adam_ref import host_clip_adam, host_norm, host_partials, outside_mask

pytestmark = pytest.mark.gpu
DEV = th.device("cuda:0")
LR, BETA1, BETA2, EPS = 1e-3, 0.9, 0.999, 1e-8

# (stride, groups)
CASES = {
    "192_seam_no_remainder": (192, [(0, 100), (100, 92)]),
    "4160_second_wave": (4160, [(0, 2077), (2077, 2083)]),
    "70016_strided_sum": (70016, [(0, 35001), (35001, 35011)]),
    "c4_row": ((25872 + 24961 + 4 + 31) // 32 * 32, [(0, 25872), (25872, 24961)]),
    "51756_plus_4": ((51756 + 4 + 31) // 32 * 32, [(0, 25880), (25880, 25876)]),
}


@pytest.fixture(scope="module")
def ops():
    from elegantrl_amd import ops as _ops
    return _ops


def bits(x):
    return x.detach().cpu().numpy().view(np.uint32) if isinstance(x, th.Tensor) else np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("clip", ["clip_active", "clip_inactive"])
@pytest.mark.parametrize("case", list(CASES))
def test_clip_adam_partials_keeps_the_norm_association(ops, case, clip):
    stride, groups = CASES[case]
    n_par = groups[-1][0] + groups[-1][1]
    scale = 0.5
    rng = np.random.default_rng(stride)
    p_h = rng.standard_normal(n_par).astype(np.float32)
    m1_h, m2_h = np.zeros(n_par, np.float32), np.zeros(n_par, np.float32)
    pa, ma, va = th.from_numpy(p_h.copy()).to(DEV), th.zeros(n_par, device=DEV), th.zeros(n_par, device=DEV)
    pb, mb, vb = pa.clone(), ma.clone(), va.clone()
    assert ops.tail_fused_ok(stride)
    for step in (1, 2):
        # magnitudes spread over eight binades: the order of the additions shows in the last bits of the fp64 sum
        g_h = (rng.standard_normal(stride) * np.exp2(rng.integers(-4, 4, stride))).astype(np.float32)
        partials = host_partials(g_h, stride, groups, scale)
        norm_min = min(float(np.sqrt(host_norm(partials[:, gi]))) for gi in range(len(groups)))
        max_norm = norm_min * 0.37 if clip == "clip_active" else 1e9
        norms = host_clip_adam(p_h, g_h, m1_h, m2_h, groups, partials, step, max_norm, scale)
        assert all(((max_norm / (float(n) + 1e-6)) < 1.0) == (clip == "clip_active") for n in norms)
        ga = th.from_numpy(g_h).to(DEV)
        ops.grad_sq_partials(ga, stride, groups, grad_scale=scale)
        ops.clip_adam_partials(pa, ga, ma, va, stride, groups, step, LR, max_norm, grad_scale=scale, betas=(BETA1, BETA2), eps=EPS)
        fb = th.empty(stride, device=DEV)
        ops.reduce_clip_adam_fused(ga.view(1, stride), 1, stride, fb, pb, mb, vb, groups, step, LR, max_norm, grad_scale=scale)
        assert th.equal(fb, ga)
        for name, dev_x, ref_x, host_x in (("exp_avg", ma, mb, m1_h), ("exp_avg_sq", va, vb, m2_h), ("params", pa, pb, p_h)):
            d, r, h = bits(dev_x), bits(ref_x), bits(host_x)
            print(f"{case} {clip} step {step} {name}: differs from the host restatement in {int((d != h).sum())}, "
                  f"from the single-launch tail in {int((d != r).sum())} of {n_par}")
            assert np.array_equal(d, h), f"{name}, step {step}: not the host restatement's bits"
            assert np.array_equal(d, r), f"{name}, step {step}: not the 1024-thread block sum's bits"
    th.cuda.synchronize()
    from elegantrl_amd import _hip
    _hip.check_async_faults()


# ---- group shapes the tail had never seen: one group, several seams in one chunk, gaps, a group that is exactly one chunk, one element,
# padding behind the last group, an empty group, a group that begins on a chunk's LAST element behind a gap (reduce_exchange_kernel's
# `touched` / `own` test decides per chunk between one butterfly and one per group).  (stride, groups, (betas, eps, first step))
DEFAULT_HYPER = ((BETA1, BETA2), EPS, 1)
SHAPE_CASES = {
    "192_one_group": (192, [(0, 192)], DEFAULT_HYPER),
    "192_three_groups_in_one_chunk": (192, [(0, 10), (10, 20), (30, 34)], DEFAULT_HYPER),
    "320_four_groups_with_gaps": (320, [(3, 50), (64, 64), (130, 1), (200, 100)], DEFAULT_HYPER),
    "4160_empty_group_and_start_on_a_chunks_last_element": (4160, [(63, 2014), (2077, 0), (2077, 2083)], DEFAULT_HYPER),
    "320_four_groups_b0.5_0.9_eps1e-3_step1000": (320, [(3, 50), (64, 64), (130, 1), (200, 100)], ((0.5, 0.9), 1e-3, 1000)),
}


def shape_case_state(stride, seed):
    """random parameters AND moments over the whole row (exp_avg_sq non-negative): gaps and padding must come back bit for bit"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(stride).astype(np.float32)
    m1 = (0.1 * rng.standard_normal(stride)).astype(np.float32)
    m2 = (0.01 * rng.standard_normal(stride) ** 2).astype(np.float32)
    return rng, p, m1, m2


@pytest.mark.parametrize("clip", ["clip_active", "clip_inactive"])
@pytest.mark.parametrize("case", list(SHAPE_CASES))
def test_clip_adam_partials_group_shapes(ops, case, clip):
    stride, groups, (betas, eps, step0) = SHAPE_CASES[case]
    scale = 0.5
    rng, p_h, m1_h, m2_h = shape_case_state(stride, stride + len(groups))
    p0, m10, m20 = p_h.copy(), m1_h.copy(), m2_h.copy()
    outside = outside_mask(stride, groups)
    pa, ma, va = (th.from_numpy(x.copy()).to(DEV) for x in (p_h, m1_h, m2_h))
    pb, mb, vb = pa.clone(), ma.clone(), va.clone()
    assert ops.tail_fused_ok(stride)
    for step in (step0, step0 + 1):
        g_h = (rng.standard_normal(stride) * np.exp2(rng.integers(-4, 4, stride))).astype(np.float32)
        partials = host_partials(g_h, stride, groups, scale)
        norm_min = min(float(np.sqrt(host_norm(partials[:, gi]))) for gi, (_, ln) in enumerate(groups) if ln)
        max_norm = norm_min * 0.37 if clip == "clip_active" else 1e9
        norms = host_clip_adam(p_h, g_h, m1_h, m2_h, groups, partials, step, max_norm, scale, LR, betas, eps)
        assert all(((max_norm / (float(n) + 1e-6)) < 1.0) == (clip == "clip_active") for n, (_, ln) in zip(norms, groups) if ln)
        ga = th.from_numpy(g_h).to(DEV)
        ops.grad_sq_partials(ga, stride, groups, grad_scale=scale)
        ops.clip_adam_partials(pa, ga, ma, va, stride, groups, step, LR, max_norm, grad_scale=scale, betas=betas, eps=eps)
        fb = th.empty(stride, device=DEV)
        ops.reduce_clip_adam_fused(ga.view(1, stride), 1, stride, fb, pb, mb, vb, groups, step, LR, max_norm, grad_scale=scale, betas=betas, eps=eps)
        assert th.equal(fb, ga)
        for name, dev_x, ref_x, host_x, x0 in (("exp_avg", ma, mb, m1_h, m10), ("exp_avg_sq", va, vb, m2_h, m20), ("params", pa, pb, p_h, p0)):
            d, r, h = bits(dev_x), bits(ref_x), bits(host_x)
            print(f"{case} {clip} step {step} {name}: differs from the host restatement in {int((d != h).sum())}, "
                  f"from the single-launch tail in {int((d != r).sum())} of {stride}; outside the groups {int((d != bits(x0))[outside].sum())} "
                  f"of {int(outside.sum())} changed")
            assert np.array_equal(d, h), f"{name}, step {step}: not the host restatement's bits"
            assert np.array_equal(d, r), f"{name}, step {step}: not the 1024-thread block sum's bits"
            assert np.array_equal(d[outside], bits(x0)[outside]), f"{name}, step {step}: a gap or the padding was written"
            assert np.array_equal(r[outside], bits(x0)[outside]), f"{name}, step {step}: the single-launch tail wrote a gap or the padding"
    th.cuda.synchronize()
    from elegantrl_amd import _hip
    _hip.check_async_faults()


@pytest.mark.parametrize("n_slabs", [1, 5])
def test_grad_reduce_partials_leaves_grad_sq_partials_table(ops, n_slabs):
    """the slab reduction's partial norms (reduce_exchange_kernel) against erl_grad_sq_partials_f32 on the summed row, at the 320 row with its
    four groups and gaps: the table is library-owned, so it is compared through what depends on it -- clip + Adam, bit for bit -- and both
    against the host restatement from the summed row"""
    stride, groups, (betas, eps, step0) = SHAPE_CASES["320_four_groups_with_gaps"]
    scale = 0.5
    rng, p_h, m1_h, m2_h = shape_case_state(stride, 7 + n_slabs)
    pa, ma, va = (th.from_numpy(x.copy()).to(DEV) for x in (p_h, m1_h, m2_h))
    pb, mb, vb = pa.clone(), ma.clone(), va.clone()
    for step in (step0, step0 + 1):
        slabs_h = (rng.standard_normal((n_slabs, stride)) * np.exp2(rng.integers(-4, 4, (n_slabs, stride)))).astype(np.float32)
        slabs = th.from_numpy(slabs_h).to(DEV)
        fa, fb = th.empty(stride, device=DEV), th.empty(stride, device=DEV)
        ops.grad_reduce_partials(slabs, n_slabs, stride, fa, groups, grad_scale=scale)
        g_h = fa.cpu().numpy()
        partials = host_partials(g_h, stride, groups, scale)
        max_norm = 0.37 * min(float(np.sqrt(host_norm(partials[:, gi]))) for gi in range(len(groups)))
        ops.clip_adam_partials(pa, fa, ma, va, stride, groups, step, LR, max_norm, grad_scale=scale, betas=betas, eps=eps)
        ops.grad_reduce(slabs, n_slabs, stride, fb)
        assert th.equal(fa, fb)
        ops.grad_sq_partials(fb, stride, groups, grad_scale=scale)
        ops.clip_adam_partials(pb, fb, mb, vb, stride, groups, step, LR, max_norm, grad_scale=scale, betas=betas, eps=eps)
        host_clip_adam(p_h, g_h, m1_h, m2_h, groups, partials, step, max_norm, scale, LR, betas, eps)
        for name, dev_x, ref_x, host_x in (("exp_avg", ma, mb, m1_h), ("exp_avg_sq", va, vb, m2_h), ("params", pa, pb, p_h)):
            d, r, h = bits(dev_x), bits(ref_x), bits(host_x)
            print(f"{n_slabs} slabs step {step} {name}: reduce-partials differs from sq-partials in {int((d != r).sum())}, "
                  f"from the host restatement in {int((d != h).sum())} of {stride}")
            assert np.array_equal(d, r), f"{name}, step {step}: the two partial-norm routes disagree"
            assert np.array_equal(d, h), f"{name}, step {step}: not the host restatement's bits"
    th.cuda.synchronize()
    from elegantrl_amd import _hip
    _hip.check_async_faults()
