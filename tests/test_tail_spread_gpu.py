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
The bf16 weight images are library-owned and exist only inside the update loop; their refresh is held bit for bit by the update-loop tests
(tests/test_kernels_gpu.py, tests/test_agent_gpu.py: the loop against the Python loop of its steps, which rebuilds the images from fp32)."""
import numpy as np
import pytest
import torch as th

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


def butterfly(v):
    """the xor-butterfly of wave_sum over the last axis (64 lanes): every lane ends with the same sum; lane 0's is returned"""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ off]
    return v[..., 0]


def host_partials(grad, stride, groups, scale):
    """the table erl_grad_sq_partials_f32 leaves: [chunk][group] fp64"""
    nblk = (stride + 63) // 64
    g = np.zeros(nblk * 64, np.float32)
    g[:stride] = grad
    xs = (g * np.float32(scale)).astype(np.float64)
    sq = xs * xs
    idx = np.arange(nblk * 64)
    out = np.zeros((nblk, len(groups)))
    for gi, (off, ln) in enumerate(groups):
        out[:, gi] = butterfly(np.where((idx >= off) & (idx < off + ln), sq, 0.0).reshape(nblk, 64))
    return out


def host_norm(col):
    """one group's column of the table summed as the kernel does: thread T over T + 1024 j, a butterfly per wave, the 16 waves in order"""
    nblk = len(col)
    pad = np.zeros((nblk + 1023) // 1024 * 1024)
    pad[:nblk] = col
    acc = np.zeros(1024)
    for row in pad.reshape(-1, 1024):
        acc = acc + row
    waves = butterfly(acc.reshape(16, 64))
    t = np.float64(0.0)
    for w in range(16):
        t = t + waves[w]
    return t


def host_clip_adam(p, g, m1, m2, groups, partials, step, max_norm, scale):
    """tail_adam_apply / erl_adam_update in numpy float32, one rounding per operation"""
    f = np.float32
    b1, b2 = f(BETA1), f(BETA2)
    bc1 = 1.0 - float(b1) ** step
    bc2 = 1.0 - float(b2) ** step
    step_size, bc2_sqrt = f(float(f(LR)) / bc1), f(np.sqrt(bc2))       # (the entry takes lr as a float)
    norms = []
    for gi, (off, ln) in enumerate(groups):
        total_norm = f(np.sqrt(host_norm(partials[:, gi])))
        norms.append(total_norm)
        coef = f(max_norm) / (total_norm + f(1e-6))
        coef = f(1.0) if coef > f(1.0) else coef
        s = slice(off, off + ln)
        gx = g[s] * (f(scale) * coef)
        a = m1[s] * b1 + (f(1.0) - b1) * gx
        b = m2[s] * b2 + (f(1.0) - b2) * (gx * gx)
        denom = np.sqrt(b) / bc2_sqrt + f(EPS)
        p[s] = p[s] - step_size * (a / denom)
        m1[s], m2[s] = a, b
    return norms


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
