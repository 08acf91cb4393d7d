"""Plain-numpy references of the library's clip + Adam kernels (no GPU, no torch), shared by tests/test_tail_spread_gpu.py,
tests/test_clip_adam_forms_gpu.py and tests/test_adam_ref_cpu.py.

Every optimiser kernel calls the one erl_adam_update (csrc/erl_common.h), compiled with contraction off: every product and sum is rounded to
float32 on its own.  numpy float32 arithmetic rounds the same way, so a restatement of the update, one rounding per operation, gives the
kernels' BITS -- provided the one quantity that is not elementwise, the group's gradient norm, rounds to the same float32:

  * the partial-norm tail (csrc/grad_tail.hip) and erl_clip_adam_parts_soft_f32 add fp64 values in an order that `host_partials` /
    `host_norm` restate exactly;
  * the three forms of erl_clip_adam_f32 (csrc/optim.hip) add the fp64 squares in three different orders.  Their sums differ from the exact
    sum by a few fp64 ulps (relative 1e-16 times at most log2 of the length), so float32(sqrt(.)) is the same for all of them whenever it is
    the same over the whole interval s (1 -+ 1e-12) around the exact sum s: `norm_is_rounding_stable`.  That is a condition on the inputs
    alone; `draw_f32_case` draws each case's gradients from a fixed seed and moves to the next seed until it holds.

`clip_adam_fp64` is the same update in float64: what the float32 restatement's own error is measured against."""
import math

import numpy as np

F = np.float32
PAD = 64            # floats of padding in front of the first and behind the last group of an erl_clip_adam_f32 case


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


def bias_corrections(step, lr, betas):
    """(step_size, bc2_sqrt) as the host side of every entry computes them: doubles from the float arguments, rounded to float32 once"""
    bc1 = 1.0 - float(F(betas[0])) ** step
    bc2 = 1.0 - float(F(betas[1])) ** step
    return F(float(F(lr)) / bc1), F(np.sqrt(bc2))


def adam_update_f32(p, gx, m1, m2, s, betas, eps, step_size, bc2_sqrt, soft=None, tau=0.0):
    """erl_adam_update (+ erl_soft_update) on the slice `s`, in place, numpy float32: one rounding per operation"""
    b1, b2 = F(betas[0]), F(betas[1])
    a = m1[s] * b1 + (F(1.0) - b1) * gx
    b = m2[s] * b2 + (F(1.0) - b2) * (gx * gx)
    denom = np.sqrt(b) / bc2_sqrt + F(eps)
    p[s] = p[s] - step_size * (a / denom)
    m1[s], m2[s] = a, b
    if soft is not None:
        soft[s] = p[s] * F(tau) + soft[s] * (F(1.0) - F(tau))       # the parameter's NEW value; products rounded separately


def clip_coef_f32(total_norm, max_norm):
    coef = F(max_norm) / (total_norm + F(1e-6))
    return F(1.0) if coef > F(1.0) else coef


def host_clip_adam(p, g, m1, m2, groups, partials, step, max_norm, scale, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """tail_adam_apply / erl_adam_update in numpy float32, one rounding per operation; the norm from the partial-norm table"""
    step_size, bc2_sqrt = bias_corrections(step, lr, betas)                # (the entry takes lr as a float)
    norms = []
    with np.errstate(all="ignore"):
        for gi, (off, ln) in enumerate(groups):
            total_norm = F(np.sqrt(host_norm(partials[:, gi])))
            norms.append(total_norm)
            s = slice(off, off + ln)
            gx = g[s] * (F(scale) * clip_coef_f32(total_norm, max_norm))
            adam_update_f32(p, gx, m1, m2, s, betas, eps, step_size, bc2_sqrt)
    return norms


def group_sq_sum(g, off, ln, scale):
    """the exact sum of the squares of float32(g * scale) over one group, rounded once to float64"""
    with np.errstate(all="ignore"):
        xs = (g[off:off + ln] * F(scale)).astype(np.float64)
        return math.fsum(xs * xs)


def norm_is_rounding_stable(sq_sum):
    """float32(sqrt(s)) is one value for every s within relative 1e-12 of `sq_sum`: any fp64 summation order gives that norm"""
    with np.errstate(all="ignore"):
        r = [F(np.sqrt(np.float64(sq_sum) * k)) for k in (1.0 - 1e-12, 1.0, 1.0 + 1e-12)]
    return bool(r[0] == r[1] == r[2]) or bool(np.isnan(r[1]) and np.isnan(r[0]) and np.isnan(r[2]))


def clip_adam_f32_restated(p, g, m1, m2, groups, step, lr, betas, eps, max_norm, grad_scale, soft=None, tau=0.0, norm="exact", bias=None):
    """erl_clip_adam_f32 / erl_clip_adam_soft_f32 / erl_clip_adam_parts_soft_f32 in numpy float32, in place; returns the groups' float32 norms.
    norm: "exact" (math.fsum over the fp64 squares of float32(g * scale)) or one fp64 squared sum per group (the parts form: `host_norm`
    of the pieces).  bias: (step_size, bc2_sqrt) instead of the host's own (the device-step form's error bound moves them by an ulp).
    Elements outside every group are not touched."""
    step_size, bc2_sqrt = bias_corrections(step, lr, betas) if bias is None else (F(bias[0]), F(bias[1]))
    norms = []
    with np.errstate(all="ignore"):
        for gi, (off, ln) in enumerate(groups):
            sq = group_sq_sum(g, off, ln, grad_scale) if isinstance(norm, str) else np.float64(norm[gi])
            total_norm = F(np.sqrt(np.float64(sq)))
            norms.append(total_norm)
            s = slice(off, off + ln)
            gx = g[s] * (F(grad_scale) * clip_coef_f32(total_norm, max_norm))
            adam_update_f32(p, gx, m1, m2, s, betas, eps, step_size, bc2_sqrt, soft, tau)
    return norms


def clip_adam_fp64(p, g, m1, m2, groups, step, lr, betas, eps, max_norm, grad_scale, soft=None, tau=0.0):
    """the same update entirely in float64 (float64 arrays, in place; the float32 hyper-parameters as the kernels receive them)"""
    d = lambda x: np.float64(F(x))          # noqa: E731
    b1, b2 = d(betas[0]), d(betas[1])
    step_size = d(lr) / (1.0 - float(b1) ** step)
    bc2_sqrt = np.sqrt(1.0 - float(b2) ** step)
    norms = []
    with np.errstate(all="ignore"):
        for off, ln in groups:
            s = slice(off, off + ln)
            xs = g[s].astype(np.float64) * d(grad_scale)
            total_norm = np.sqrt(math.fsum(xs * xs))
            norms.append(total_norm)
            coef = min(d(max_norm) / (total_norm + d(1e-6)), 1.0)
            gx = g[s].astype(np.float64) * (d(grad_scale) * coef)
            a = m1[s] * b1 + (1.0 - b1) * gx
            b = m2[s] * b2 + (1.0 - b2) * (gx * gx)
            p[s] = p[s] - step_size * (a / (np.sqrt(b) / bc2_sqrt + d(eps)))
            m1[s], m2[s] = a, b
            if soft is not None:
                soft[s] = p[s] * d(tau) + soft[s] * (1.0 - d(tau))
    return norms


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of erl_clip_adam_f32 (tests/test_clip_adam_forms_gpu.py runs them, tests/test_adam_ref_cpu.py checks their inputs).
# groups: (offset, length) relative to the first float behind the front padding; form: what erl_clip_adam_form must report
# ("per-thread", "grid-wait", "loop"); route: "host" (step passed by value) or "device" (step_base).
# ---------------------------------------------------------------------------------------------------------------------------------
HYPER_ROWS = {       # step = the first of the case's consecutive steps
    "step1_default": dict(step=1, betas=(0.9, 0.999), eps=1e-8, scale=1.0, clip=True),
    "step2_b0.5_0.9_eps1e-3_scale.125_noclip": dict(step=2, betas=(0.5, 0.9), eps=1e-3, scale=0.125, clip=False),
    "step1000_b0_0.999_scale.125": dict(step=1000, betas=(0.0, 0.999), eps=1e-8, scale=0.125, clip=True),
    "step100000_eps1e-3_noclip": dict(step=100000, betas=(0.9, 0.999), eps=1e-3, scale=1.0, clip=False),
    "step1000_b0.5_0.9": dict(step=1000, betas=(0.5, 0.9), eps=1e-8, scale=1.0, clip=True),
    "zero_grad_zero_moments": dict(step=1, betas=(0.9, 0.999), eps=1e-8, scale=1.0, clip=True, grad="zero", moments="zero"),
    "zero_grad": dict(step=3, betas=(0.9, 0.999), eps=1e-8, scale=1.0, clip=True, grad="zero"),
    "one_inf": dict(step=2, betas=(0.9, 0.999), eps=1e-8, scale=1.0, clip=True, grad="inf"),
}
BASE = dict(step=1, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, scale=0.5, clip=True, grad="random", moments="random", route="host")


def _case(groups, form, **kw):
    return dict(BASE, groups=list(groups), form=form, **kw)


F32_CASES = {}
for _n in (1, 63, 64, 65, 1023, 1024, 1025, 32768, 32769, 65536):
    F32_CASES[f"len{_n}_per-thread"] = _case([(0, _n)], "per-thread")
for _n in (65537, 70000):
    F32_CASES[f"len{_n}_grid-wait"] = _case([(0, _n)], "grid-wait")
for _n in (65537, 200000):
    F32_CASES[f"len{_n}_loop_device_step"] = _case([(0, _n)], "loop", route="device")
F32_CASES.update({
    "groups1": _case([(0, 700)], "per-thread"),
    "groups2_gap": _case([(0, 100), (130, 1000)], "per-thread"),
    "groups3_descending_gaps": _case([(3000, 500), (1200, 1500), (0, 1100)], "per-thread"),
    "groups4_one_empty": _case([(0, 300), (300, 0), (350, 1030), (1400, 5)], "per-thread"),
    "groups2_70000_and_5_grid-wait": _case([(0, 70000), (70010, 5)], "grid-wait"),
})
for _n, _form in ((1025, "per-thread"), (65537, "grid-wait")):
    for _name, _row in HYPER_ROWS.items():
        F32_CASES[f"len{_n}_{_name}"] = _case([(0, _n)], _form, **_row)
for _n, _form in ((1025, "per-thread"), (65537, "loop")):
    for _base in (0, 1, 999):
        F32_CASES[f"len{_n}_step_base{_base}"] = _case([(0, _n)], _form, route="device", step_base=_base, betas=(0.9, 0.999))
N_STEPS = 3


def loop_host_case(length):
    """the loop form with a host step: four equal groups of `length` (found through erl_clip_adam_form), 64 floats between them"""
    return _case([(k * (length + PAD), length) for k in range(4)], "loop")


def case_span(case):
    return max(off + ln for off, ln in case["groups"])


def draw_f32_case(case, seed0=2024, n_steps=N_STEPS):
    """the inputs of one case: params, both moments (exp_avg random, exp_avg_sq random and non-negative), a target, `n_steps` gradients and
    each step's max_norm -- whole buffers with PAD floats in front of and behind the groups' span, random there as well.  Gradients spread
    over eight binades.  The seed moves on (at most 8 times) until every group's norm of every step is rounding-stable."""
    span, groups = case_span(case), case["groups"]
    total = PAD + span + PAD
    shifted = [(PAD + off, ln) for off, ln in groups]
    for seed in range(seed0, seed0 + 8):
        rng = np.random.default_rng(seed)
        p = rng.standard_normal(total).astype(np.float32)
        soft = rng.standard_normal(total).astype(np.float32)
        m1 = (0.1 * rng.standard_normal(total)).astype(np.float32)
        m2 = (0.01 * rng.standard_normal(total) ** 2).astype(np.float32)
        if case["moments"] == "zero":
            m1[:], m2[:] = 0, 0
        grads, max_norms, sq_sums = [], [], []
        for _ in range(n_steps):
            g = (rng.standard_normal(total) * np.exp2(rng.integers(-4, 4, total))).astype(np.float32)
            if case["grad"] == "zero":
                for off, ln in shifted:
                    g[off:off + ln] = 0
            elif case["grad"] == "inf":
                off, ln = max(shifted, key=lambda x: x[1])
                g[off + ln // 3] = np.inf
            sq = [group_sq_sum(g, off, ln, case["scale"]) for off, ln in shifted]
            live = [float(np.sqrt(s)) for s, (_, ln) in zip(sq, shifted) if ln > 0]
            ref_norm = min(live)
            if case["grad"] != "random":
                max_norms.append(3.0)                 # (a zero or infinite norm has no multiple to clip at)
            else:
                max_norms.append(ref_norm * (0.37 if case["clip"] else 1e9))
            grads.append(g)
            sq_sums.extend(sq)
        if all(norm_is_rounding_stable(s) for s in sq_sums):
            return dict(seed=seed, total=total, groups=shifted, p=p, m1=m1, m2=m2, soft=soft, grads=grads, max_norms=max_norms, sq_sums=sq_sums)
    raise AssertionError("no rounding-stable gradient norm within 8 seeds")


def outside_mask(total, groups):
    """True where no group reaches: gaps and padding"""
    out = np.ones(total, bool)
    for off, ln in groups:
        out[off:off + ln] = False
    return out


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
