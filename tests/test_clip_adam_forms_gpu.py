"""Every form of the clip + Adam kernels of csrc/optim.hip, called directly and compared BIT FOR BIT (params, exp_avg, exp_avg_sq, soft target)
with the float32 numpy restatement of tests/adam_ref.py (one rounding per operation, as erl_adam_update compiles; checked against torch and
fp64 on the CPU in tests/test_adam_ref_cpu.py):

  erl_clip_adam_f32            per-thread (clip_adam_kernel, one element per thread), grid-wait (clip_adam_grid_kernel) and loop (clip_adam_kernel's
                               per > 1024 loop); with a host step and with the step read from device memory (`step_base`: device pow).  Every
                               case ASSERTS the form erl_clip_adam_form reports -- the launcher's own branch -- so a case cannot silently run
                               another kernel than the one it is named after.
  erl_clip_adam_soft_f32       the same launch with the soft target update folded in.
  erl_clip_adam_parts_soft_f32 clip + Adam + soft update of one group from fp64 squared-norm pieces (clip_adam_parts_kernel).

Three consecutive steps from non-zero moments (random exp_avg, random non-negative exp_avg_sq).  Buffers carry 64 floats of padding in front of
and behind the groups (random values): gaps and padding must come back bit for bit in all three tensors.  The gradients' norms are rounding-
stable (adam_ref.norm_is_rounding_stable), so the three forms' different fp64 summation orders give one float32 norm and one restatement serves
all of them.  No case makes the grid wait time out; every test ends with a synchronise and the async-fault check."""
import numpy as np
import pytest
import torch as th

from tests import adam_ref as R

pytestmark = pytest.mark.gpu
DEV = th.device("cuda:0")
LR = 1e-3
FORM_NAMES = {0: "per-thread", 1: "grid-wait", 2: "loop"}
TENSORS = ("params", "exp_avg", "exp_avg_sq")


@pytest.fixture(scope="module")
def ops():
    from elegantrl_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def no_device_fault():
    yield
    th.cuda.synchronize()
    from elegantrl_amd import _hip
    _hip.check_async_faults()


def to_dev(x):
    return th.from_numpy(np.ascontiguousarray(x)).to(DEV)


def dbits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def assert_same_words(what, dev, host, nan_pattern=False):
    """bit equality, the number of differing words printed first; nan_pattern: NaNs must sit in the same places (their payload is the
    hardware's), every other word is compared bit for bit"""
    d, h = dbits(dev), R.bits(host)
    if nan_pattern:
        dn, hn = np.isnan(dev.detach().cpu().numpy()), np.isnan(host)
        assert np.array_equal(dn, hn), f"{what}: NaNs in other places than the restatement's"
        d, h = d[~dn], h[~hn]
    print(f"{what}: {int((d != h).sum())} of {d.size} words differ")
    assert np.array_equal(d, h), f"{what}: not the restatement's bits"


def run_f32_case(ops, name, case, call=None):
    """three steps of one case on the device (views behind the front padding, group offsets relative to them) and in the restatement (whole
    buffers), compared after every step; returns the device tensors"""
    inp = R.draw_f32_case(case)
    rel_groups, groups, total = case["groups"], inp["groups"], inp["total"]
    longest = max(ln for _, ln in rel_groups)
    form = ops.clip_adam_form(longest, len(rel_groups), case["route"] == "device")
    print(f"{name}: erl_clip_adam_form({longest}, {len(rel_groups)}, {case['route']} step) = {form} ({FORM_NAMES[form]}); seed {inp['seed']}")
    assert FORM_NAMES[form] == case["form"]
    host = [inp[k].copy() for k in ("p", "m1", "m2")]
    dev = [to_dev(inp[k]) for k in ("p", "m1", "m2")]
    outside = R.outside_mask(total, groups)
    step_base = th.tensor([case.get("step_base", 0)], dtype=th.int32, device=DEV) if case["route"] == "device" else None
    for k in range(R.N_STEPS):
        g, max_norm = inp["grads"][k], inp["max_norms"][k]
        offset = case["step"] + k
        step = offset + case.get("step_base", 0)
        R.clip_adam_f32_restated(host[0], g, host[1], host[2], groups, step, LR, case["betas"], case["eps"], max_norm, case["scale"])
        gd = to_dev(g)
        if call is None:
            ops.clip_adam(dev[0][R.PAD:], gd[R.PAD:], dev[1][R.PAD:], dev[2][R.PAD:], rel_groups, offset, LR, max_norm, grad_scale=case["scale"],
                          betas=case["betas"], eps=case["eps"], step_base=step_base)
        else:
            call(dev, gd, rel_groups, step, max_norm, k)
        for t, tname in enumerate(TENSORS):
            assert_same_words(f"{name} step {step} {tname}", dev[t], host[t], nan_pattern=case["grad"] == "inf")
            changed = int((dbits(dev[t]) != R.bits(inp[("p", "m1", "m2")[t]]))[outside].sum())
            assert changed == 0, f"{tname}: {changed} words outside the groups (gaps, padding) were written"
    return dev, inp


@pytest.mark.parametrize("name", list(R.F32_CASES))
def test_clip_adam_f32_form(ops, name):
    case = R.F32_CASES[name]
    dev, inp = run_f32_case(ops, name, case)
    if case["grad"] == "zero" and case["moments"] == "zero":
        assert np.array_equal(dbits(dev[0]), R.bits(inp["p"])), "a zero gradient from zero moments moved the parameters"
    if case["grad"] == "inf":
        assert int(th.isnan(dev[0]).sum()) == 1


def test_clip_adam_f32_loop_form_with_host_step(ops):
    """the loop form with a host step: the launch is too large to be resident at once.  Built from the query: the smallest four-group launch
    of equal lengths (whole workgroups + 1 element) for which erl_clip_adam_form answers 2."""
    limit = 64 * 1024 * 1024 // 4
    length = next((n for n in ((bx - 1) * 1024 + 1 for bx in range(65, limit // 1024 + 1)) if ops.clip_adam_form(n, 4, False) == ops.CLIP_ADAM_LOOP), None)
    if length is None:
        print("four groups of up to 16 Mi floats all stay in the grid-wait form on this device")
        pytest.skip("the loop form with a host step needs more than 64 Mi floats on this device")
    assert ops.clip_adam_form(length - 1024, 4, False) == ops.CLIP_ADAM_GRID_WAIT or length == 64 * 1024 + 1
    print(f"smallest loop-form launch with a host step: 4 groups x {length} = {length // 1024 + 1} workgroups each; "
          f"{(length - 1) // 1024} workgroups each still wait on the grid")
    run_f32_case(ops, f"loop_host_step_4x{length}", R.loop_host_case(length))


@pytest.mark.parametrize("name", [n for n in R.F32_CASES if "step_base" in n])
def test_device_step_equals_host_step(ops, name):
    """step_base (an int32 on the device) + offset against the host-step call at base + offset: bit for bit, i.e. the device's pow rounds
    the two bias corrections to the float32 the host's does"""
    case = R.F32_CASES[name]
    host_case = dict(case, route="host", form="per-thread" if case["groups"][0][1] <= 65536 else "grid-wait")
    inp = R.draw_f32_case(case)
    a = [to_dev(inp[k]) for k in ("p", "m1", "m2")]
    b = [to_dev(inp[k]) for k in ("p", "m1", "m2")]
    base = th.tensor([case["step_base"]], dtype=th.int32, device=DEV)
    n = case["groups"][0][1]
    assert FORM_NAMES[ops.clip_adam_form(n, 1, True)] == case["form"] and FORM_NAMES[ops.clip_adam_form(n, 1, False)] == host_case["form"]
    for k in range(R.N_STEPS):
        gd, offset = to_dev(inp["grads"][k]), case["step"] + k
        ops.clip_adam(a[0][R.PAD:], gd[R.PAD:], a[1][R.PAD:], a[2][R.PAD:], case["groups"], offset, LR, inp["max_norms"][k], grad_scale=case["scale"],
                      step_base=base)
        ops.clip_adam(b[0][R.PAD:], gd[R.PAD:], b[1][R.PAD:], b[2][R.PAD:], case["groups"], offset + case["step_base"], LR, inp["max_norms"][k],
                      grad_scale=case["scale"])
        for t, tname in enumerate(TENSORS):
            diff = int((dbits(a[t]) != dbits(b[t])).sum())
            print(f"{name} step {offset + case['step_base']} {tname}: device step differs from host step in {diff} of {a[t].numel()} words")
            assert diff == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the soft-update forms
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [5e-3, 1.0])
@pytest.mark.parametrize("n,form", [(1025, "per-thread"), (65537, "grid-wait")])
def test_clip_adam_soft(ops, n, form, tau):
    """the target is mixed with the parameter's NEW value (the restatement's order); tau = 1 makes it that value exactly"""
    case = R._case([(0, n)], form)
    inp = R.draw_f32_case(case)
    soft_h, soft_d = inp["soft"].copy(), to_dev(inp["soft"])
    outside = R.outside_mask(inp["total"], inp["groups"])
    host = [inp[k].copy() for k in ("p", "m1", "m2")]

    def call(dev, gd, rel_groups, step, max_norm, k):
        ops.clip_adam_soft(dev[0][R.PAD:], gd[R.PAD:], dev[1][R.PAD:], dev[2][R.PAD:], rel_groups, step, LR, max_norm, soft_d[R.PAD:], tau,
                           grad_scale=case["scale"])
        old = host[0].copy()
        R.clip_adam_f32_restated(host[0], inp["grads"][k], host[1], host[2], inp["groups"], step, LR, case["betas"], case["eps"], max_norm,
                                 case["scale"], soft=soft_h, tau=tau)
        assert_same_words(f"soft n={n} tau={tau} step {step} target", soft_d, soft_h)
        assert np.array_equal(dbits(soft_d)[outside], R.bits(inp["soft"])[outside]), "the target was written outside the group"
        if tau == 1.0:
            assert np.array_equal(dbits(soft_d)[~outside], R.bits(host[0])[~outside]) and not np.array_equal(host[0], old)

    run_f32_case(ops, f"soft n={n} tau={tau}", case, call)


@pytest.mark.parametrize("n,form", [(1025, "per-thread"), (65537, "grid-wait")])
def test_clip_adam_soft_without_a_target(ops, n, form):
    """soft = NULL: erl_clip_adam_f32's result, and a target that is not passed keeps its bits"""
    case = R._case([(0, n)], form)
    bystander = to_dev(R.draw_f32_case(case)["soft"])
    before = dbits(bystander).copy()

    def call(dev, gd, rel_groups, step, max_norm, k):
        ops.clip_adam_soft(dev[0][R.PAD:], gd[R.PAD:], dev[1][R.PAD:], dev[2][R.PAD:], rel_groups, step, LR, max_norm, None, 5e-3, grad_scale=case["scale"])

    run_f32_case(ops, f"soft=None n={n}", case, call)
    assert np.array_equal(dbits(bystander), before)


PARTS_PAD = 1024          # floats behind the group: a whole workgroup's worth, so that no thread of the last workgroup has an index outside


@pytest.mark.parametrize("nparts", [1, 7, 1024, 1025])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 70000])
def test_clip_adam_parts_soft(ops, n, nparts):
    """the pieces: host fp64 sums of squares over a split of the gradient into `nparts` runs (empty runs give 0.0); the kernel adds them as
    block_sum does -- thread T takes T + 1024 j, so with 1025 pieces thread 0 adds two -- which `host_norm` restates.  Steps alternate between
    an active and an inactive clip."""
    rng = np.random.default_rng(1000 * nparts + n)
    total = n + PARTS_PAD
    host = [rng.standard_normal(total).astype(np.float32), (0.1 * rng.standard_normal(total)).astype(np.float32),
            (0.01 * rng.standard_normal(total) ** 2).astype(np.float32), rng.standard_normal(total).astype(np.float32)]
    start = [x.copy() for x in host]
    dev = [to_dev(x) for x in host]
    tau, betas, eps = 5e-3, (0.9, 0.999), 1e-8
    cuts = np.sort(rng.integers(0, n + 1, nparts - 1))
    for k, step in enumerate((1, 2, 3)):
        g = (rng.standard_normal(total) * np.exp2(rng.integers(-4, 4, total))).astype(np.float32)
        pieces = np.array([np.sum(run.astype(np.float64) ** 2) for run in np.split(g[:n], cuts)])
        assert len(pieces) == nparts
        sq = R.host_norm(pieces)
        max_norm = float(np.sqrt(sq)) * (0.37 if k != 1 else 1e9)
        norms = R.clip_adam_f32_restated(host[0], g, host[1], host[2], [(0, n)], step, LR, betas, eps, max_norm, 1.0, soft=host[3], tau=tau, norm=[sq])
        assert (max_norm / (float(norms[0]) + 1e-6) < 1.0) == (k != 1)
        ops.clip_adam_parts_soft(dev[0], to_dev(g), dev[1], dev[2], n, to_dev(pieces), nparts, step, LR, max_norm, dev[3], tau, betas=betas, eps=eps)
        for t, tname in enumerate(TENSORS + ("target",)):
            assert_same_words(f"parts n={n} nparts={nparts} step {step} {tname}", dev[t], host[t])
            assert np.array_equal(dbits(dev[t])[n:], R.bits(start[t])[n:]), f"{tname}: the padding behind the group was written"
