"""Every buffer the library keeps per (device, stream) (csrc/stream_slots.h), through the public ops only: for each route that has one, three
input sets of different sizes are computed alone on the current stream and then replayed interleaved on three streams for three rounds --
same bits (every route here repeats bit for bit), no device-side fault; and a buffer that grew serves a smaller request, then the large
one again, unchanged.  One module-wide pair of side streams: a (device, stream) entry is kept until the process exits, so no test here
makes streams of its own, and none tries to fill a table (tests/test_stream_slots_cpu.py does that on the host)."""
import numpy as np
import pytest
import torch as th

from tests.test_kernels_gpu import cu, flat_params, ppo_case, random_net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from elegantrl_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def dev():
    return th.device("cuda:0")


@pytest.fixture(scope="module")
def streams(dev):
    return [th.cuda.Stream(device=dev), th.cuda.Stream(device=dev), th.cuda.current_stream(dev)]


def interleaved(streams, sets, run):
    """run(set) -> tuple of tensors, from nothing but the set (it clones what it updates)"""
    from elegantrl_amd import _hip
    ref = [run(s) for s in sets]
    th.cuda.synchronize()
    outs = []
    for _ in range(3):
        for s, st in zip(sets, streams):
            with th.cuda.stream(st):
                outs.append(run(s))
    th.cuda.synchronize()
    for i, out in enumerate(outs):
        for j, (x, y) in enumerate(zip(out, ref[i % 3])):
            assert th.equal(x, y), f"round {i // 3}, set {i % 3}, output {j}: max difference {(x - y).abs().max().item():.3e}"
    _hip.check_async_faults()


def same(first, third):
    for j, (x, y) in enumerate(zip(first, third)):
        assert th.isfinite(x).all() and th.equal(x, y), f"output {j}"


# ---- the (256, h2) step: scratch per (device, stream), sized by the slab count --------------------------------------------------
def wide_set(dev, B, S=8, h2=64, A=2, H=9, N=50):
    rng = np.random.default_rng(100 + B)
    case = ppo_case(rng, H, N, S, A, B)
    actor, critic = random_net(rng, S, 256, h2, A, True), random_net(rng, S, 256, h2, 1, False)
    norm = [cu(actor.state_avg, dev), cu(actor.state_std, dev), cu(critic.state_avg, dev), cu(critic.state_std, dev)]
    return dict(S=S, h2=h2, A=A, B=B, P=cu(np.concatenate([flat_params(actor), flat_params(critic)]), dev), norm=norm,
                buf=[cu(x, dev) for x in case[:6]], ids=cu(case[6], dev))


def wide_run(ops, c):
    S, h2, A, B = c["S"], c["h2"], c["A"], c["B"]
    Pa = ops.MlpSpec(S, 256, h2, A, True).count
    n_slabs, stride = ops.ppo_num_slabs(B), ops.ppo_slab_stride(S, 256, h2, A)
    slabs = th.full((n_slabs, stride), float("nan"), device=c["P"].device)
    flat = th.zeros(stride, device=c["P"].device)
    ops.ppo_step(c["P"][:Pa], c["P"][Pa:], *c["norm"], S, 256, h2, A, *c["buf"], c["ids"], 0.25, 0.001, 1.0 / B, slabs, n_slabs)
    ops.grad_reduce(slabs, n_slabs, stride, flat)
    return (flat,)


# ---- the split-arithmetic update loop at [128, 128]: weight images and per-sample records per (device, stream) ---------------------
def loop_set(dev, H, N, S=3, A=1, B=128, T=3):
    rng = np.random.default_rng(H * N)
    buf = ppo_case(rng, H, N, S, A, B)[:6]
    actor, critic = random_net(rng, S, 128, 128, A, True), random_net(rng, S, 128, 128, 1, False)
    norm = [cu(actor.state_avg, dev), cu(actor.state_std, dev), cu(critic.state_avg, dev), cu(critic.state_std, dev)]
    return dict(S=S, A=A, B=B, T=T, P=cu(np.concatenate([flat_params(actor), flat_params(critic)]), dev), norm=norm,
                buf=[cu(x, dev) for x in buf], ids=cu(rng.integers(0, H * N, (T, B)), dev))


def loop_run(ops, c):
    S, A, B, T, P0 = c["S"], c["A"], c["B"], c["T"], c["P"]
    stride, n_slabs = ops.ppo_slab_stride(S, 128, 128, A), ops.ppo_num_slabs(B)
    P, M1, M2 = P0.clone(), th.zeros_like(P0), th.zeros_like(P0)
    slabs, rows = th.zeros((n_slabs, stride), device=P0.device), th.zeros((T, stride), device=P0.device)
    ops.ppo_update(P, M1, M2, *c["norm"], S, 128, 128, A, *c["buf"], c["ids"], 0.25, 0.001, slabs, rows, 1, 1e-3, 3.0)
    return P, M1, M2, rows


@pytest.fixture
def split_arith(ops):
    prev = ops.ppo_set_arith("split")
    yield
    ops.ppo_set_arith(prev)


# the two grow tests come first: they want entries that have not grown yet
def test_wide_scratch_grows_serves_less_and_grows_again(ops, dev, streams):
    """1 slab, 8 slabs, 1 slab on one stream: the third result is the first"""
    small, large = wide_set(dev, 1), wide_set(dev, 1024)
    th.cuda.synchronize()
    with th.cuda.stream(streams[0]):
        first, big, third = wide_run(ops, small), wide_run(ops, large), wide_run(ops, small)
        again = wide_run(ops, large)
    th.cuda.synchronize()
    same(first, third)
    same(big, again)


def test_update_loop_buffers_grow_serve_less_and_grow_again(ops, dev, streams, split_arith):
    """rollouts of 8 x 64, 16 x 128 and 8 x 64 rows on one stream (the per-sample records grow with the rollout): the third result is the first"""
    small, large = loop_set(dev, 8, 64), loop_set(dev, 16, 128)
    th.cuda.synchronize()
    with th.cuda.stream(streams[0]):
        first, big, third = loop_run(ops, small), loop_run(ops, large), loop_run(ops, small)
        again = loop_run(ops, large)
    th.cuda.synchronize()
    same(first, third)
    same(big, again)
    assert not th.equal(first[0], small["P"])


def test_wide_step_scratch_is_per_stream(ops, dev, streams):
    """ops.ppo_step at (S, h2, A) = (8, 64, 2) with 1, 2 and 8 slabs"""
    assert ops.ppo_arith_in_use(8, 256, 64, 2) == "split"
    interleaved(streams, [wide_set(dev, B) for B in (1, 200, 1024)], lambda c: wide_run(ops, c))


def test_wide3_step_buffers_are_per_stream(ops, dev, streams):
    """ops.mlpn_ppo_step at (S, h3, A) = (17, 64, 5), the row of tests/test_ppo_wide_gpu.py's WIDE3_SHAPES with the fewest parameters: images,
    slabs and scratch in one block per (device, stream), sized by the slab count"""
    from tests.test_mlpn_gpu import random_net_n
    S, h3, A, H, N = 17, 64, 5, 9, 50
    dims = [S, 256, 128, h3]
    spec = ops.MlpSpecN(dims + [A], True)
    count = spec.count + ops.MlpSpecN(dims + [1], False).count + 4

    def make(B):
        rng = np.random.default_rng(300 + B)
        case = ppo_case(rng, H, N, S, A, B)
        actor, critic = random_net_n(rng, dims + [A], True), random_net_n(rng, dims + [1], False)
        return [B, cu(flat_params(actor), dev), cu(flat_params(critic), dev), cu(actor.state_avg, dev), cu(actor.state_std, dev),
                cu(critic.state_avg, dev), cu(critic.state_std, dev)] + [cu(x, dev) for x in case]

    def run(c):
        flat = th.full((count,), float("nan"), device=dev)
        ops.mlpn_ppo_step(*c[1:7], spec, *c[7:], 0.25, 0.001, 1.0 / c[0], flat)
        return (flat,)

    interleaved(streams, [make(B) for B in (1, 200, 1024)], run)


def test_update_loop_images_and_records_are_per_stream(ops, dev, streams, split_arith):
    """ops.ppo_update at [128, 128] with rollouts of 8 x 64, 16 x 128 and 8 x 256 rows"""
    assert ops.ppo_arith_in_use(3, 128, 128, 1) == "split"
    interleaved(streams, [loop_set(dev, H, N) for H, N in ((8, 64), (16, 128), (8, 256))], lambda c: loop_run(ops, c))


# ---- the optimiser tails: partial-norm tables ----------------------------------------------------------------------------------
def tail_set(dev, n_slabs, Pa, Pc, steps=2):
    g = th.Generator(device=dev).manual_seed(n_slabs + Pa)
    stride = (Pa + Pc + 4 + 31) // 32 * 32
    slabs = [th.randn((n_slabs, stride), device=dev, generator=g) * (0.1 if k % 2 else 10.0) for k in range(steps)]
    return dict(n_slabs=n_slabs, stride=stride, groups=[(0, Pa), (Pa, Pc)], p0=th.randn(Pa + Pc, device=dev, generator=g), slabs=slabs)


def test_two_launch_tail_table_is_per_stream(ops, dev, streams):
    """ops.grad_reduce_partials writes the stream's table, ops.clip_adam_partials reads it"""
    def run(c):
        p, m, v = c["p0"].clone(), th.zeros_like(c["p0"]), th.zeros_like(c["p0"])
        f = th.empty(c["stride"], device=dev)
        for step, slabs in enumerate(c["slabs"], 1):
            ops.grad_reduce_partials(slabs, c["n_slabs"], c["stride"], f, c["groups"])
            ops.clip_adam_partials(p, f, m, v, c["stride"], c["groups"], step, 1e-3, 3.0)
        return f, p, m, v

    interleaved(streams, [tail_set(dev, 1, 300, 200), tail_set(dev, 7, 1000, 37), tail_set(dev, 37, 70000, 5)], run)


def test_single_launch_tail_tables_are_per_stream_and_row_length(ops, dev, streams):
    """ops.reduce_clip_adam_fused with two row lengths alternating on ONE stream, three steps each: the parity of every (stream, row length)
    table advances on its own (and by an odd count per replay, so a replay starts on the other half of the table)"""
    def run(pair):
        state = [(c, c["p0"].clone(), th.zeros_like(c["p0"]), th.zeros_like(c["p0"]), th.empty(c["stride"], device=dev)) for c in pair]
        for step in range(1, 4):
            for c, p, m, v, f in state:
                ops.reduce_clip_adam_fused(c["slabs"][step - 1], c["n_slabs"], c["stride"], f, p, m, v, c["groups"], step, 1e-3, 3.0)
        return tuple(t for _, p, m, v, f in state for t in (f, p, m, v))

    a, b, c, d = (tail_set(dev, 1, 300, 200, 3), tail_set(dev, 7, 1000, 37, 3), tail_set(dev, 3, 2000, 100, 3), tail_set(dev, 37, 70000, 5, 3))
    assert all(ops.tail_fused_ok(x["stride"]) for x in (a, b, c, d))
    interleaved(streams, [(a, b), (b, c), (d, a)], run)


# ---- the fused SAC step: exchange slots ----------------------------------------------------------------------------------------
def test_sac_exchange_slots_are_per_stream(ops, dev, streams):
    """ops.sac_update at S = 11, A = 3, [256, 256], one critic (the smallest shape of tests/test_sac.py whose second layer splits), batches
    of 37, 64 and 100: granules, arrival counters and nonces per (device, stream)"""
    S, A = 11, 3
    spec = ops.SacSpec(S, A, (256, 256), 1)

    def make(B):
        g = th.Generator(device=dev).manual_seed(7 * B)
        r = lambda *shape: th.randn(shape, device=dev, generator=g)                                     # noqa: E731
        flag = lambda: (th.rand(B, device=dev, generator=g) > 0.1).float()                              # noqa: E731
        init = [0.05 * r(n) for n in (spec.actor_count, spec.critic_count, spec.critic_count)]
        steps = [((r(B, S), r(B, A).tanh(), r(B), flag(), flag(), r(B, S)), r(B, A), r(B, A)) for _ in range(2)]
        return B, init, steps

    def run(c):
        B, init, steps = c
        pa, pc, pt = [x.clone() for x in init]
        alpha = th.full((1,), -1.0, device=dev)
        mom = [th.zeros_like(pa), th.zeros_like(pa), th.zeros_like(pc), th.zeros_like(pc), th.zeros(1, device=dev), th.zeros(1, device=dev)]
        objs, td, out = th.zeros(2, device=dev), th.zeros(B, device=dev), []
        for step, (batch, e_next, e_cur) in enumerate(steps, 1):
            ops.sac_update(spec, pa, pc, pt, alpha, mom, list(batch), step, gamma=0.97, target_entropy=-float(A), tau=5e-3, lr=1e-3,
                           max_norm=3.0, objs_out=objs, noises=(e_next, e_cur), td_error_out=td)
            out += [objs.clone(), td.clone()]
        return tuple([pa, pc, pt, alpha] + mom + out)

    interleaved(streams, [make(B) for B in (37, 64, 100)], run)
