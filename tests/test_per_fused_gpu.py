"""The two kernels behind the prioritised update loop (csrc/per.hip), each against the calls it replaces, bit for bit, on identical inputs:
erl_per_sample_rows_f32 (draw + gather in one launch) against erl_per_sample_f32 followed by erl_replay_sample_rows_f32(sample_len =
cur_size), and erl_per_update_index_f32 (the tree update that decodes the sampler's indices itself) against th.fmod / th.div +
erl_per_update_f32 and against oracle/per_numpy.py.

Shapes: the smallest at which each rule bites (the table in CASES).  The priorities are made non-uniform first (td errors from a seeded
generator, with values at and beyond both clamp ends, 1e-8 and 10), and the injected uniforms carry 0.0 and 1 - 2**-24 in the first and
the last stratum of every sequence (the `v <= left` tie at the left edge, the right edge of the last stratum)."""
import functools

import numpy as np
import pytest
import torch as th

from oracle.per_numpy import PerTrees as OraclePerTrees

pytestmark = pytest.mark.gpu

# name: (max_size, num_seqs, S, A, appends (rows per ReplayBuffer.update), n_per_seq)
CASES = {
    "L-beyond-max_size": (40, 2, 3, 2, (17,), 8),            # L = 64 > max_size, zero leaves beyond the data; not full
    "more-draws-than-rows": (8, 4, 5, 1, (3,), 16),          # duplicates, and the cur_size - 2 clamp on most draws
    "full-ring-cursor": (64, 1, 11, 3, (40, 47), 64),        # full, write position 23 after a wrap: the cursor rule, one sequence
    "bulk-update": (4096, 8, 17, 6, (3000,), 1200),          # B = 9600 > 8 x 1024: several items per thread, the bulk tree update
}
ONE_LESS = float(1 - 2.0 ** -24)


def _uniforms(Q, n, gen, dev, flip):
    u = th.rand((Q, n), device=dev, generator=gen)
    u[:, 0], u[:, -1] = (ONE_LESS, 0.0) if flip else (0.0, ONE_LESS)
    assert float(u.max()) < 1.0
    return u


def _oracle_follow(ref, trees, Q):
    """the device's leaves against the oracle's within the priority power's tolerance (tests/test_per.py: two powf, one ulp), then the
    oracle continues from the device's leaves so that everything above them is compared exactly"""
    got_sum, got_min = trees.sum.view(Q, -1).cpu().numpy(), trees.min.view(Q, -1).cpu().numpy()
    np.testing.assert_allclose(got_sum[:, ref.L:], ref.sum[:, ref.L:], rtol=2e-7)
    np.testing.assert_allclose(got_min[:, ref.L:], ref.min[:, ref.L:], rtol=2e-7)
    if not (np.array_equal(got_sum[:, ref.L:], ref.sum[:, ref.L:]) and np.array_equal(got_min[:, ref.L:], ref.min[:, ref.L:])):
        ref.sum[:, ref.L:], ref.min[:, ref.L:] = got_sum[:, ref.L:], got_min[:, ref.L:]
        for node in range(ref.L - 1, 0, -1):
            ref.sum[:, node] = ref.sum[:, 2 * node] + ref.sum[:, 2 * node + 1]
            ref.min[:, node] = np.minimum(ref.min[:, 2 * node], ref.min[:, 2 * node + 1])
    np.testing.assert_array_equal(got_sum[:, 1:], ref.sum[:, 1:])            # the tree arithmetic above the leaves: exact
    np.testing.assert_array_equal(got_min[:, 1:], ref.min[:, 1:])


@functools.lru_cache(maxsize=None)
def _setup(name):
    """the filled prioritised buffer of a case with non-uniform priorities, its oracle twin, the injected uniforms, and the reference
    route's outputs (computed once, never written to afterwards)"""
    from elegantrl_amd.train import Config, ReplayBuffer
    max_size, Q, S, A, appends, n = CASES[name]
    dev = th.device("cuda:0")
    args = Config()
    args.per_alpha, args.per_beta = 0.6, 0.4
    gen = th.Generator(device=dev).manual_seed(sum(map(ord, name)))
    buf = ReplayBuffer(max_size=max_size, state_dim=S, action_dim=A, gpu_id=0, num_seqs=Q, if_use_per=True, args=args)
    ref = OraclePerTrees(max_size, Q)
    for add in appends:
        ref.add_rows(buf.p, add)
        buf.update((th.randn((add, Q, S), device=dev, generator=gen), th.randn((add, Q, A), device=dev, generator=gen),
                    th.randn((add, Q), device=dev, generator=gen), th.rand((add, Q), device=dev, generator=gen) < 0.9,
                    th.rand((add, Q), device=dev, generator=gen) < 0.9))
    cur = buf.cur_size
    # non-uniform priorities: td errors on most transitions, some at and beyond the clamp ends
    m = max(4, (cur * Q * 3) // 4)
    idx0 = th.randint(cur * Q, (m,), device=dev, generator=gen)
    td0 = th.rand(m, device=dev, generator=gen) * 12.0                        # (a sixth of them above 10: clamped)
    td0[0], td0[1], td0[2], td0[3] = 1e-8, 10.0, 0.0, 3e-9
    buf.td_error_update_for_per(idx0, td0)
    i0 = idx0.cpu().numpy()
    ref.td_error_update(i0 % cur, i0 // cur, td0.cpu().numpy())
    _oracle_follow(ref, buf.sum_trees, Q)
    cursor = buf.p if buf.if_full else -1
    uniforms = [_uniforms(Q, n, gen, dev, flip) for flip in (False, True)]
    want = []
    for u in uniforms:                                                        # the calls the fused launch replaces
        idx, w = buf.sum_trees.sample(u, cur, buf.per_beta, cursor=cursor)
        out, ids = buf._ring.sample(idx, cur)
        want.append((idx, w, out, ids))
    td = th.rand(Q * n, device=dev, generator=gen) * 12.0
    td[0], td[-1], td[1], td[-2] = 1e-8, 10.0, 0.0, 11.5
    return dict(buf=buf, ref=ref, cur=cur, cursor=cursor, uniforms=uniforms, want=want, td=td, dev=dev)


def _tree_copy(trees, dev):
    from elegantrl_amd import ops
    t = ops.PerTrees(trees.max_size, trees.num_seqs, dev)
    t.sum.copy_(trees.sum)
    t.min.copy_(trees.min)
    return t


@pytest.mark.parametrize("name", list(CASES))
def test_draw_and_gather_in_one_launch_equals_the_two_calls(name):
    from elegantrl_amd import ops
    c = _setup(name)
    buf, (max_size, Q, S, A, _, n) = c["buf"], CASES[name]
    if name == "full-ring-cursor":
        assert buf.if_full and buf.p == 23
    for u, (idx, w, out, ids) in zip(c["uniforms"], c["want"]):
        got_out, got_ids, got_idx, got_w = ops.per_sample_rows(buf.sum_trees, buf._ring, u, c["cur"], buf.per_beta, cursor=c["cursor"])
        assert got_idx.shape == (Q * n,) and th.equal(got_idx, idx)
        assert th.equal(got_w, w) and bool(th.isfinite(got_w).all())
        for k, (x, y) in enumerate(zip(got_out, out)):       # state, action, reward, undone, unmask, next_state
            assert x.shape == y.shape and th.equal(x, y), k
        assert th.equal(got_ids[0], ids[0]) and th.equal(got_ids[1], ids[1])
        ids0 = got_ids[0]
        assert int(ids0.min()) >= 0 and int(ids0.max()) <= c["cur"] - 2
        if name == "more-draws-than-rows":                   # 3 rows: every draw lands on row 0 or 1, most of them moved there
            assert len(set(got_idx.tolist())) < got_idx.numel()
        if name == "full-ring-cursor":
            assert 22 not in set(ids0.tolist())               # the newest row is never drawn
    # a reused stage gives the same tensors (the loop's form: no allocation per step)
    st, ps = ops.ReplayStage(Q * n, S, A, False, c["dev"]), ops.PerStage(Q * n, c["dev"])
    ops.per_sample_rows(buf.sum_trees, buf._ring, c["uniforms"][0], c["cur"], buf.per_beta, cursor=c["cursor"], stage=st, per_stage=ps)
    assert th.equal(ps.is_index, c["want"][0][0]) and th.equal(st.out[5], c["want"][0][2][5])


@pytest.mark.parametrize("name", list(CASES))
def test_tree_update_from_the_samplers_indices_equals_fmod_div_and_update(name):
    from elegantrl_amd import ops
    c = _setup(name)
    buf, (max_size, Q, S, A, _, n) = c["buf"], CASES[name]
    cur, dev, td = c["cur"], c["dev"], c["td"]
    idx = c["want"][0][0]                                     # the sampler's own indices: duplicates included
    a, b = _tree_copy(buf.sum_trees, dev), _tree_copy(buf.sum_trees, dev)
    ops.per_update_index(a, idx, cur, td, buf.per_alpha)
    b.update(th.fmod(idx, cur), th.div(idx, cur, rounding_mode="floor"), td, buf.per_alpha)
    assert th.equal(a.sum, b.sum) and th.equal(a.min, b.min)
    assert not th.equal(a.sum, buf.sum_trees.sum)
    # ... against the oracle: leaves within the priority power's tolerance, everything above them exact
    ref = OraclePerTrees(max_size, Q)
    ref.sum[:], ref.min[:] = c["ref"].sum, c["ref"].min
    i = idx.cpu().numpy()
    ref.td_error_update(i % cur, i // cur, td.cpu().numpy())
    _oracle_follow(ref, a, Q)
    # ... and with indices outside the trees in the list (skipped by both routes): below zero, the first one past the last sequence, far out
    bad = th.tensor([-1, Q * cur, -(1 << 40), (1 << 40) + 3, Q * cur + cur - 1], dtype=th.int64, device=dev)
    idx2 = th.cat([bad[:2], idx, bad[2:]])
    td2 = th.cat([td.new_full((2,), 5.0), td.flip(0), td.new_full((3,), 5.0)])
    ops.per_update_index(a, idx2, cur, td2, buf.per_alpha)
    b.update(th.fmod(idx2, cur), th.div(idx2, cur, rounding_mode="floor"), td2, buf.per_alpha)
    assert th.equal(a.sum, b.sum) and th.equal(a.min, b.min)
