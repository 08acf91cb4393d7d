"""The comparators of tests/gemm_ref.py have teeth, and its case lists say what they claim (no GPU: the "kernel" here is numpy).

Exact regime: the honest fp32 result is accepted, and each corruption a tiling bug would produce -- the last reduction index left out, one
whole 32-chunk left out, two outputs swapped, the bias dropped, `=` where `+=` is meant -- is rejected at the smallest and at the largest
case shape.  Rounding regime: numpy's own fp32 product passes the derived bound at every reduction length the cases use, the same product
with operands rounded to bf16 fails it at every one.  GELU regime: z is exact, reproducible in fp64, inside [-10, 10] and, over the case
set, present in every unit interval of it."""
import numpy as np
import pytest

from tests import gemm_ref as R


def _smallest_and_largest(cases):
    """of (rows, Nw, K) triples, by the count of multiply-adds"""
    key = lambda c: (c[0] * c[1] * c[2], c)  # noqa: E731
    return min(cases, key=key), max(cases, key=key)


def _all_shapes(contraction):
    if contraction == R.FORWARD:
        return list(R.SMALL_FORWARD) + [c[1:4] for c in R.large_cases(R.FORWARD)]
    if contraction == R.BACKWARD:
        return list(R.SMALL_LATIN) + [c[1:4] for c in R.large_cases(R.BACKWARD)]
    small = [(r, n, k) for r in R.SMALL_WGRAD_UNSPLIT_ROWS + R.SMALL_WGRAD_SPLIT_ROWS for n, k in R.SMALL_WGRAD_NK]
    return list(R.SMALL_LATIN) + small + R.large_wgrad_cases()


def _operands(contraction, shape, seed=0):
    rows, Nw, K = shape
    rng = np.random.default_rng([seed, rows, Nw, K])
    if contraction == R.FORWARD:
        return R.exact_ints(rng, (rows, K)), R.exact_ints(rng, (Nw, K)), R.exact_ints(rng, Nw)
    if contraction == R.BACKWARD:
        return R.exact_ints(rng, (rows, Nw)), R.exact_ints(rng, (Nw, K)), R.exact_ints(rng, (rows, K))     # dZ, W, gate or pre-fill
    return R.exact_ints(rng, (rows, Nw)), R.exact_ints(rng, (rows, K)), None


def _f32_result(contraction, A, B, extra, epi, keep=None, assign=False, no_bias=False):
    """what a kernel would return, in fp32 arithmetic, with the reduction indices `keep` only (a corrupted kernel's view)"""
    red = A.shape[0] if contraction == R.WGRAD else A.shape[1]
    keep = np.arange(red) if keep is None else keep
    if contraction == R.FORWARD:
        acc = A[:, keep] @ B[:, keep].T
        return acc if no_bias else acc + extra[None, :]
    if contraction == R.BACKWARD:
        acc = A[:, keep] @ B[keep, :]
        if epi == "mul":
            return acc * extra
        return acc + extra if epi == "acc" and not assign else acc
    return A[keep, :].T @ B[keep, :], A[keep, :].sum(axis=0, dtype=np.float32)


def _reference(contraction, A, B, extra, epi):
    if contraction == R.FORWARD:
        return R.forward_exact(A, B, extra)
    if contraction == R.BACKWARD:
        return R.backward_exact(A, B, epi, gate=extra, prefill=extra)
    return R.wgrad_exact(A, B)


def _swap_two(x, ref):
    """x with two outputs exchanged whose reference values differ (rows when there are two that differ somewhere, else two elements)"""
    y = x.copy()
    if y.ndim == 2 and y.shape[0] > 1:
        i = next(i for i in range(1, y.shape[0]) if (ref[i] != ref[0]).any())
        y[[0, i]] = y[[i, 0]]
        return y
    flat, rf = y.reshape(-1), ref.reshape(-1)
    i = next(i for i in range(1, flat.size) if rf[i] != rf[0])
    flat[[0, i]] = flat[[i, 0]]
    return y


CASES = [(c, epi) for c in (R.FORWARD,) for epi in ("bias",)] + [(R.BACKWARD, e) for e in R.EPI_BACKWARD] + [(R.WGRAD, "partial")]


@pytest.mark.parametrize("contraction,epi", CASES)
@pytest.mark.parametrize("which", ["smallest", "largest"])
def test_exact_comparator_accepts_the_honest_result_and_rejects_each_corruption(contraction, epi, which):
    shapes = _all_shapes(contraction)
    shape = _smallest_and_largest(shapes)[which == "largest"]
    A, B, extra = _operands(contraction, shape)
    red = R.gemm_dims(contraction, *shape)[2]
    ref = _reference(contraction, A, B, extra, epi)
    refs = ref if isinstance(ref, tuple) else (ref,)

    def problems(got):
        got = got if isinstance(got, tuple) else (got,)
        return [p for g, r, n in zip(got, refs, ("C", "row sums")) for p in R.exact_problems(np.asarray(g, dtype=np.float32), r, n)]

    assert problems(_f32_result(contraction, A, B, extra, epi)) == []
    # the last reduction index left out; the last 32-chunk left out (at a reduction length of 32 or less that is every term)
    assert problems(_f32_result(contraction, A, B, extra, epi, keep=np.arange(red - 1)))
    assert problems(_f32_result(contraction, A, B, extra, epi, keep=np.arange(32 * ((red - 1) // 32))))
    if red > 64:                                                      # a chunk in the middle
        assert problems(_f32_result(contraction, A, B, extra, epi, keep=np.r_[0:32, 64:red]))
    # two outputs swapped (where the case has two outputs that differ)
    honest = _f32_result(contraction, A, B, extra, epi)
    first, first_ref = (honest[0], refs[0]) if isinstance(honest, tuple) else (honest, refs[0])
    if np.unique(first_ref).size > 1:
        swapped = _swap_two(first, first_ref)
        assert problems((swapped,) + tuple(honest[1:]) if isinstance(honest, tuple) else swapped)
    else:
        assert first_ref.size == 1, "only a single output cannot be swapped"
    if contraction == R.FORWARD:
        assert problems(_f32_result(contraction, A, B, extra, epi, no_bias=True))
    if epi == "acc":
        assert problems(_f32_result(contraction, A, B, extra, epi, assign=True))
    if contraction == R.WGRAD:                                        # the row sums alone wrong: dW right, db short of its last row
        good = _f32_result(contraction, A, B, extra, epi)
        assert problems((good[0], A[:-1].sum(axis=0, dtype=np.float32)))
    # a result in which one element was never written
    bad = np.array(first, dtype=np.float32, copy=True)
    bad.reshape(-1)[-1] = np.nan
    assert R.exact_problems(bad, first_ref)


def test_exact_comparator_sees_the_sign_of_a_zero_and_the_guards():
    ref = np.zeros((2, 2), np.float32)
    assert R.exact_problems(np.zeros((2, 2), np.float32), ref) == [] and R.exact_problems(-np.zeros((2, 2), np.float32), ref)
    buf = R.guarded(np.full(10, np.nan, np.float32))
    assert len(R.guard_problems(buf, 10)) == 1                        # never written
    buf[R.GUARD:R.GUARD + 10] = 1.0
    assert R.guard_problems(buf, 10) == []
    for at in (0, R.GUARD - 1, R.GUARD + 10, buf.size - 1):
        b2 = buf.copy()
        b2[at] = 0.0
        assert R.guard_problems(b2, 10), at


def _bf16(x):
    """fp32 rounded to bf16 (round to nearest even), as fp32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _rounding_reduction_lengths():
    reds = set()
    for c in R.CONTRACTIONS:
        reds |= {R.gemm_dims(c, *s)[2] for s in _all_shapes(c)}
    return sorted(k for k in reds if k <= R.ROUNDING_MAX_RED)


def test_rounding_bound_takes_fp32_and_refuses_bf16_at_every_reduction_length():
    reds = _rounding_reduction_lengths()
    assert reds[0] == 1 and reds[-1] <= R.ROUNDING_MAX_RED and {1, 31, 32, 33, 64, 65, 95, 96, 97, 129, 160} <= set(reds)
    ints = R.exact_ints(np.random.default_rng(1), 4096)
    assert np.array_equal(_bf16(ints), ints)                          # the exact regime's integers survive bf16: it cannot see a downgrade
    for K in reds:
        rng = np.random.default_rng([7, K])
        X, W, b = R.rounding_values(rng, (96, K)), R.rounding_values(rng, (80, K)), R.rounding_values(rng, 80)
        assert (np.abs(X) >= 0.5).all() and (np.abs(X) < 2).all()
        prod, mag = R.product_f64(R.FORWARD, X, W)
        ref, mag = prod + b.astype(np.float64), mag + np.abs(b.astype(np.float64))
        assert R.rounding_problems(X @ W.T + b, ref, K, mag) == [], K
        assert R.rounding_problems(_bf16(X) @ _bf16(W).T + b, ref, K, mag), K
        # the gated backward: the bound scales with the gate
        dZ, Wb, gate = R.rounding_values(rng, (96, K)), R.rounding_values(rng, (K, 72)), R.rounding_values(rng, (96, 72))
        bprod, bmag = R.product_f64(R.BACKWARD, dZ, Wb)
        g64 = gate.astype(np.float64)
        assert R.rounding_problems((dZ @ Wb) * gate, bprod * g64, K, bmag * np.abs(g64)) == [], K
        assert R.rounding_problems((_bf16(dZ) @ _bf16(Wb)) * gate, bprod * g64, K, bmag * np.abs(g64)), K
    # a NaN is a failure, not a pass
    bad = (X @ W.T + b).astype(np.float32)
    bad[0, 0] = np.nan
    assert R.rounding_problems(bad, ref, K, mag)


def test_gelu_regime_inputs_are_exact_and_cover_the_interval():
    shapes = [s for s in _all_shapes(R.FORWARD)]
    hist = np.zeros(20, np.int64)
    for rows, Nw, K in shapes:
        if rows * Nw * K > 1 << 22 and (rows, Nw, K) != _smallest_and_largest(shapes)[1]:
            continue                                                  # (the largest case and everything of moderate size: the rule is the same)
        rng = np.random.default_rng([3, rows, Nw, K])
        X, W, b = R.gelu_inputs(rng, rows, Nw, K)
        assert X.dtype == W.dtype == b.dtype == np.float32 and (X == np.rint(X)).all() and (X != 0).all()
        assert (16 * W == np.rint(16 * W)).all() and (16 * b == np.rint(16 * b)).all() and (W != 0).all()
        z32 = X @ W.T + b                                             # fp32 arithmetic
        z64 = X.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
        assert (z32.astype(np.float64) == z64).all(), (rows, Nw, K)   # exact: fp32 and fp64 agree to the bit
        assert np.abs(z64).max() <= 10.0
        R.gelu_f64(z64)                                               # (asserts the grid)
        hist += np.histogram(z64, bins=20, range=(-10.0, 10.0))[0]
    assert (hist > 0).all(), hist
    assert (hist / hist.sum() > 1e-3).all(), hist / hist.sum()        # every unit interval holds a real share of the z


def test_gelu_reference_and_bar():
    import math
    for z in (-10.0, -3.0625, -0.0625, 0.0, 0.5, 2.75, 10.0):
        y, gd = R.gelu_f64(np.array([z]))
        phi = 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))
        assert abs(y[0] - z * phi) < 1e-15 and abs(gd[0] - (phi + z * math.exp(-0.5 * z * z) / math.sqrt(2 * math.pi))) < 1e-15
    z = np.arange(-160, 161).reshape(3, 107) / 16.0
    y, gd = R.gelu_f64(z)
    allowance = 1e-7
    assert R.gelu_problems(y.astype(np.float32), gd.astype(np.float32), z, allowance) == []          # fp32 rounding of the exact values: 6e-8 |y|
    assert R.gelu_problems(y.astype(np.float32), None, z, allowance) == []
    # tanh-form GELU (the other "GELU") is refused: it differs from the erf form by up to 5e-4
    t = 0.5 * z * (1 + np.tanh(math.sqrt(2 / math.pi) * (z + 0.044715 * z ** 3)))
    assert R.gelu_problems(t.astype(np.float32), None, z, allowance)
    # a derivative without its density term, and a Y that is 2e-6 |z| off, are refused
    phi = np.array([0.5 * math.erfc(-v / math.sqrt(2)) for v in z.reshape(-1)]).reshape(z.shape)
    assert R.gelu_problems(y.astype(np.float32), phi.astype(np.float32), z, allowance)
    assert R.gelu_problems((y + 2e-6 * np.abs(z) + 2e-6).astype(np.float32), None, z, allowance)
    with pytest.raises(AssertionError):
        R.gelu_problems(y, gd, z, 0.5e-6)                             # twice the allowance must stay below 1e-6


def test_case_lists_cover_what_they_claim():
    assert len(R.SMALL_FORWARD) == 512 and len(set(R.SMALL_LATIN)) == 64 >= 24
    for axis in range(3):
        assert {c[axis] for c in R.SMALL_LATIN} == set(R.EDGES)
    assert all(R.expected_form(R.FORWARD, *c) == 0 for c in R.SMALL_FORWARD)
    assert all(R.expected_form(c, *s) == 0 for c in (R.BACKWARD, R.WGRAD) for s in R.SMALL_LATIN)
    for rows in R.SMALL_WGRAD_UNSPLIT_ROWS + R.SMALL_WGRAD_SPLIT_ROWS:
        for Nw, K in R.SMALL_WGRAD_NK:
            assert R.expected_form(R.WGRAD, rows, Nw, K) == 0
            assert (R.n_splits(R.WGRAD, rows) > 1) == (rows in R.SMALL_WGRAD_SPLIT_ROWS)
    assert sorted({r - 256 * (R.n_splits(R.WGRAD, r) - 1) for r in R.SMALL_WGRAD_SPLIT_ROWS}) == [1, 255, 256]     # the last chunk's rows
    # large cases: >= 128 tiles by the production rule, every value of every list with every epilogue
    for contraction, epis in ((R.FORWARD, R.EPI_FORWARD), (R.BACKWARD, R.EPI_BACKWARD)):
        cases = R.large_cases(contraction)
        assert 40 <= len(cases) <= 75
        for epi in epis:
            mine = [c for c in cases if c[0] == epi]
            for pos, values in enumerate((R.LARGE_R, R.LARGE_REM, R.LARGE_WIDTH_FORMS, R.LARGE_RED)):
                assert {c[4][pos] for c in mine} == set(values), (contraction, epi, pos)
        for epi, rows, Nw, K, _ in cases:
            assert R.tiles64(contraction, rows, Nw, K) >= 128 and R.expected_form(contraction, rows, Nw, K) >= 1
            assert max(Nw, K) <= 4096
        # the XCD remap: row-tile counts that are multiples of 8, and counts >= 8 that are not
        ny = {R.cdiv(c[1], 64) for c in cases}
        assert any(n % 8 == 0 for n in ny) and any(n >= 8 and n % 8 for n in ny) and any(n < 8 for n in ny)
        assert {R.cdiv(R.gemm_dims(contraction, *c[1:4])[2], 32) for c in cases} == {1, 2, 3, 4, 5}
    wg = R.large_wgrad_cases()
    assert len(wg) == 16 and all(R.tiles64(R.WGRAD, *c) >= 128 and R.n_splits(R.WGRAD, c[0]) >= 4 for c in wg)
    assert {c[0] % 256 for c in wg} == {0, 1, 31, 255}
    # the exact regime's premise: rows * 64 < 2^24 for every case
    for c in R.CONTRACTIONS:
        assert max(R.gemm_dims(c, *s)[2] for s in _all_shapes(c)) * 64 < 2 ** 24
    # the load-form shapes reach the large kernel, and with aligned bases the fully vectorised form
    for c, s in R.LOAD_FORM_SHAPES.items():
        assert R.expected_form(c, *s) == 4
        assert {R.expected_form(c, *s, aligned_a=a, aligned_b=b) for a in (0, 1) for b in (0, 1)} == {1, 2, 3, 4}
        for shape, lost in R.LOAD_FORM_RAGGED[c]:
            assert R.expected_form(c, *shape) == 1 + 2 * ("a" not in lost) + ("b" not in lost)
