"""Every kernel form of csrc/gemm_tiles.h, one dense layer at a time, against exact references (tests/gemm_ref.py: the three input
regimes, their comparators and the case lists; tests/test_gemm_ref_cpu.py shows that the comparators reject what they should).

The layers are reached through erl_dense_forward_f32 / erl_dense_backward_input_f32 / erl_dense_weight_grad_f32, which call the host helpers
the networks call: gemm_launch picks the kernel (32 x 32 tiles below 128 tiles of 64 x 64, else 64 x 64 tiles) and the load forms (16-byte or
scalar, per operand) by its production rule, and every case asserts the `out_form` it was built for -- a case meant for the large kernel
cannot quietly run on the small one.  Every output sits between two guard bands of 256 sentinel floats and starts as NaN (an accumulating
output as its pre-fill): a tile that is never written, or written out of bounds, fails.

Exact regime: every case; bit equality with the integer reference.  Rounding regime: the cases with a reduction length <= 300.  GELU regime:
the forward cases; the bar's rounding part is twice GELU_ROUNDING_ALLOWANCE, measured on an MI355X over this file's whole forward case set
(profiles/gemm_forms_gelu_error.txt, written by tools/record_gemm_gelu_error.py)."""
import numpy as np
import pytest
import torch as th

from tests import gemm_ref as R

pytestmark = pytest.mark.gpu

# max over the forward case set of (error - Abramowitz-Stegun term) / max(1, |z|), Y and G together (profiles/gemm_forms_gelu_error.txt)
GELU_ROUNDING_ALLOWANCE = 1.0236e-07

FORMS_REACHED = {c: set() for c in R.CONTRACTIONS}


@pytest.fixture(scope="module")
def ops():
    from elegantrl_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def dev():
    return th.device("cuda:0")


# ---- device buffers ---------------------------------------------------------------------------------------------------------------
def up(x, dev, offset=0):
    """x on the device, `offset` floats behind a 16-byte aligned base (offset 1: an unaligned base)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    buf = th.empty(x.size + offset, dtype=th.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:].view(x.shape)
    view.copy_(th.from_numpy(x))
    return view


class Out:
    """an output of `shape` between two guard bands; starts as NaN or as `prefill`"""

    def __init__(self, dev, shape, prefill=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        host = np.full(self.n, np.nan, np.float32) if prefill is None else prefill
        self.buf = th.from_numpy(R.guarded(host)).to(dev)
        self.view = self.buf[R.GUARD:R.GUARD + self.n].view(self.shape)

    def part(self, start, shape):
        """a view of the payload (the joint dW | db output)"""
        return self.buf[R.GUARD + start:R.GUARD + start + int(np.prod(shape))].view(tuple(shape))

    def collect(self, what):
        host = self.buf.cpu().numpy()
        problems = R.guard_problems(host, self.n, what)
        assert not problems, problems
        return host[R.GUARD:R.GUARD + self.n].reshape(self.shape)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- one launch each --------------------------------------------------------------------------------------------------------------
def run_forward(ops, dev, X, W, b, gelu=False, want_g=True, off_a=0, off_b=0):
    rows, Nw = X.shape[0], W.shape[0]
    Y = Out(dev, (rows, Nw))
    G = Out(dev, (rows, Nw)) if gelu and want_g else None
    form = ops.dense_forward(up(X, dev, off_a), up(W, dev, off_b), up(b, dev), Y.view, G.view if G else None, gelu=gelu)
    FORMS_REACHED[R.FORWARD].add(form)
    return form, Y.collect("Y"), (G.collect("G") if G else None)


def run_backward(ops, dev, dZ, W, epi, extra, off_a=0, off_b=0):
    rows, K = dZ.shape[0], W.shape[1]
    dX = Out(dev, (rows, K), prefill=extra if epi == "acc" else None)
    form = ops.dense_backward_input(up(dZ, dev, off_a), up(W, dev, off_b), dX.view, up(extra, dev) if epi == "mul" else None,
                                    accumulate=epi == "acc")
    FORMS_REACHED[R.BACKWARD].add(form)
    return form, dX.collect("dX")


def run_wgrad(ops, dev, dZ, X, joint, split=True, off_a=0, off_b=0, twice=False):
    Nw, K = dZ.shape[1], X.shape[1]
    d_dZ, d_X = up(dZ, dev, off_a), up(X, dev, off_b)
    results = []
    for _ in range(2 if twice else 1):
        if joint:                        # db right behind dW, as in a parameter block: one fixed-order sum folds both
            both = Out(dev, (Nw * K + Nw,))
            dW, db = both.part(0, (Nw, K)), both.part(Nw * K, (Nw,))
            assert db.data_ptr() == dW.data_ptr() + 4 * Nw * K
        else:
            oW, ob = Out(dev, (Nw, K)), Out(dev, (Nw,))
            dW, db = oW.view, ob.view
        form = ops.dense_weight_grad(d_dZ, d_X, dW, db, split=split)
        FORMS_REACHED[R.WGRAD].add(form)
        if joint:
            flat = both.collect("dW|db")
            results.append((form, flat[:Nw * K].reshape(Nw, K), flat[Nw * K:]))
        else:
            results.append((form, oW.collect("dW"), ob.collect("db")))
    if twice:                            # the split sum is a fixed-order sum: the same bits every time
        assert results[0][0] == results[1][0]
        assert np.array_equal(bits(results[0][1]), bits(results[1][1])) and np.array_equal(bits(results[0][2]), bits(results[1][2]))
    return results[0]


# ---- one case each: every regime the case takes -------------------------------------------------------------------------------------
def check(problems, case):
    assert not problems, (case, problems)


def gelu_run(ops, dev, shape, want_form=None):
    """the GELU regime of one forward shape: (z as the BIAS form returned it, Y, G)"""
    rows, Nw, K = shape
    X, W, b = R.gelu_inputs(np.random.default_rng([3, rows, Nw, K]), rows, Nw, K)
    z64 = X.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    form, Z, _ = run_forward(ops, dev, X, W, b)
    check(R.exact_problems(Z, z64.astype(np.float32), "z"), ("gelu regime: z of the BIAS form", shape))
    form_g, Y, G = run_forward(ops, dev, X, W, b, gelu=True)
    form_n, Y_alone, _ = run_forward(ops, dev, X, W, b, gelu=True, want_g=False)
    assert form == form_g == form_n and (want_form is None or form == want_form), (shape, form, form_g, form_n, want_form)
    assert np.array_equal(bits(Y), bits(Y_alone)), ("G == NULL changed Y", shape)
    return Z, Y, G


def forward_case(ops, dev, shape, want_form):
    rows, Nw, K = shape
    rng = np.random.default_rng([1, rows, Nw, K])
    X, W, b = R.exact_ints(rng, (rows, K)), R.exact_ints(rng, (Nw, K)), R.exact_ints(rng, Nw)
    form, Y, _ = run_forward(ops, dev, X, W, b)
    assert form == want_form, (shape, form, want_form)
    check(R.exact_problems(Y, R.forward_exact(X, W, b), "Y"), ("exact", R.FORWARD, shape))
    if K <= R.ROUNDING_MAX_RED:
        X, W, b = R.rounding_values(rng, (rows, K)), R.rounding_values(rng, (Nw, K)), R.rounding_values(rng, Nw)
        form, Y, _ = run_forward(ops, dev, X, W, b)
        prod, mag = R.product_f64(R.FORWARD, X, W)
        b64 = b.astype(np.float64)
        assert form == want_form
        check(R.rounding_problems(Y, prod + b64, K, mag + np.abs(b64), "Y"), ("rounding", R.FORWARD, shape))
    Z, Y, G = gelu_run(ops, dev, shape, want_form)
    check(R.gelu_problems(Y, G, Z, GELU_ROUNDING_ALLOWANCE), ("gelu", shape))


def backward_case(ops, dev, shape, epi, want_form):
    rows, Nw, K = shape
    rng = np.random.default_rng([2, rows, Nw, K, R.EPI_BACKWARD.index(epi)])
    dZ, W, extra = R.exact_ints(rng, (rows, Nw)), R.exact_ints(rng, (Nw, K)), R.exact_ints(rng, (rows, K))
    form, dX = run_backward(ops, dev, dZ, W, epi, extra)
    assert form == want_form, (shape, epi, form, want_form)
    check(R.exact_problems(dX, R.backward_exact(dZ, W, epi, gate=extra, prefill=extra), "dX"), ("exact", R.BACKWARD, epi, shape))
    if Nw <= R.ROUNDING_MAX_RED:
        dZ, W, extra = R.rounding_values(rng, (rows, Nw)), R.rounding_values(rng, (Nw, K)), R.rounding_values(rng, (rows, K))
        form, dX = run_backward(ops, dev, dZ, W, epi, extra)
        prod, mag = R.product_f64(R.BACKWARD, dZ, W)
        e64 = extra.astype(np.float64)
        if epi == "mul":
            prod, mag = prod * e64, mag * np.abs(e64)
        elif epi == "acc":
            prod, mag = prod + e64, mag + np.abs(e64)
        assert form == want_form
        check(R.rounding_problems(dX, prod, Nw, mag, "dX"), ("rounding", R.BACKWARD, epi, shape))


def wgrad_case(ops, dev, shape, joint, want_form, split=True):
    rows, Nw, K = shape
    rng = np.random.default_rng([4, rows, Nw, K])
    dZ, X = R.exact_ints(rng, (rows, Nw)), R.exact_ints(rng, (rows, K))
    is_split = R.n_splits(R.WGRAD, rows, split) > 1
    form, dW, db = run_wgrad(ops, dev, dZ, X, joint, split=split, twice=is_split)
    assert form == want_form, (shape, joint, form, want_form)
    ref_w, ref_b = R.wgrad_exact(dZ, X)
    check(R.exact_problems(dW, ref_w, "dW") + R.exact_problems(db, ref_b, "db"), ("exact", R.WGRAD, shape, "joint" if joint else "separate"))
    if rows <= R.ROUNDING_MAX_RED:
        dZ, X = R.rounding_values(rng, (rows, Nw)), R.rounding_values(rng, (rows, K))
        form, dW, db = run_wgrad(ops, dev, dZ, X, joint, split=split)
        prod, mag = R.product_f64(R.WGRAD, dZ, X)
        z64 = dZ.astype(np.float64)
        assert form == want_form
        check(R.rounding_problems(dW, prod, rows, mag, "dW") + R.rounding_problems(db, z64.sum(axis=0), rows, np.abs(z64).sum(axis=0), "db"),
              ("rounding", R.WGRAD, shape))


# ---- the small kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", R.EDGES)
def test_small_kernel_forward_full_product(ops, dev, rows):
    for shape in (s for s in R.SMALL_FORWARD if s[0] == rows):           # includes Nw = 1 (a value head) and K = 1
        forward_case(ops, dev, shape, 0)


@pytest.mark.parametrize("epi", R.EPI_BACKWARD)
def test_small_kernel_backward_input(ops, dev, epi):
    for shape in R.SMALL_LATIN:
        backward_case(ops, dev, shape, epi, 0)


@pytest.mark.parametrize("joint", [True, False], ids=["joint_db", "separate_db"])
def test_small_kernel_weight_grad(ops, dev, joint):
    for shape in R.SMALL_LATIN:
        wgrad_case(ops, dev, shape, joint, 0)


@pytest.mark.parametrize("joint", [True, False], ids=["joint_db", "separate_db"])
@pytest.mark.parametrize("rows", R.SMALL_WGRAD_UNSPLIT_ROWS + R.SMALL_WGRAD_SPLIT_ROWS)
def test_small_kernel_weight_grad_unsplit_and_split(ops, dev, rows, joint):
    for Nw, K in R.SMALL_WGRAD_NK:
        wgrad_case(ops, dev, (rows, Nw, K), joint, 0)
        if rows in R.SMALL_WGRAD_SPLIT_ROWS:                             # the same rows in one pass: no scratch, no split
            wgrad_case(ops, dev, (rows, Nw, K), joint, 0, split=False)


# ---- the large kernel ---------------------------------------------------------------------------------------------------------------
def _id(case):
    return "-".join(str(v) for v in case[:4])


@pytest.mark.parametrize("case", R.large_cases(R.FORWARD), ids=_id)
def test_large_kernel_forward(ops, dev, case):
    _, rows, Nw, K, _ = case                                             # (every forward case runs both epilogues)
    want = R.expected_form(R.FORWARD, rows, Nw, K)
    assert want >= 1
    forward_case(ops, dev, (rows, Nw, K), want)


@pytest.mark.parametrize("case", R.large_cases(R.BACKWARD), ids=_id)
def test_large_kernel_backward_input(ops, dev, case):
    epi, rows, Nw, K, _ = case
    want = R.expected_form(R.BACKWARD, rows, Nw, K)
    assert want >= 1
    backward_case(ops, dev, (rows, Nw, K), epi, want)


@pytest.mark.parametrize("joint", [True, False], ids=["joint_db", "separate_db"])
@pytest.mark.parametrize("shape", R.large_wgrad_cases(), ids=lambda s: "-".join(map(str, s)))
def test_large_kernel_weight_grad(ops, dev, shape, joint):
    want = R.expected_form(R.WGRAD, *shape)
    assert want >= 1 and R.n_splits(R.WGRAD, shape[0]) >= 4
    wgrad_case(ops, dev, shape, joint, want)


def test_entries_refuse_widths_beyond_the_limit(ops, dev):
    """(4, 4100), a weight gradient 65 column tiles wide, is beyond ERL_MAXN_WIDTH: refused under the entry's name, nothing written"""
    from elegantrl_amd._hip import HipExtensionError
    dZ, X = up(np.ones((8, 4), np.float32), dev), up(np.ones((8, 4100), np.float32), dev)
    both = Out(dev, (4 * 4100 + 4,))
    with pytest.raises(HipExtensionError, match="erl_dense_weight_grad_f32.*4096"):
        ops.dense_weight_grad(dZ, X, both.part(0, (4, 4100)), both.part(4 * 4100, (4,)), split=False)
    assert np.isnan(both.buf.cpu().numpy()[R.GUARD:-R.GUARD]).all()


# ---- the four load forms ------------------------------------------------------------------------------------------------------------
_LOAD_FORMS = {}


def load_forms(ops, dev, contraction):
    """one mid-size shape with the bases of operand A and B at offset 0 or 1 float: {(off_a, off_b): (form, outputs...)} (run once)"""
    if contraction in _LOAD_FORMS:
        return _LOAD_FORMS[contraction]
    rows, Nw, K = shape = R.LOAD_FORM_SHAPES[contraction]
    rng = np.random.default_rng([5, rows, Nw, K])
    got = {}
    if contraction == R.FORWARD:
        X, W, b = R.exact_ints(rng, (rows, K)), R.exact_ints(rng, (Nw, K)), R.exact_ints(rng, Nw)
        ref = (R.forward_exact(X, W, b),)
    elif contraction == R.BACKWARD:
        dZ, W, gate = R.exact_ints(rng, (rows, Nw)), R.exact_ints(rng, (Nw, K)), R.exact_ints(rng, (rows, K))
        ref = (R.backward_exact(dZ, W, "mul", gate=gate),)
    else:
        dZ, X = R.exact_ints(rng, (rows, Nw)), R.exact_ints(rng, (rows, K))
        ref = R.wgrad_exact(dZ, X)
    for off_a in (0, 1):
        for off_b in (0, 1):
            if contraction == R.FORWARD:
                form, Y, _ = run_forward(ops, dev, X, W, b, off_a=off_a, off_b=off_b)
                outs = (Y,)
            elif contraction == R.BACKWARD:
                form, dX = run_backward(ops, dev, dZ, W, "mul", gate, off_a=off_a, off_b=off_b)
                outs = (dX,)
            else:
                form, dW, db = run_wgrad(ops, dev, dZ, X, True, off_a=off_a, off_b=off_b, twice=True)
                outs = (dW, db)
            assert form == R.expected_form(contraction, *shape, aligned_a=not off_a, aligned_b=not off_b), (contraction, off_a, off_b, form)
            for o, r in zip(outs, ref):
                check(R.exact_problems(o, r), ("exact", contraction, shape, off_a, off_b))
            got[(off_a, off_b)] = (form,) + outs
    _LOAD_FORMS[contraction] = got
    return got


@pytest.mark.parametrize("contraction", R.CONTRACTIONS)
def test_four_load_forms_give_identical_bits(ops, dev, contraction):
    got = load_forms(ops, dev, contraction)
    assert sorted(v[0] for v in got.values()) == [1, 2, 3, 4]
    first = got[(0, 0)]
    for key, val in got.items():                                         # the same data in the same order: the same bits
        for a, b in zip(first[1:], val[1:]):
            assert np.array_equal(bits(a), bits(b)), (contraction, key)


@pytest.mark.parametrize("contraction", R.CONTRACTIONS)
def test_an_extent_that_is_no_multiple_of_four_takes_scalar_loads(ops, dev, contraction):
    for shape, lost in R.LOAD_FORM_RAGGED[contraction]:
        want = 1 + 2 * ("a" not in lost) + ("b" not in lost)
        if contraction == R.FORWARD:
            forward_case(ops, dev, shape, want)
        elif contraction == R.BACKWARD:
            for epi in R.EPI_BACKWARD:
                backward_case(ops, dev, shape, epi, want)
        else:
            wgrad_case(ops, dev, shape, True, want)
            wgrad_case(ops, dev, shape, False, want)


def test_every_form_of_every_contraction_was_reached(ops, dev):
    """the small kernel and all four (VA, VB) forms of the large one, for each of the three contractions: 15 forms.  (Self-contained: the
    load-form sweep reaches the four large forms, one small case each the small kernel; the cases above add to the same record.)"""
    for c in R.CONTRACTIONS:
        load_forms(ops, dev, c)
    forward_case(ops, dev, (33, 31, 65), 0)
    backward_case(ops, dev, (33, 31, 65), "store", 0)
    wgrad_case(ops, dev, (33, 31, 65), True, 0)
    assert FORMS_REACHED == {c: {0, 1, 2, 3, 4} for c in R.CONTRACTIONS}, FORMS_REACHED
