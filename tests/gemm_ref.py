"""References, input regimes, comparators and the case lists of the operator-level GEMM tests (tests/test_gemm_forms_gpu.py drives the
kernels of csrc/gemm_tiles.h through erl_dense_*; tests/test_gemm_ref_cpu.py proves that the comparators have teeth).  numpy only.

One dense layer's three contractions, row-major fp32:
    forward         Y (rows, Nw) = act(X (rows, K) . W (Nw, K)^T + b)         reduction length K       output rows x Nw
    backward_input  dX (rows, K) = [gate *] dZ (rows, Nw) . W (Nw, K) [+ dX]  reduction length Nw      output rows x K
    weight_grad     dW (Nw, K) = dZ^T . X,  db (Nw) = column sums of dZ       reduction length rows    output Nw x K

Three input regimes, one comparator each:

EXACT.  Every operand, the bias, the gate and the pre-fill of an accumulating output hold non-zero integers in [-8, 8].  A product is at
most 64 in magnitude, so every partial sum of at most 2^18 terms is an integer below 2^24: exact in fp32 in any summation order.  The
result must equal the integer reference bit for bit (`exact_problems`); a dropped, duplicated or mis-indexed term changes at least one
integer.  (The integers are exact in bf16 as well: this regime cannot see a precision downgrade; the next one does.)

ROUNDING.  Magnitudes uniform in [0.5, 2), random signs.  The kernel's result is a chain of fp32 fmas in some order: K products, each
added to a partial sum with one rounding (K roundings), the bias (or the pre-fill) added with one more, the gate multiplied with one more.
The standard forward bound for such a chain of n roundings is gamma_n * sum of the terms' magnitudes, gamma_n = n u / (1 - n u), u = 2^-24
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), whatever the order.  With n = K + 2 and n u < 2^-15 the first-order
(K + 2) u is used as stated, against the fp64 product of the same fp32 inputs (whose own error, K 2^-53 relative, is nine orders below).
The terms are the K products and, where there is one, the bias or the pre-fill; a gate scales the whole bound.

GELU.  X holds integers, W and b multiples of 1/16, so z = X . W^T + b is exact in fp32 and in fp64 and all of the error in Y = GELU(z) and
G = GELU'(z) is the epilogue's (gelu_and_grad_fast: erf by Abramowitz-Stegun 7.1.26, __expf, a hardware reciprocal).  b is drawn per
column so that every z of the case lies in [-10, 10].  Reference: exact-erf GELU z Phi(z) and Phi(z) + z phi(z) in fp64.  Bar:
    |Y - y|   <= 0.75e-7 |z| + R max(1, |z|),      |G - gd| <= 0.75e-7 + R max(1, |z|)
0.75e-7 is A&S 7.1.26's |erf error| <= 1.5e-7 carried through Phi = (1 + erf) / 2; R = 2 x the rounding allowance measured on the device
over the whole case set (profiles/gemm_forms_gelu_error.txt records the measurement and the z at which it occurred).
"""
import math

import numpy as np

FORWARD, BACKWARD, WGRAD = "forward", "backward_input", "weight_grad"
CONTRACTIONS = (FORWARD, BACKWARD, WGRAD)
# epilogues by contraction (csrc/gemm_tiles.h EPI_*): the forward runs BIAS and BIAS_GELU, the backward STORE, ACC and MUL, the weight
# gradient PARTIAL (with its row sums)
EPI_FORWARD = ("bias", "gelu")
EPI_BACKWARD = ("store", "acc", "mul")

U32 = 2.0 ** -24
GUARD = 256                    # floats of sentinel on either side of every output
SENTINEL = np.float32(-12345.5)

# ---- gemm_launch's rule (csrc/gemm_tiles.h), restated: which kernel and which load forms a call takes --------------------------------
DW_CHUNK = 256                 # csrc/mlpn_common.h


def cdiv(a, b):
    return -(-a // b)


def gemm_dims(contraction, rows, Nw, K):
    """(M, N, reduction length) of the kernel's C = M x N"""
    return {FORWARD: (rows, Nw, K), BACKWARD: (rows, K, Nw), WGRAD: (Nw, K, rows)}[contraction]


def n_splits(contraction, rows, split=True):
    return cdiv(rows, DW_CHUNK) if contraction == WGRAD and split and rows >= 4 * DW_CHUNK else 1


def tiles64(contraction, rows, Nw, K, split=True):
    M, N, _ = gemm_dims(contraction, rows, Nw, K)
    return cdiv(M, 64) * cdiv(N, 64) * n_splits(contraction, rows, split)


def expected_form(contraction, rows, Nw, K, aligned_a=True, aligned_b=True, split=True):
    """out_form of the entry: 0 = the 32 x 32-tile kernel, 1 + 2 VA + VB = the 64 x 64-tile kernel; aligned_*: the operand's base is 16-byte
    aligned.  Operand A is X / dZ / dZ, operand B is W / W / X."""
    if tiles64(contraction, rows, Nw, K, split) < 128:
        return 0
    if contraction == FORWARD:        # both operands reduction-contiguous, ld = K: the reduction length must be a multiple of 4
        va, vb = K % 4 == 0, K % 4 == 0
    elif contraction == BACKWARD:     # A = dZ (ld = Nw, reduction-contiguous), B = W (ld = K, output-contiguous)
        va, vb = Nw % 4 == 0, K % 4 == 0
    else:                             # A = dZ (ld = Nw, output-contiguous), B = X (ld = K, output-contiguous)
        va, vb = Nw % 4 == 0, K % 4 == 0
    return 1 + 2 * int(va and aligned_a) + int(vb and aligned_b)


# ---- the case lists --------------------------------------------------------------------------------------------------------------
EDGES = (1, 31, 32, 33, 63, 64, 65, 129)
SMALL_FORWARD = tuple((r, n, k) for r in EDGES for n in EDGES for k in EDGES)                  # the full product
# a Latin square over EDGES (the third index is (i + j) mod 8): 64 triples in which every value of every axis meets every value of every
# other axis exactly once
SMALL_LATIN = tuple((EDGES[i], EDGES[j], EDGES[(i + j) % 8]) for i in range(8) for j in range(8))
SMALL_WGRAD_UNSPLIT_ROWS = (1, 63, 64, 65, 1023)
SMALL_WGRAD_SPLIT_ROWS = (1024, 1025, 1279, 1281)                                              # last chunk: full, 1 row, 255 rows, 1 row
SMALL_WGRAD_NK = ((3, 5), (33, 31), (64, 1))

LARGE_R_ONE_TILE = (128, 129)                  # output one tile wide
LARGE_R_WIDE = (7, 8, 9, 15, 16, 17)           # row tiles of outputs several tiles wide (the XCD remap with and without a partial group of 8)
LARGE_R = LARGE_R_ONE_TILE + LARGE_R_WIDE
LARGE_REM = (0, 1, 33, 63)                     # rows = 64 R + r
LARGE_WIDTH_FORMS = ("64nx", "64nx-1", "64(nx-1)+1", "64(nx-1)+33")
LARGE_RED = (1, 31, 32, 33, 64, 65, 95, 96, 97, 129, 160)      # reduction chunks of 32: 1 .. 5, ragged and whole tails


def _large_shape(R, r, wform, red):
    rows = 64 * R + r
    ny = R + (1 if r else 0)
    nx = 1 if R in LARGE_R_ONE_TILE else cdiv(128, ny)          # as many column tiles as the 128-tile rule needs
    width = {"64nx": 64 * nx, "64nx-1": 64 * nx - 1, "64(nx-1)+1": 64 * (nx - 1) + 1, "64(nx-1)+33": 64 * (nx - 1) + 33}[wform]
    return rows, width, red


def large_cases(contraction):
    """[(epilogue, rows, Nw, K, (R, r, width form, reduction length))]: per epilogue 22 cases in which every value of every list above
    appears at least once, and two with whole row tiles only (7 of them: no remapped tile; 16: every tile remapped); every case has
    >= 128 tiles of 64 x 64"""
    out = []
    for e, epi in enumerate(EPI_FORWARD if contraction == FORWARD else EPI_BACKWARD):
        for i in range(22):
            R = LARGE_R[(3 * i + e) % 8]
            r = LARGE_REM[(i + i // 8 + e) % 4]
            wf = LARGE_WIDTH_FORMS[(i + i // 4 + e) % 4]
            red = LARGE_RED[(i + 4 * e) % 11]
            rows, width, red = _large_shape(R, r, wf, red)
            Nw, K = (width, red) if contraction == FORWARD else (red, width)
            out.append((epi, rows, Nw, K, (R, r, wf, red)))
        for R, wf, red in ((7, LARGE_WIDTH_FORMS[e % 4], 97), (16, LARGE_WIDTH_FORMS[(e + 1) % 4], 33)):
            rows, width, red = _large_shape(R, 0, wf, red)
            Nw, K = (width, red) if contraction == FORWARD else (red, width)
            out.append((epi, rows, Nw, K, (R, 0, wf, red)))
    return out


# (Nw, K) of the large weight-gradient cases.  The last pair stands for an output far wider than tall whose last column tile holds 4
# columns; widths above 4096 (ERL_MAXN_WIDTH) are refused by the entry as by every network of the library, so it is 63 * 64 + 4.
LARGE_WGRAD_NK = ((130, 130), (64, 256), (257, 63), (4, 4036))
LARGE_WGRAD_REM = (0, 1, 31, 255)


def large_wgrad_cases():
    """[(rows, Nw, K)]: rows = 256 s + r, s the smallest count of full chunks with >= 128 tiles (and at least the 4 chunks from which the
    contraction is split at all)"""
    out = []
    for Nw, K in LARGE_WGRAD_NK:
        s = max(4, cdiv(128, cdiv(Nw, 64) * cdiv(K, 64)))
        out += [(DW_CHUNK * s + r, Nw, K) for r in LARGE_WGRAD_REM]
    return out


# one mid-size shape per contraction for the four load forms (extents multiples of 4; >= 128 tiles)
LOAD_FORM_SHAPES = {FORWARD: (4160, 132, 68), BACKWARD: (4160, 68, 132), WGRAD: (2817, 132, 196)}
# the same with one extent no multiple of 4: (shape, operands that lose their 16-byte loads)
LOAD_FORM_RAGGED = {FORWARD: (((4160, 132, 67), "ab"),),
                    BACKWARD: (((4160, 67, 132), "a"), ((4160, 68, 131), "b"), ((4160, 67, 131), "ab")),
                    WGRAD: (((2817, 131, 196), "a"), ((2817, 132, 195), "b"), ((2817, 131, 195), "ab"))}

ROUNDING_MAX_RED = 300


# ---- the regimes' inputs ------------------------------------------------------------------------------------------------------------
def exact_ints(rng, shape):
    """non-zero integers in [-8, 8] as fp32"""
    return (rng.integers(1, 9, size=shape) * rng.choice((-1, 1), size=shape)).astype(np.float32)


def rounding_values(rng, shape):
    """magnitudes uniform in [0.5, 2), random signs, fp32"""
    return (rng.uniform(0.5, 2.0, size=shape) * rng.choice((-1.0, 1.0), size=shape)).astype(np.float32)


def gelu_inputs(rng, rows, Nw, K):
    """X integers, W in {-1/16, +1/16}, b multiples of 1/16 drawn per column so that every z = X . W^T + b lies in [-10, 10]; the
    integers' amplitude shrinks with K so that the dot products stay a few units wide and b carries the spread"""
    amp = max(1, min(8, int(8 / math.sqrt(K))))
    X = (rng.integers(1, amp + 1, size=(rows, K)) * rng.choice((-1, 1), size=(rows, K))).astype(np.float32)
    W = (rng.choice((-1.0, 1.0), size=(Nw, K)) / 16.0).astype(np.float32)
    dot16 = np.rint(X.astype(np.float64) @ (16.0 * W.astype(np.float64)).T).astype(np.int64)      # 16 * dot, integers
    lo, hi = -160 - dot16.min(axis=0), 160 - dot16.max(axis=0)
    assert (lo <= hi).all(), "the dot products of one column span more than 20"
    b16 = rng.integers(lo, hi + 1)
    return X, W, (b16 / 16.0).astype(np.float32)


# ---- references ---------------------------------------------------------------------------------------------------------------------
def _i64(x):
    i = np.rint(x).astype(np.int64)
    assert (i == x).all(), "the exact regime takes integers"
    return i


def _imatmul(a, b):
    """integer matrix product through fp64 BLAS: exact while every partial sum stays below 2^53 (numpy's own int64 product is a plain
    loop, two orders slower at the large cases)"""
    p = a.astype(np.float64) @ b.astype(np.float64)
    assert np.abs(p).max(initial=0) < 2.0 ** 52
    return np.rint(p).astype(np.int64)


def int_to_f32(ref):
    """the fp32 image of an integer reference, which must be exact"""
    assert np.abs(ref).max(initial=0) < 2 ** 24, "the integer reference leaves fp32's exact range"
    return ref.astype(np.float32)


def forward_exact(X, W, b):
    return int_to_f32(_imatmul(_i64(X), _i64(W).T) + _i64(b)[None, :])


def backward_exact(dZ, W, epi, gate=None, prefill=None):
    acc = _imatmul(_i64(dZ), _i64(W))
    if epi == "mul":      # (an fp32 product of the two exact factors: keeps the sign of a zero as the kernel's multiply does)
        int_to_f32(acc * _i64(gate))
        return int_to_f32(acc) * gate.astype(np.float32)
    return int_to_f32(acc + _i64(prefill)) if epi == "acc" else int_to_f32(acc)


def wgrad_exact(dZ, X):
    return int_to_f32(_imatmul(_i64(dZ).T, _i64(X))), int_to_f32(_i64(dZ).sum(axis=0))


def product_f64(contraction, A, B):
    """(fp64 product of the fp32 operands, product of their magnitudes) in the output's layout; A, B as the entry takes them"""
    a, b = A.astype(np.float64), B.astype(np.float64)
    if contraction == FORWARD:
        return a @ b.T, np.abs(a) @ np.abs(b).T
    if contraction == BACKWARD:
        return a @ b, np.abs(a) @ np.abs(b)
    return a.T @ b, np.abs(a).T @ np.abs(b)


_Z16 = np.arange(-160, 161)
_ZT = _Z16 / 16.0
_PHI = np.array([0.5 * math.erfc(-z / math.sqrt(2.0)) for z in _ZT])                 # (erfc: no cancellation in the lower tail)
_PDF = np.exp(-0.5 * _ZT * _ZT) / math.sqrt(2.0 * math.pi)
_GELU_Y, _GELU_GD = _ZT * _PHI, _PHI + _ZT * _PDF


def gelu_f64(z):
    """(GELU(z), GELU'(z)) in fp64, exact erf; z multiples of 1/16 in [-10, 10]"""
    i = np.rint(np.asarray(z, dtype=np.float64) * 16.0).astype(np.int64)
    assert (i / 16.0 == z).all() and np.abs(i).max(initial=0) <= 160, "z is no multiple of 1/16 in [-10, 10]"
    return _GELU_Y[i + 160], _GELU_GD[i + 160]


# ---- comparators: each returns a list of problems (empty = accepted) -----------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def exact_problems(got, ref, what="C"):
    """bit equality of an fp32 result with the fp32 image of the integer reference"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != np.float32:
        return [f"{what}: shape / dtype {got.shape} {got.dtype} against {ref.shape} float32"]
    bad = _bits(got) != _bits(ref)
    if not bad.any():
        return []
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    return [f"{what}: {int(bad.sum())} of {bad.size} elements differ from the integer reference, first at {at}: {got[at]!r} against {ref[at]!r}"]


def rounding_bound(n_red, magnitude):
    """(K + 2) 2^-24 times the sum of the terms' magnitudes"""
    return (n_red + 2) * U32 * magnitude


def rounding_problems(got, ref64, n_red, magnitude, what="C"):
    got = np.asarray(got, dtype=np.float64)
    if got.shape != ref64.shape:
        return [f"{what}: shape {got.shape} against {ref64.shape}"]
    err, bound = np.abs(got - ref64), rounding_bound(n_red, magnitude)
    bad = ~(err <= bound)                                              # (a NaN fails)
    if not bad.any():
        return []
    at = tuple(int(v) for v in np.argwhere(bad)[0])
    return [f"{what}: {int(bad.sum())} of {bad.size} elements beyond (K + 2) 2^-24 sum|a||b| (K = {n_red}), first at {at}: error {err[at]:.3e}, "
            f"bound {bound[at]:.3e}; largest error / bound {np.nanmax(err / bound):.3g}"]


AS_CDF = 0.75e-7               # Abramowitz-Stegun 7.1.26: |erf error| <= 1.5e-7, halved by Phi = (1 + erf) / 2
GELU_BAR_CAP = 1e-6            # the asserted rounding part must stay below this times max(1, |z|)


def gelu_excess(Y, G, z):
    """what the rounding allowance has to cover: (error - A&S term) / max(1, |z|), elementwise, for Y and (G not None) for G"""
    y, gd = gelu_f64(z)
    az = np.abs(np.asarray(z, dtype=np.float64))
    scale = np.maximum(1.0, az)
    ey = (np.abs(np.asarray(Y, dtype=np.float64) - y) - AS_CDF * az) / scale
    eg = None if G is None else (np.abs(np.asarray(G, dtype=np.float64) - gd) - AS_CDF) / scale
    return ey, eg


def gelu_problems(Y, G, z, allowance):
    """the bar: A&S term + 2 x allowance x max(1, |z|)"""
    R = 2.0 * allowance
    assert 0.0 <= R < GELU_BAR_CAP
    out = []
    for name, ex in zip(("Y", "G"), gelu_excess(Y, G, z)):
        if ex is None:
            continue
        bad = ~(ex <= R)
        if bad.any():
            at = tuple(int(v) for v in np.argwhere(bad)[0])
            out.append(f"{name}: {int(bad.sum())} of {bad.size} elements beyond the bar, first at {at} (z = {np.asarray(z)[at]}): excess "
                       f"{ex[at]:.3e} per max(1, |z|) against {R:.3e}; largest {np.nanmax(ex):.3e}")
    return out


# ---- guarded outputs (host images; the GPU test uploads them and checks what comes back) ---------------------------------------------
def guarded(payload):
    """[GUARD sentinels | payload | GUARD sentinels] as one flat fp32 array"""
    flat = np.asarray(payload, dtype=np.float32).reshape(-1)
    return np.concatenate([np.full(GUARD, SENTINEL, np.float32), flat, np.full(GUARD, SENTINEL, np.float32)])


def guard_problems(buf, n, what="C"):
    """the sentinels around a payload of n floats are untouched and no NaN is left in the payload"""
    buf = np.asarray(buf)
    out = []
    s = _bits(np.full(1, SENTINEL))[0]
    for name, part in (("front", buf[:GUARD]), ("back", buf[GUARD + n:])):
        hit = _bits(part) != s
        if part.size != GUARD or hit.any():
            out.append(f"{what}: {int(hit.sum())} floats of the {name} guard band were written (first at {int(np.argmax(hit))})")
    nan = np.isnan(buf[GUARD:GUARD + n])
    if nan.any():
        out.append(f"{what}: {int(nan.sum())} of {n} payload elements were never written (first at {int(np.argmax(nan))})")
    return out
