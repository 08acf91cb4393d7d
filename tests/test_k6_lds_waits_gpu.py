"""Same bits from the split-arithmetic minibatch kernel after its LDS waits were rearranged: SHA-256 digests of the gradient slabs
(the logged sums are part of every slab) of erl_ppo_step_f32 and of the one-call update loop (which hands the kernel weight images)
against tests/golden/k6_slab_digests.json, recorded from the commit before the change by this file's own --record path:

    python tests/test_k6_lds_waits_gpu.py --record [PATH]

Cases: the smallest that reach every changed path -- B = 128 (one workgroup per network) and 130 (a second, nearly empty tile with
masked rows), S = 64 and 60 (unaligned first layer), the four nets, A = 8 and 1, with and without weight images."""
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "k6_slab_digests.json")

pytestmark = pytest.mark.gpu

NETS = [(128, 128), (128, 64), (64, 128), (64, 64)]
SHAPES = list(itertools.product((128, 130), (64, 60), (8, 1)))          # (B, S, A)
H, N = 3, 50


def _case(B, S, A, h1, h2):
    rng = np.random.default_rng(1000003 * B + 1009 * S + 101 * A + 7 * h1 + h2)
    f32 = np.float32

    def net(out, with_std):
        parts = []
        for o, i in ((h1, S), (h2, h1), (out, h2)):
            parts += [(rng.standard_normal((o, i)) / np.sqrt(i)).astype(f32).reshape(-1), (0.1 * rng.standard_normal(o)).astype(f32)]
        if with_std:
            parts.append((-0.3 + 0.1 * rng.standard_normal(out)).astype(f32))
        return np.concatenate(parts), (0.1 * rng.standard_normal(S)).astype(f32), (1.0 + 0.2 * rng.random(S)).astype(f32)

    actor, critic = net(A, True), net(1, False)
    buf = (rng.standard_normal((H, N, S), dtype=f32), rng.standard_normal((H, N, A), dtype=f32) * f32(0.7), rng.random((H, N)) > 0.1,
           (-1.0 * A + 0.3 * rng.standard_normal((H, N))).astype(f32), rng.standard_normal((H, N), dtype=f32),
           rng.standard_normal((H, N), dtype=f32))
    ids = rng.integers(0, H * N, size=B).astype(np.int64)
    return actor, critic, buf, ids


def _digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _run(ops, dev, B, S, A, h1, h2, images):
    cu = lambda a: th.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    (pa, avg_a, std_a), (pc, avg_c, std_c), buf, ids = _case(B, S, A, h1, h2)
    stride, n_slabs = ops.ppo_slab_stride(S, h1, h2, A), ops.ppo_num_slabs(B)
    norm = [cu(avg_a), cu(std_a), cu(avg_c), cu(std_c)]
    tb = [cu(x) for x in buf]
    slabs = th.zeros((n_slabs, stride), device=dev)
    if images:
        P = cu(np.concatenate([pa, pc]))
        rows = th.zeros((1, stride), device=dev)
        ops.ppo_update(P, th.zeros_like(P), th.zeros_like(P), *norm, S, h1, h2, A, *tb, cu(ids.reshape(1, B)), 0.25, 0.001, slabs, rows, 1,
                       1e-3, 3.0)
        th.cuda.synchronize()
        return _digest(slabs) + ":" + _digest(rows)
    ops.ppo_step(cu(pa), cu(pc), *norm, S, h1, h2, A, *tb, cu(ids), 0.25, 0.001, 1.0 / B, slabs, n_slabs)
    th.cuda.synchronize()
    return _digest(slabs)


def _key(B, S, A, h1, h2, images):
    return f"B{B}_S{S}_A{A}_net{h1}x{h2}_{'images' if images else 'plain'}"


def _all(ops, dev, h1, h2, images):
    prev = ops.ppo_set_arith("split")
    try:
        for B, S, A in SHAPES:
            assert ops.ppo_arith_in_use(S, h1, h2, A) == "split"
        return {_key(B, S, A, h1, h2, images): _run(ops, dev, B, S, A, h1, h2, images) for B, S, A in SHAPES}
    finally:
        ops.ppo_set_arith(prev)


@pytest.mark.parametrize("images", [False, True], ids=["plain", "images"])
@pytest.mark.parametrize("h1,h2", NETS)
def test_slabs_and_logged_sums_keep_their_bits(h1, h2, images):
    from elegantrl_amd import ops
    with open(GOLDEN) as f:
        want = json.load(f)["digests"]
    got = _all(ops, th.device("cuda:0"), h1, h2, images)
    assert set(got) <= set(want)
    bad = [k for k in got if got[k] != want[k]]
    assert not bad, f"slab digests differ from the recorded ones: {bad}"


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    from elegantrl_amd import ops as _ops
    digests = {}
    for (h1_, h2_), img in itertools.product(NETS, (False, True)):
        first = _all(_ops, th.device("cuda:0"), h1_, h2_, img)
        assert first == _all(_ops, th.device("cuda:0"), h1_, h2_, img), "the kernel is not deterministic from call to call"
        digests.update(first)
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    with open(path, "w") as f:
        json.dump({"what": "SHA-256 of the fp32 slabs (and, with images, ':' + the reduced gradient row) per case", "digests": digests}, f,
                  indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(digests)} digests to {path}")
