"""Record tests/golden/ppo_update_loop_digests.json: SHA-256 of the weights, both Adam moments and the gradient rows that the one-call PPO
update loop leaves on the cases of tests/test_kernels_gpu.py::test_update_loop_matches_parent_digests.

Run it on a GPU from a checkout of the commit whose bits are the reference (the parent of a change to the loop or its kernels), with this
file and the test module of the change copied over that checkout -- never from the tree under test:

    python tools/record_update_loop_digests.py [PATH]

The cases and the run come from the test module, so the recording and the test cannot drift."""
import json
import os
import sys

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from elegantrl_amd import ops  # noqa: E402
from tests import test_kernels_gpu as T  # noqa: E402

if __name__ == "__main__":
    dev = th.device("cuda:0")
    digests = {}
    for case in T.UPDATE_LOOP_CASES:
        first, moved = T.run_update_loop_case(ops, dev, *case)
        assert first == T.run_update_loop_case(ops, dev, *case)[0], f"{case}: the loop is not deterministic from call to call"
        assert moved > 1e-4, case
        digests[T.update_loop_case_key(*case)] = first
    path = sys.argv[1] if len(sys.argv) > 1 else T.UPDATE_LOOP_DIGESTS
    with open(path, "w") as f:
        json.dump({"what": "SHA-256 of the raw fp32 bytes per case: weights, exp_avg, exp_avg_sq, the 2T gradient rows", "digests": digests}, f,
                  indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(digests)} cases to {path}")
