"""Record what tests/test_offpolicy_routes_gpu.py::test_update_net_matches_parent_digests and tests/test_offpolicy_ckpt_cpu.py compare
against: tests/golden/offpolicy_update_digests.json (digests of everything `update_net` leaves on the cases of the former) and
tests/golden/offpolicy_ckpt_parent/ (checkpoints of stamped agents for the latter).

Run it from a checkout of the commit whose bits are the reference (the parent of a change to the off-policy agents, their ops wrappers or
their steps), with this file and the two test modules of the change copied over that checkout -- never from the tree under test:

    python tools/record_offpolicy_digests.py digests [PATH]         (needs a GPU)
    python tools/record_offpolicy_digests.py checkpoints [DIR]      (on the CPU)

The cases and the runs come from the test modules, so the recording and the tests cannot drift."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "checkpoints":
        from tests import test_offpolicy_ckpt_cpu as C
        root = sys.argv[2] if len(sys.argv) > 2 else C.GOLDEN
        C.record(root)
        print(f"recorded {len(C.KINDS)} checkpoints under {root}")
    elif what == "digests":
        from tests import test_offpolicy_routes_gpu as T
        digests = {}
        for name in T.CASES:
            digests[name] = T.run_case(name)
            assert digests[name] == T.run_case(name), f"{name}: update_net is not deterministic from call to call"
            print(name, digests[name]["first"]["update_path"], digests[name]["first"]["per_path"], flush=True)
        path = sys.argv[2] if len(sys.argv) > 2 else T.DIGESTS
        with open(path, "w") as f:
            json.dump({"what": "per case and stage, the first 20 hex digits of SHA-256 of the raw bytes of every flat block, moment pair, "
                               "objs_all, the returned pair, ids0 / ids1 and the CUDA generator's state; counters and paths as repr",
                       "digests": digests}, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"recorded {len(digests)} cases to {path}")
    else:
        sys.exit(__doc__)
