"""The refusals of the fourteen C entries of the continuous device envs (csrc/rollout_fused.hip, rollout_eval.hip, sac.hip, envs.hip),
replayed from tests/golden/continuous_entry_refusals.json: every recorded call is refused with the recorded code and the recorded text.
The JSON was recorded by tools/record_continuous_entry_refusals.py from the library as it was before the entries' host bodies were merged,
never from the code under test: a failing case means a refusal changed (its text, or which of two faults is named first).  No GPU: a
refusal comes before any launch and no pointer is dereferenced."""
import collections
import ctypes
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "continuous_entry_refusals.json")
with open(GOLDEN) as f:
    CASES = json.load(f)
BY_ENTRY = collections.defaultdict(list)
for c in CASES:
    BY_ENTRY[c["entry"]].append(c)

ENTRIES = ([f"erl_{form}_{env}_f32" for form in ("rollout", "eval") for env in ("synenv", "pendulum")] +
           [f"erl_sac_{form}_{mod}{env}_f32" for form in ("rollout", "eval") for mod in ("", "mod_") for env in ("synenv", "pendulum")] +
           ["erl_synenv_step_f32", "erl_pendulum_step_f32"])


def test_the_golden_file_covers_the_fourteen_entries():
    assert sorted(BY_ENTRY) == sorted(ENTRIES)
    assert all(c["rc"] == -1 and c["error"].startswith(c["entry"] + ": ") for c in CASES)
    assert all(len({json.dumps(c["args"]) for c in cs}) == len(cs) for cs in BY_ENTRY.values())      # no call twice


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_refuses_what_it_refused_with_the_same_text(entry):
    from elegantrl_amd import _hip
    L = _hip.lib()
    buf = ctypes.create_string_buffer(4096)          # dummy non-NULL host address: never dereferenced, nothing is launched
    for c in BY_ENTRY[entry]:
        keep = [(ctypes.c_int * len(a["ints"]))(*a["ints"]) for a in c["args"] if isinstance(a, dict)]
        arrays = iter(keep)
        args = [ctypes.addressof(buf) if a == "P" else next(arrays) if isinstance(a, dict) else a for a in c["args"]]
        rc = getattr(L, entry)(*args)
        got = (rc, (L.erl_last_error_string() or b"").decode())
        assert got == (c["rc"], c["error"]), (entry, c["case"])
