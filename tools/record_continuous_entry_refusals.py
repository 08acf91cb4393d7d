#!/usr/bin/env python3
"""Records what the fourteen C entries of the continuous device envs answer to calls they must refuse: erl_rollout_{synenv,pendulum}_f32,
erl_eval_{synenv,pendulum}_f32, erl_sac_{rollout,eval}_{,mod_}{synenv,pendulum}_f32, erl_synenv_step_f32 and erl_pendulum_step_f32.

    python tools/record_continuous_entry_refusals.py [lib] > tests/golden/continuous_entry_refusals.json

Per entry a fixed list of refused calls: every pointer NULL, dummy non-NULL host addresses with one thing wrong, and two things wrong at
once (which of the two the entry names is its precedence).  Recorded per case: the arguments, the return code and
erl_last_error_string().  A refusal comes before any launch and no pointer is dereferenced, so this needs no GPU.  The recorder stops if
an entry does not refuse a case with rc == -1: a call that passes validation has no place in the list.

tests/golden/continuous_entry_refusals.json was recorded from the library as it was BEFORE the entries' host bodies were merged (one env
pack, one body per launch form), never from the code under test: tests/test_continuous_entries_abi_cpu.py replays it against the built
library and asks for the same code and the same text.  A case that fails there means a refusal changed: fix the code, not the JSON.

Arguments in the JSON: "P" is a dummy non-NULL host address, null is NULL, {"ints": [..]} is an int array (`hidden`), numbers are
themselves."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NET6 = ["actor_params", "critic_params", "act_avg", "act_std", "cri_avg", "cri_std"]
NET3 = ["actor_params", "act_avg", "act_std"]
SYN = ["env_state", "Ws", "Wa", "step_count", "episode"]
PEN = ["phys", "obs", "step_count", "episode"]
PLANES8 = ["out_states", "out_actions", "out_logprobs", "out_rewards", "out_undones", "out_unmasks", "out_values", "out_next_value"]
PLANES6 = PLANES8[:6]
EPILOGUE = ["out_last_state", "out_advantages", "out_reward_sums", "gae_stats", "gae_workspace"]
SAC_PLANES = ["out_states", "out_actions", "out_rewards", "out_undones", "out_unmasks", "out_last_state"]
N, H = 64, 8
GAE_WS = 3 * ((N + 15) // 16) * 8                              # erl_rollout_gae_workspace_bytes(N)
EVAL_WS = (N * H * 8 + N * 4 + 255) // 256 * 256               # erl_eval_workspace_bytes(N, H)
HID = {"ints": [64, 64]}


def ptrs(names):
    return [(n, "P") for n in names]


def ppo_rollout(env, dims):
    return (ptrs(NET6) + dims + ptrs(env) + [("max_step", 5), ("env_seed", 0), ("N", N), ("H", H), ("noise", "P"), ("seed", 1), ("counter0", 2),
            ("reward_scale", 1.0)] + ptrs(PLANES8) + ptrs(EPILOGUE) + [("gae_workspace_bytes", GAE_WS), ("gamma", 0.99), ("lambda_gae", 0.95),
            ("use_v_trace", 1), ("stream", None)])


def ppo_eval(env, dims):
    return (ptrs(NET3) + dims + ptrs(env) + [("max_step", 5), ("env_seed", 0), ("N", N), ("H", H), ("workspace", "P"),
            ("workspace_bytes", EVAL_WS), ("stream", None)])


def sac_rollout(env, dims):
    return ([("actor_params", "P")] + dims + [("hidden", HID), ("n_hidden", 2)] + ptrs(env) + [("max_step", 5), ("env_seed", 0), ("N", N),
            ("H", H), ("noise", "P"), ("seed", 1), ("counter0", 2), ("reward_scale", 1.0)] + ptrs(SAC_PLANES) + [("stream", None)])


def sac_eval(env, dims):
    return ([("actor_params", "P")] + dims + [("hidden", HID), ("n_hidden", 2)] + ptrs(env) + [("max_step", 5), ("env_seed", 0), ("N", N),
            ("H", H), ("workspace", "P"), ("workspace_bytes", EVAL_WS), ("stream", None)])


PPO_DIMS = [("S", 64), ("h1", 128), ("h2", 128), ("A", 8)]
PEN_DIMS = [("h1", 128), ("h2", 64)]
SAC_DIMS = [("S", 17), ("A", 3)]

# a call that would pass validation, per entry (never made: every case below changes it into one that must be refused)
BASE = {
    "erl_rollout_synenv_f32": ppo_rollout(SYN, PPO_DIMS),
    "erl_rollout_pendulum_f32": ppo_rollout(PEN, PEN_DIMS),
    "erl_eval_synenv_f32": ppo_eval(SYN, PPO_DIMS),
    "erl_eval_pendulum_f32": ppo_eval(PEN, PEN_DIMS),
    "erl_synenv_step_f32": ptrs(["state", "action", "Ws", "Wa", "step_count", "episode", "reward", "terminal", "truncate"]) +
                           [("N", N), ("S", 64), ("A", 8), ("max_step", 5), ("seed", 0), ("stream", None)],
    "erl_pendulum_step_f32": ptrs(["phys", "obs", "action", "step_count", "episode", "reward", "terminal", "truncate"]) +
                             [("N", N), ("max_step", 5), ("seed", 0), ("stream", None)],
}
for mod in ("", "mod_"):
    BASE[f"erl_sac_rollout_{mod}synenv_f32"] = sac_rollout(SYN, SAC_DIMS)
    BASE[f"erl_sac_rollout_{mod}pendulum_f32"] = sac_rollout(PEN, [])
    BASE[f"erl_sac_eval_{mod}synenv_f32"] = sac_eval(SYN, SAC_DIMS)
    BASE[f"erl_sac_eval_{mod}pendulum_f32"] = sac_eval(PEN, [])


def null(*names):
    return {n: None for n in names}


def changes_of(entry):
    """[(label, {argument: value})] for one entry; the labels say what is wrong"""
    names = [n for n, _ in BASE[entry]]
    pointers = [n for n, v in BASE[entry] if v == "P"]
    env = [n for n in dict.fromkeys(SYN + PEN) if n in names]
    syn, sac, step = "synenv" in entry, "_sac_" in entry, entry.endswith("_step_f32")
    out = [("every pointer NULL", null(*pointers, *(["hidden"] if sac else [])))]
    out += [(f"{n} NULL", null(n)) for n in env]
    out += [("every env buffer NULL", null(*env))]
    if step:
        out += [(f"{n} NULL", null(n)) for n in pointers if n not in env]
        out += [("N = 0", {"N": 0}), ("N = -1", {"N": -1}), ("action NULL and N = 0", {"action": None, "N": 0})]
        if syn:
            out += [("S = 0", {"S": 0}), ("S = 129", {"S": 129}), ("A = 0", {"A": 0}), ("A = 65", {"A": 65}), ("Ws NULL and S = 129", {"Ws": None, "S": 129})]
        else:
            out += [("max_step = 0", {"max_step": 0}), ("phys NULL and max_step = 0", {"phys": None, "max_step": 0})]
        return out
    out += [("N = 0", {"N": 0}), ("H = 0", {"H": 0}), ("H = 1 << 30", {"H": 1 << 30}), ("max_step = 0", {"max_step": 0}),
            ("N = 0 and max_step = 0", {"N": 0, "max_step": 0}), ("H = 0 and episode NULL", {"H": 0, "episode": None}),
            ("step_count NULL and max_step = 0", {"step_count": None, "max_step": 0})]
    rollout = "rollout" in entry
    if sac:
        out += [("actor_params NULL", null("actor_params")), ("hidden NULL", null("hidden")), ("n_hidden = 3", {"n_hidden": 3}),
                ("n_hidden = 0", {"n_hidden": 0}), ("a hidden width of 100", {"hidden": {"ints": [100, 64]}}),
                ("a hidden width of 272", {"hidden": {"ints": [64, 272]}}), ("N = 4097", {"N": 4097}),
                ("N = 4097 and H = 0", {"N": 4097, "H": 0}), ("actor_params NULL and N = 4097", {"actor_params": None, "N": 4097}),
                ("N = 4097 and max_step = 0", {"N": 4097, "max_step": 0})]
        if syn:
            out += [("S + A = 65", {"S": 57, "A": 8}), ("A = 9", {"A": 9}), ("S = 0", {"S": 0}), ("S = 65", {"S": 65, "A": 1}),
                    ("Ws NULL and A = 9", {"Ws": None, "A": 9}), ("Wa NULL and actor_params NULL", null("Wa", "actor_params")),
                    ("A = 9 and H = 0", {"A": 9, "H": 0})]
        if rollout:
            out += [(f"{n} NULL", null(n)) for n in SAC_PLANES[:5]]
            out += [("every rollout buffer NULL", null(*SAC_PLANES[:5])), ("out_states NULL and N = 4097", {"out_states": None, "N": 4097})]
        else:
            out += [("workspace NULL", null("workspace")), ("workspace one byte short", {"workspace_bytes": EVAL_WS - 1}),
                    ("workspace of 0 bytes", {"workspace_bytes": 0}), ("N * H beyond int32", {"N": 4096, "H": 1 << 29}),
                    ("workspace NULL and N = 4097", {"workspace": None, "N": 4097}),
                    ("workspace one byte short and max_step = 0", {"workspace_bytes": EVAL_WS - 1, "max_step": 0}),
                    ("workspace one byte short and a hidden width of 100", {"workspace_bytes": EVAL_WS - 1, "hidden": {"ints": [100, 64]}})]
        return out
    net = NET6 if rollout else NET3
    out += [(f"{n} NULL", null(n)) for n in net]
    out += [("every network tensor NULL", null(*net)), ("h1 = 100", {"h1": 100}), ("h2 = 160", {"h2": 160}), ("h2 = 0", {"h2": 0}),
            ("h1 = 100 and N = 0", {"h1": 100, "N": 0}), ("act_std NULL and h1 = 100", {"act_std": None, "h1": 100}),
            ("h1 = 100 and step_count NULL", {"h1": 100, "step_count": None}), ("N = 0 and env buffers NULL", {"N": 0, **null(*env)})]
    if syn:
        out += [("S = 65", {"S": 65}), ("S = 0", {"S": 0}), ("A = 17", {"A": 17}), ("A = 0", {"A": 0}), ("S = 65 and H = 0", {"S": 65, "H": 0}),
                ("actor_params NULL and S = 65", {"actor_params": None, "S": 65}), ("S = 65 and Ws NULL", {"S": 65, "Ws": None})]
    if rollout:
        out += [(f"{n} NULL", null(n)) for n in PLANES6]
        out += [("every rollout buffer NULL", null(*PLANES6)), ("out_rewards NULL and h1 = 100", {"out_rewards": None, "h1": 100}),
                ("cri_std NULL and out_states NULL", null("cri_std", "out_states")),
                ("out_advantages without out_reward_sums", null("out_reward_sums")),
                ("out_reward_sums without out_advantages", null("out_advantages")),
                ("the epilogue without gae_workspace", null("gae_workspace")),
                ("the epilogue without out_values", null("out_values")),
                ("the epilogue without out_next_value", null("out_next_value")),
                ("gae_workspace one byte short", {"gae_workspace_bytes": GAE_WS - 1}),
                ("gae_workspace of 0 bytes", {"gae_workspace_bytes": 0}),
                ("gae_workspace one byte short and N = 0", {"gae_workspace_bytes": GAE_WS - 1, "N": 0}),
                ("gae_workspace one byte short and episode NULL", {"gae_workspace_bytes": GAE_WS - 1, "episode": None}),
                ("out_advantages without out_reward_sums and max_step = 0", {"out_reward_sums": None, "max_step": 0}),
                ("out_advantages without out_reward_sums and gae_workspace one byte short", {"out_reward_sums": None, "gae_workspace_bytes": GAE_WS - 1}),
                ("no epilogue and max_step = 0", {**null("out_advantages", "out_reward_sums", "gae_workspace"), "gae_workspace_bytes": 0, "max_step": 0})]
    else:
        out += [("workspace NULL", null("workspace")), ("workspace one byte short", {"workspace_bytes": EVAL_WS - 1}),
                ("workspace of 0 bytes", {"workspace_bytes": 0}), ("N * H beyond int32", {"N": 1 << 20, "H": 1 << 20}),
                ("workspace NULL and act_avg NULL", null("workspace", "act_avg")), ("workspace NULL and h1 = 100", {"workspace": None, "h1": 100}),
                ("workspace one byte short and N = 0", {"workspace_bytes": EVAL_WS - 1, "N": 0}),
                ("workspace one byte short and Ws or phys NULL", {"workspace_bytes": EVAL_WS - 1, env[1 if syn else 0]: None}),
                ("workspace one byte short and max_step = 0", {"workspace_bytes": EVAL_WS - 1, "max_step": 0})]
    return out


def cases():
    """[{"entry", "case", "args"}]: the fixed list, in the order it is replayed"""
    out = []
    for entry, base in BASE.items():
        for label, change in changes_of(entry):
            assert all(k in dict(base) for k in change), (entry, label)
            out.append({"entry": entry, "case": label, "args": [change.get(n, v) for n, v in base]})
    return out


def call(lib, case, keep):
    """one recorded call: (rc, text).  `keep` holds the buffers the arguments point to"""
    buf = ctypes.create_string_buffer(4096)
    keep.append(buf)
    args = []
    for a in case["args"]:
        if a == "P":
            args.append(ctypes.addressof(buf))
        elif isinstance(a, dict):
            keep.append((ctypes.c_int * len(a["ints"]))(*a["ints"]))
            args.append(keep[-1])
        else:
            args.append(a)
    rc = getattr(lib, case["entry"])(*args)
    return rc, (lib.erl_last_error_string() or b"").decode()


def main():
    if len(sys.argv) > 1:
        os.environ["ERL_HIP_LIB"] = os.path.abspath(sys.argv[1])
    sys.path.insert(0, ROOT)
    from elegantrl_amd import _hip
    lib, keep, out = _hip.lib(), [], []
    for c in cases():
        rc, text = call(lib, c, keep)
        if rc != -1:
            sys.exit(f"{c['entry']}: '{c['case']}' is not refused (rc = {rc}): it has no place in the list")
        out.append({**c, "rc": rc, "error": text})
    sys.stdout.write("[\n" + ",\n".join(json.dumps(c) for c in out) + "\n]\n")      # one case per line


if __name__ == "__main__":
    main()
