"""CPU-side checks of AgentTD3's / AgentDDPG's one-launch rollout / evaluation entry points (csrc/sac.hip erl_td3_rollout_*, erl_td3_eval_*,
erl_td3_explore_action_tile_f32, erl_td3_rollout_supported; csrc/sac_fused.hip sac_rollout_synenv_kernel<.., DET>, det_actor_tile_kernel):
the eight symbols in the header, the binding and the library with the ABI still 23, the shape query at the class's edges, argument
validation before any launch, and the agents' switch and reasons (no GPU)."""
import ctypes
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEMS = ("synenv", "pendulum", "pointchasing")
ROLLOUTS = tuple(f"erl_td3_rollout_{s}_f32" for s in STEMS)
EVALS = tuple(f"erl_td3_eval_{s}_f32" for s in STEMS)
TILE = "erl_td3_explore_action_tile_f32"
SUPPORTED = "erl_td3_rollout_supported"
NAMES = (SUPPORTED, TILE) + ROLLOUTS + EVALS


def test_the_eight_symbols_and_abi_23():
    from elegantrl_amd import _hip
    txt = open(os.path.join(ROOT, "include", "erl_hip.h")).read()
    assert int(re.search(r"#define ERL_ABI_VERSION (\d+)", txt).group(1)) == _hip.ABI_VERSION == _hip.lib().erl_abi_version() == 23
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert len(NAMES) == 8
    for name in NAMES:
        assert name in _hip.EXPORTED_SYMBOLS and re.search(r"ERL_API int " + name + r"\(", txt), name
        assert hasattr(raw, name) and getattr(_hip.lib(), name).restype is ctypes.c_int, name
    # the argument lists: the erl_sac_* twins', the rollouts with `float action_std` in front of the stream
    for stem in STEMS:
        twin = _hip._SIGNATURES[f"erl_sac_rollout_{stem}_f32"][1]
        assert _hip._SIGNATURES[f"erl_td3_rollout_{stem}_f32"] == (ctypes.c_int, twin[:-1] + [ctypes.c_float, ctypes.c_void_p]), stem
        assert _hip._SIGNATURES[f"erl_td3_eval_{stem}_f32"] == _hip._SIGNATURES[f"erl_sac_eval_{stem}_f32"], stem
        assert re.search(r"erl_td3_rollout_" + stem + r"_f32\([^;]*float \*out_last_state,\s*float action_std,\s*void \*stream\);", txt), stem
    assert _hip._SIGNATURES[TILE] == _hip._SIGNATURES["erl_td3_explore_action_f32"]
    assert _hip._SIGNATURES[SUPPORTED] == _hip._SIGNATURES["erl_sac_rollout_synenv_supported"]


def _hid(*h):
    return (ctypes.c_int * len(h))(*h), len(h)


# (S, A, hidden, N, supported): the edges of the class
EDGE_CASES = ((11, 3, (16, 16), 64, 1),                                    # h = 16
              (11, 3, (256, 256), 64, 1),                                  # h = 256
              (11, 3, (272, 256), 64, 0), (11, 3, (256, 272), 64, 0),      # h = 272
              (11, 3, (24, 64), 64, 0), (11, 3, (64, 24), 64, 0),          # h = 24: no step of 16
              (11, 3, (64,), 64, 0),                                       # one hidden layer
              (11, 3, (64, 48, 32), 64, 0),                                # three
              (56, 8, (64, 48), 64, 1),                                    # A = 8 (S + A = 64)
              (55, 9, (64, 48), 64, 0),                                    # A = 9
              (64, 1, (64, 48), 64, 0),                                    # S = 64: S + A > 64
              (63, 1, (64, 48), 64, 1),
              (11, 3, (64, 48), 4096, 1),                                  # N = 4096
              (11, 3, (64, 48), 4097, 0),                                  # N = 4097
              (11, 3, (64, 48), 0, 0))                                     # N = 0


@pytest.mark.parametrize("S,A,hid,N,want", EDGE_CASES)
def test_supported_truth_table_at_the_edges(S, A, hid, N, want):
    from elegantrl_amd import _hip, ops
    assert _hip.lib().erl_td3_rollout_supported(S, A, *_hid(*hid), N) == want
    assert _hip.lib().erl_sac_rollout_synenv_supported(S, A, *_hid(*hid), N) == want         # the class of the SAC launches
    assert ops.td3_rollout_supported(ops.Td3Spec(S, A, list(hid), 2), N) == bool(want)


def test_erl_sac_fused_0_turns_the_class_off():
    """the library reads ERL_SAC_FUSED once per process: asked of a fresh one"""
    import subprocess
    import sys
    code = ("import ctypes; from elegantrl_amd import _hip; h = (ctypes.c_int * 2)(64, 48); "
            "print(_hip.lib().erl_td3_rollout_supported(11, 3, h, 2, 64))")
    for value, want in (("0", "0"), ("1", "1")):
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, ERL_SAC_FUSED=value), capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == want, (value, out.stdout, out.stderr)


S, A, N, H = 11, 3, 64, 8


def _calls(p, hid=(64, 32), H_=H, max_step=5, ws_bytes=1 << 40, std=0.05, N_=N, S_=S, A_=A):
    """argument lists of the seven launching entries with `p` for every tensor"""
    h, nh = _hid(*hid)
    tail = [None, 1, 0, 1.0, p, p, p, p, p, p, std, None]      # noise, seed, counter0, reward_scale, five outputs, last_state, action_std, stream
    pS, pA = 4 * min(A_, 4), min(A_, 4)                        # PointChasing: S = 4 A, A in 1..4
    if (S_, A_) != (S, A):
        pS, pA = S_, A_
    return {
        ROLLOUTS[0]: [p, S_, A_, h, nh, p, p, p, p, p, max_step, 0, N_, H_] + tail,
        ROLLOUTS[1]: [p, h, nh, p, p, p, p, max_step, 0, N_, H_] + tail,
        ROLLOUTS[2]: [p, pS, pA, h, nh, p, p, p, p, max_step, 0, N_, H_] + tail,
        EVALS[0]: [p, S_, A_, h, nh, p, p, p, p, p, max_step, 0, N_, H_, p, ws_bytes, None],
        EVALS[1]: [p, h, nh, p, p, p, p, max_step, 0, N_, H_, p, ws_bytes, None],
        EVALS[2]: [p, pS, pA, h, nh, p, p, p, p, max_step, 0, N_, H_, p, ws_bytes, None],
        TILE: [p, S_, A_, h, nh, p, N_, None, 1, 0, std, p, None, None, 0, None],
    }


def test_entry_points_validate_before_any_launch():
    """every refusal comes back as ERL_EINVAL with the entry's OWN name in the error string; nothing is launched (no device here), and
    the dummy non-NULL host address is never dereferenced"""
    from elegantrl_amd import _hip
    L = _hip.lib()
    err = L.erl_last_error_string
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def refused(name, args, *words):
        rc = getattr(L, name)(*args)
        msg = err()
        assert rc == -1 and name.encode() in msg and all(w in msg for w in words), (name, rc, msg)
        assert b"erl_sac_" not in msg, msg                                                               # not the AgentSAC twin's name

    for name in ROLLOUTS + EVALS + (TILE,):
        refused(name, _calls(None)[name], b"NULL")                                                       # NULL tensors
        for hid in ((64,), (64, 48, 32), (64, 24), (272, 64)):                                           # outside the class
            refused(name, _calls(p, hid=hid)[name], b"unsupported dims")
        refused(name, _calls(p, N_=4097)[name], b"unsupported dims")
        refused(name, _calls(p, N_=0)[name], b"unsupported dims")
    for name in ROLLOUTS + EVALS:
        refused(name, _calls(p, H_=0)[name], b"H=0")                                                     # H < 1
        refused(name, _calls(p, H_=-3)[name], b"H=-3")
        refused(name, _calls(p, max_step=0)[name], b"max_step=0")
        a = _calls(p)[name]
        a[3 if "pendulum" in name else 5] = None                                                         # one tensor missing
        refused(name, a, b"NULL")
    for name in (ROLLOUTS[0], EVALS[0], TILE):
        refused(name, _calls(p, S_=57, A_=8, hid=(256, 256))[name], b"unsupported dims")                 # S + A = 65
        refused(name, _calls(p, S_=55, A_=9, hid=(256, 256))[name], b"unsupported dims")                 # A = 9
    for name in (ROLLOUTS[2], EVALS[2]):
        refused(name, _calls(p, S_=12, A_=4)[name], b"bad shape")                                        # PointChasing: S = 4 A
    for name in ROLLOUTS + (TILE,):                                                                      # action_std < 0 or not finite
        for std in (-0.05, math.inf, -math.inf, math.nan):
            refused(name, _calls(p, std=std)[name], b"action_std")
    need = L.erl_eval_workspace_bytes(N, H)
    assert need > 0
    for name in EVALS:                                                                                   # a short workspace
        refused(name, _calls(p, ws_bytes=need - 1)[name], b"workspace")
        refused(name, _calls(p, ws_bytes=0)[name], b"workspace")


AGENTS = ("AgentTD3", "AgentDDPG")


def _agent(name, net, on=None, fused_rollout=None, num_envs=64, **extra):
    from elegantrl_amd import agents
    from elegantrl_amd.train import Config
    cls = getattr(agents, name)
    args = Config(cls, None, {"env_name": "x", "num_envs": num_envs, "max_step": 10, "state_dim": 11, "action_dim": 3, "if_discrete": False})
    args.net_dims, args.quiet, args.batch_size = list(net), True, 64
    if on is not None:
        args.fused_td3_rollout = on
    if fused_rollout is not None:
        args.fused_rollout = fused_rollout
    for k, v in extra.items():
        setattr(args, k, v)
    return cls(args.net_dims, 11, 3, gpu_id=-1, args=args)


@pytest.mark.parametrize("name", AGENTS)
def test_the_switch_and_the_agents_reasons(name, monkeypatch):
    """built without a device: the switch off / on / unset, args over the environment variable, shapes the launch does not cover"""
    monkeypatch.delenv("ERL_FUSED_TD3_ROLLOUT", raising=False)
    monkeypatch.delenv("ERL_SAC_FUSED", raising=False)
    from elegantrl_amd.agents import AgentTD3
    assert AgentTD3._fused_td3_rollout_default == "0"                          # ships off
    default, off, on = _agent(name, (256, 256)), _agent(name, (256, 256), False), _agent(name, (256, 256), True)
    assert default.fused_td3_rollout is False and off.fused_td3_rollout is False and on.fused_td3_rollout is True
    assert default.fused_rollout is True
    for a in (default, off):                                                   # off: nothing changes, and the reason names the switch
        assert "fused_td3_rollout is off" in a._one_launch_agent_reason() and "ERL_FUSED_TD3_ROLLOUT" in a._one_launch_agent_reason()
        assert "fused_td3_rollout is off" in a._tile_action_reason(64)
        assert a.kernel_path.startswith("layered TD3 step") and "rollout" not in a.kernel_path
        assert "out of scope for AgentTD3" not in a._loop_path(64, "env.step_into", a._one_launch_agent_reason())
        assert a._loop_path(64, "env.step_into", a._one_launch_agent_reason()).startswith("per-step loop (erl_td3_explore_action_f32")
    assert on._one_launch_agent_reason() is None and on._tile_action_reason(64) is None
    assert "rollout: one launch" in on.kernel_path and "erl_td3_rollout_" in on.kernel_path and "erl_td3_explore_action_tile_f32" in on.kernel_path
    assert on.rollout_path is None                                             # set by _explore_vec_env
    # fused_rollout off keeps the loop (the tile action stays: it is the loop's action)
    a = _agent(name, (256, 256), True, fused_rollout=False)
    assert "fused_rollout is off" in a._one_launch_agent_reason() and a._tile_action_reason(64) is None
    assert a._loop_path(64, "env.step_into", a._one_launch_agent_reason()).startswith(
        "per-step loop (tile action erl_td3_explore_action_tile_f32 + env.step_into per step): args.fused_rollout is off")
    # without a device the pairing rule answers first
    assert on._one_launch_reason(object(), "fused_rollout_offpolicy") == "no GPU" == on._fused_eval_reason(object())
    # shapes: one and three hidden layers and widths outside the class keep the loop and the layered action; the reason names the shape
    for net in ((64,), (64, 48, 32), (100, 100)):
        a = _agent(name, net, True)
        why = a._one_launch_agent_reason()
        assert why is not None and str(list(net)) in why and "outside" in why, why
        assert a._tile_action_reason(64) is not None and str(list(net)) in a._tile_action_reason(64)
        assert "rollout: per-step loop" in a.kernel_path
        assert a._loop_path(64, "env.step", why).startswith("per-step loop (erl_td3_explore_action_f32")
    assert "outside" in _agent(name, (256, 256), True, num_envs=4097)._one_launch_agent_reason()
    assert on._tile_action_reason(4097) is not None                            # asked per call: the rows of this call
    # the switch is read per call
    on.fused_td3_rollout = False
    assert "fused_td3_rollout is off" in on._one_launch_agent_reason()
    on.fused_td3_rollout = True
    # the environment variable, and args over it
    monkeypatch.setenv("ERL_FUSED_TD3_ROLLOUT", "1")
    assert _agent(name, (64, 32)).fused_td3_rollout is True and _agent(name, (64, 32))._one_launch_agent_reason() is None
    assert _agent(name, (64, 32), False).fused_td3_rollout is False            # args wins over the environment
    monkeypatch.setenv("ERL_FUSED_TD3_ROLLOUT", "0")
    assert _agent(name, (64, 32)).fused_td3_rollout is False
    a = _agent(name, (64, 32), True)
    assert a.fused_td3_rollout is True and a._one_launch_agent_reason() is None


def test_the_std_of_the_launch_is_the_agents_own():
    """AgentTD3 reads args.explore_noise_std, AgentDDPG args.explore_noise (the reference's spellings); _sac_call hands that to the entry"""
    assert _agent("AgentTD3", (64, 32), True, explore_noise_std=0.25).explore_noise_std == 0.25
    assert _agent("AgentDDPG", (64, 32), True, explore_noise=0.125).explore_noise_std == 0.125
    from elegantrl_amd import ops
    assert ops.Td3Spec(11, 3, [64, 32], 2).rollout_family == "td3" and not hasattr(ops.SacSpec(11, 3, [64, 32], 2), "rollout_family")


def test_the_new_public_methods_are_wrapped_once():
    from elegantrl_amd.agents import AgentDDPG, AgentTD3
    for cls in (AgentTD3, AgentDDPG):
        for meth in ("evaluate_env", "explore_action", "_explore_vec_env"):
            f = getattr(cls, meth)
            assert hasattr(f, "__wrapped__") and not hasattr(f.__wrapped__, "__wrapped__"), (cls.__name__, meth)


def test_the_clip_case_holds_what_it_is_meant_to():
    """tests/test_td3_rollout_gpu.py's clip case, decided by its reference formula alone, on the CPU: at least 10 % of the elements on the
    clip (0.562 of 500), every one of them outside [-1, 1] before the clip, none within 1e-3 of the clip's edge (an fp32 sum there could
    land on the other side), none within 0.1 of zero"""
    import numpy as np
    from tests.test_td3_rollout_gpu import _clip_case
    eps, want, raw = _clip_case()
    on_clip = np.abs(want) == 1.0
    assert eps.dtype == np.float32 and on_clip.mean() >= 0.10 and (~on_clip).mean() >= 0.10
    assert (np.abs(raw[on_clip]) > 1.0).all() and np.abs(np.abs(raw) - 1.0).min() > 1e-3 and np.abs(raw).min() >= 0.1
    assert (want[on_clip] > 0).any() and (want[on_clip] < 0).any()
