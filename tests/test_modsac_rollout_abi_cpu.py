"""CPU-side checks of AgentModSAC's one-launch rollout / evaluation entry points (csrc/sac.hip erl_sac_rollout_mod_*, erl_sac_eval_mod_*,
erl_sac_explore_action_tile_f32; csrc/sac_fused.hip sac_rollout_synenv_kernel<.., FIX>): the six symbols in the header, the binding and the
library with the ABI still 22, the shape query at its limits, argument validation before any launch, and the agent's switch and reasons
(no GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLLOUTS = ("erl_sac_rollout_mod_synenv_f32", "erl_sac_rollout_mod_pendulum_f32")
EVALS = ("erl_sac_eval_mod_synenv_f32", "erl_sac_eval_mod_pendulum_f32")
TILE = "erl_sac_explore_action_tile_f32"
NAMES = ("erl_sac_rollout_mod_supported",) + ROLLOUTS + EVALS + (TILE,)


def test_the_six_symbols_and_abi_22():
    from elegantrl_amd import _hip
    txt = open(os.path.join(ROOT, "include", "erl_hip.h")).read()
    assert int(re.search(r"#define ERL_ABI_VERSION (\d+)", txt).group(1)) == _hip.ABI_VERSION == _hip.lib().erl_abi_version() == 23
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert len(NAMES) == 6
    for name in NAMES:
        assert name in _hip.EXPORTED_SYMBOLS and re.search(r"ERL_API int " + name + r"\(", txt), name
        assert hasattr(raw, name) and getattr(_hip.lib(), name) is not None
    # the twins keep their argument lists
    for mod in ROLLOUTS + EVALS:
        twin = mod.replace("_mod_", "_")
        assert _hip._SIGNATURES[mod] == _hip._SIGNATURES[twin], mod
    assert _hip._SIGNATURES[TILE] == _hip._SIGNATURES["erl_sac_explore_action_opt_f32"]
    assert _hip._SIGNATURES["erl_sac_rollout_mod_supported"] == _hip._SIGNATURES["erl_sac_rollout_synenv_supported"]


def _hid(*h):
    return (ctypes.c_int * len(h))(*h), len(h)


LIMIT_CASES = ((56, 8, (256, 256), 4096, 1), (1, 1, (16, 16), 1, 1), (3, 1, (128, 64), 50, 1),
               (56, 8, (256,), 4096, 0),                                   # one hidden layer
               (56, 8, (256, 256, 256), 4096, 0),                          # three
               (56, 8, (272, 256), 4096, 0), (56, 8, (256, 272), 4096, 0),  # width 272
               (56, 8, (24, 256), 4096, 0),                                # no step of 16
               (57, 8, (256, 256), 4096, 0),                               # S + A = 65
               (55, 9, (256, 256), 4096, 0),                               # A = 9
               (56, 8, (256, 256), 0, 0), (56, 8, (256, 256), 4097, 0))    # N of 0 / 4097


def test_supported_answers_at_the_limits():
    from elegantrl_amd import _hip, ops
    sup, twin = _hip.lib().erl_sac_rollout_mod_supported, _hip.lib().erl_sac_rollout_synenv_supported
    for S, A, hid, N, want in LIMIT_CASES:
        assert sup(S, A, *_hid(*hid), N) == want == twin(S, A, *_hid(*hid), N), (S, A, hid, N)
    assert ops.sac_rollout_mod_supported(ops.SacSpec(56, 8, [256, 256], 8, actor_variant=_hip.SAC_ACTOR_FIX), 4096)
    assert not ops.sac_rollout_mod_supported(ops.SacSpec(11, 3, [64], 8, actor_variant=_hip.SAC_ACTOR_FIX), 64)


S, A, N, H = 11, 3, 64, 8


def _calls(p, hid=(64, 32), H_=H, max_step=5, ws_bytes=1 << 40, variant=1, N_=N, S_=S, A_=A):
    """argument lists of the five entries with `p` for every tensor"""
    h, nh = _hid(*hid)
    tail = [None, 1, 0, 1.0, p, p, p, p, p, p, None]          # noise, seed, counter0, reward_scale, five outputs, last_state, stream
    return {
        ROLLOUTS[0]: [p, S_, A_, h, nh, p, p, p, p, p, max_step, 0, N_, H_] + tail,
        ROLLOUTS[1]: [p, h, nh, p, p, p, p, max_step, 0, N_, H_] + tail,
        EVALS[0]: [p, S_, A_, h, nh, p, p, p, p, p, max_step, 0, N_, H_, p, ws_bytes, None],
        EVALS[1]: [p, h, nh, p, p, p, p, max_step, 0, N_, H_, p, ws_bytes, None],
        TILE: [p, S_, A_, h, nh, p, N_, None, 1, 0, p, None, p, ws_bytes, variant, None],
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
        twin = name.replace("_mod_", "_").encode()
        assert name == TILE or twin not in msg.replace(name.encode(), b""), msg        # not the AgentSAC twin's name

    for name in ROLLOUTS + EVALS + (TILE,):
        refused(name, _calls(None)[name], b"NULL")                                                       # NULL tensors
        for hid in ((64,), (64, 48, 32), (64, 24), (272, 64)):                                           # outside the shapes
            refused(name, _calls(p, hid=hid)[name])
        refused(name, _calls(p, N_=4097)[name])
        refused(name, _calls(p, N_=0)[name])
    for name in ROLLOUTS + EVALS:
        refused(name, _calls(p, H_=0)[name], b"H=0")                                                     # H = 0
        refused(name, _calls(p, max_step=0)[name], b"max_step=0")                                        # max_step = 0
        a = _calls(p)[name]
        a[3 if "pendulum" in name else 5] = None                                                         # one tensor missing
        refused(name, a, b"NULL")
    refused(ROLLOUTS[0], _calls(p, S_=57, A_=8, hid=(256, 256))[ROLLOUTS[0]], b"unsupported dims")       # S + A = 65
    refused(EVALS[0], _calls(p, S_=55, A_=9, hid=(256, 256))[EVALS[0]], b"unsupported dims")             # A = 9
    need = L.erl_eval_workspace_bytes(N, H)
    assert need > 0
    for name in EVALS:                                                                                   # a short workspace
        refused(name, _calls(p, ws_bytes=need - 1)[name], b"workspace")
    refused(TILE, _calls(p, ws_bytes=0)[TILE], b"workspace")
    refused(TILE, _calls(p, ws_bytes=N * 4 - 1)[TILE], b"workspace")
    for variant in (2, -1):                                                                              # an unknown variant
        refused(TILE, _calls(p, variant=variant)[TILE], b"actor_variant")
    refused(TILE, _calls(p, S_=57, A_=8, hid=(256, 256))[TILE], b"outside the tile kernel's shapes")


def _agent(net, mod=None, fused_rollout=None, num_envs=64):
    from elegantrl_amd.agents import AgentModSAC
    from elegantrl_amd.train import Config
    args = Config(AgentModSAC, None, {"env_name": "x", "num_envs": num_envs, "max_step": 10, "state_dim": 11, "action_dim": 3, "if_discrete": False})
    args.net_dims, args.quiet, args.batch_size = list(net), True, 64
    if mod is not None:
        args.fused_mod_rollout = mod
    if fused_rollout is not None:
        args.fused_rollout = fused_rollout
    return AgentModSAC(args.net_dims, 11, 3, gpu_id=-1, args=args)


def test_the_switch_and_the_agents_reasons(monkeypatch):
    """built without a device: the switch off / on / unset, args over the environment variable, shapes the launch does not cover"""
    monkeypatch.delenv("ERL_FUSED_MODSAC_ROLLOUT", raising=False)
    monkeypatch.delenv("ERL_SAC_FUSED", raising=False)
    from elegantrl_amd.agents import AgentModSAC, AgentSAC
    assert AgentModSAC._fused_mod_rollout_default == "0"                       # ships off
    default, off, on = _agent((256, 256)), _agent((256, 256), False), _agent((256, 256), True)
    assert default.fused_mod_rollout is False and off.fused_mod_rollout is False and on.fused_mod_rollout is True
    for a in (default, off):                                                   # off: nothing changes, and the reason names the actor
        assert "ActorFixSAC" in a._one_launch_agent_reason()
        assert a._tile_action_reason(64) is not None
        assert "rollout: per-step loop" in a.kernel_path and "ActorFixSAC" in a.kernel_path
    assert on._one_launch_agent_reason() is None and on._tile_action_reason(64) is None
    assert "rollout: one launch" in on.kernel_path and "erl_sac_rollout_mod_" in on.kernel_path and "erl_sac_explore_action_tile_f32" in on.kernel_path
    assert on.rollout_path is None                                             # set by _explore_vec_env
    # fused_rollout off keeps the loop (the tile action stays: it is the loop's action)
    a = _agent((256, 256), True, fused_rollout=False)
    assert "fused_rollout is off" in a._one_launch_agent_reason() and a._tile_action_reason(64) is None
    # without a device the pairing rule answers first
    assert on._one_launch_reason(object(), "fused_rollout_offpolicy") == "no GPU"
    # shapes: one and three hidden layers keep the loop and the layered action, with a reason that names the shape
    for net in ((64,), (64, 48, 32)):
        a = _agent(net, True)
        why = a._one_launch_agent_reason()
        assert why is not None and "ActorFixSAC" not in why and str(list(net)) in why and "outside" in why, why
        assert a._tile_action_reason(64) is not None and str(list(net)) in a._tile_action_reason(64)
        assert "rollout: per-step loop" in a.kernel_path
    assert "outside" in _agent((256, 256), True, num_envs=4097)._one_launch_agent_reason()
    assert on._tile_action_reason(4097) is not None                            # asked per call: the rows of this call
    # the switch is read per call
    on.fused_mod_rollout = False
    assert "ActorFixSAC" in on._one_launch_agent_reason()
    on.fused_mod_rollout = True
    # the environment variable, and args over it
    monkeypatch.setenv("ERL_FUSED_MODSAC_ROLLOUT", "1")
    assert _agent((64, 32)).fused_mod_rollout is True and _agent((64, 32))._one_launch_agent_reason() is None
    assert _agent((64, 32), False).fused_mod_rollout is False                  # args wins over the environment
    monkeypatch.setenv("ERL_FUSED_MODSAC_ROLLOUT", "0")
    assert _agent((64, 32)).fused_mod_rollout is False
    a = _agent((64, 32), True)
    assert a.fused_mod_rollout is True and a._one_launch_agent_reason() is None
    # AgentSAC is as it was
    from elegantrl_amd.train import Config
    args = Config(AgentSAC, None, {"env_name": "x", "num_envs": 64, "max_step": 10, "state_dim": 11, "action_dim": 3, "if_discrete": False})
    args.net_dims, args.quiet = [64, 32], True
    sac = AgentSAC(args.net_dims, 11, 3, gpu_id=-1, args=args)
    assert sac._one_launch_agent_reason() is None and sac._tile_action_reason(64) is not None and sac.rollout_path is None
