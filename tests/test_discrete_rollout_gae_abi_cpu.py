"""CPU-side checks of the GAE_ form of the one-launch discrete rollout (csrc/rollout_discrete.hip): the four new symbols in the header,
the binding and the library at ABI 22, the two host-only queries, and argument validation before any launch (no GPU)."""
import ctypes
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("erl_rollout_discrete_gae_partials", "erl_rollout_discrete_gae_workspace_bytes", "erl_rollout_discrete_cartpole_gae_f32",
         "erl_rollout_discrete_acrobot_gae_f32")
NEW_POINTERS = ("critic_params", "cri_avg", "cri_std", "out_values", "out_next_value", "out_advantages", "out_reward_sums", "gae_partials")
UNSUPPORTED_NETS = ((100, 32), (256, 64), (64, 160), (16, 32))


def test_abi_is_still_22_with_the_four_symbols():
    from elegantrl_amd import _hip
    txt = open(os.path.join(ROOT, "include", "erl_hip.h")).read()
    assert int(re.search(r"#define ERL_ABI_VERSION (\d+)", txt).group(1)) == _hip.ABI_VERSION == _hip.lib().erl_abi_version() == 23
    for name in NAMES:
        proto = re.search(r"ERL_API (?:int|int64_t) " + name + r"\(([^;]*)\);", txt)
        assert proto is not None and name in _hip.EXPORTED_SYMBOLS, name
        assert getattr(_hip.lib(), name) is not None
        assert len(proto.group(1).split(",")) == len(_hip._SIGNATURES[name][1]), name       # the header's parameter count is the binding's
    # the new entries take the old ones' arguments and twelve more
    for env in ("cartpole", "acrobot"):
        old, new = (_hip._SIGNATURES[f"erl_rollout_discrete_{env}{s}_f32"][1] for s in ("", "_gae"))
        assert len(new) == len(old) + 12 and new[:len(old) - 1] == old[:-1] and new[-1] == old[-1]


def test_the_host_only_queries():
    from elegantrl_amd import _hip
    L = _hip.lib()
    for n in (1, 16, 17, 4100):
        assert L.erl_rollout_discrete_gae_partials(n) == math.ceil(n / 16)
        assert L.erl_rollout_discrete_gae_workspace_bytes(n) == 24 * math.ceil(n / 16)
    for n in (0, -1, -4100):
        assert L.erl_rollout_discrete_gae_workspace_bytes(n) == -1
        assert L.erl_rollout_discrete_gae_partials(n) == -1


def _calls():
    """the two entry points as f(dims, new_pointers, partials_bytes, N=64, max_step=5) on dummy host addresses: never dereferenced,
    nothing is launched"""
    from elegantrl_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)

    def cartpole(dims, new, nbytes, N=64, max_step=5):
        return L.erl_rollout_discrete_cartpole_gae_f32(p, p, p, *dims, p, p, p, max_step, 0, N, 8, None, 0, 0, 1.0, p, p, p, p, p, p, None,
                                                       None, *new, nbytes, 0.99, 0.95, 1, None)

    def acrobot(dims, new, nbytes, N=64, max_step=5):
        return L.erl_rollout_discrete_acrobot_gae_f32(p, p, p, *dims, p, p, p, p, max_step, 0, N, 8, None, 0, 0, 1.0, p, p, p, p, p, p, None,
                                                      None, *new, nbytes, 0.99, 0.95, 1, None)
    return L, p, ((b"erl_rollout_discrete_cartpole_gae_f32", cartpole, (4, 64, 32, 2)),
                  (b"erl_rollout_discrete_acrobot_gae_f32", acrobot, (6, 64, 32, 3)))


def test_entry_points_validate_before_any_launch():
    L, p, entries = _calls()
    err = L.erl_last_error_string
    need = L.erl_rollout_discrete_gae_workspace_bytes(64)
    assert need == 96
    for what, call, dims in entries:
        # every new pointer is required, and the message names it
        for i, name in enumerate(NEW_POINTERS):
            new = [p] * 8
            new[i] = None
            assert call(dims, new, need) == -1
            assert what in err() and b"NULL" in err() and name.encode() in err(), (name, err())
        # an old one still is
        assert L.erl_rollout_discrete_cartpole_gae_f32(None, p, p, 4, 64, 32, 2, p, p, p, 5, 0, 64, 8, None, 0, 0, 1.0, p, p, p, p, p, p, None,
                                                       None, *([p] * 8), need, 0.99, 0.95, 1, None) == -1 and b"NULL" in err()
        # a short workspace: both sizes are named
        assert call(dims, [p] * 8, need - 1) == -1
        assert what in err() and str(need - 1).encode() in err() and str(need).encode() in err(), err()
        assert call(dims, [p] * 8, 0) == -1 and what in err()
        # unsupported nets, whatever the pointers are
        for h1, h2 in UNSUPPORTED_NETS:
            assert call((dims[0], h1, h2, dims[3]), [p] * 8, need) == -1
            assert what in err() and b"unsupported dims" in err(), (h1, h2, err())
        # bad shapes
        assert call(dims, [p] * 8, need, N=0) == -1 and what in err() and b"bad shape" in err()
        assert call(dims, [p] * 8, need, max_step=0) == -1 and what in err() and b"bad shape" in err()
    (wc, cartpole, _), (wa, acrobot, _) = entries
    # a policy shape the kernel has on an env whose dims are others
    assert cartpole((6, 64, 32, 2), [p] * 8, need) == -1 and wc in err() and b"state_dim is 4" in err()
    assert acrobot((4, 64, 32, 3), [p] * 8, need) == -1 and wa in err() and b"state_dim is 6" in err()
    assert acrobot((6, 64, 32, 2), [p] * 8, need) == -1 and wa in err() and b"action_dim is 3" in err()


def test_the_switch_and_the_kernel_path_text(monkeypatch):
    """built without a device: off by default, not reached by the continuous agents' ERL_FUSED_GAE, on by args or its own variable"""
    from elegantrl_amd.agents import AgentDiscretePPO
    from elegantrl_amd.train import Config

    def agent(**kw):
        args = Config(AgentDiscretePPO, None, {"env_name": "CartPole-v1", "num_envs": 8, "max_step": 10, "state_dim": 4, "action_dim": 2,
                                               "if_discrete": True})
        args.net_dims, args.quiet, args.fused_rollout = [64, 32], True, True
        for k, v in kw.items():
            setattr(args, k, v)
        return AgentDiscretePPO(args.net_dims, 4, 2, gpu_id=-1, args=args)
    monkeypatch.delenv("ERL_FUSED_DISCRETE_GAE", raising=False)
    monkeypatch.delenv("ERL_FUSED_GAE", raising=False)
    a = agent()
    assert a.fused_gae is False and a.advantage_path is None and "advantages: value pre-pass + scan" in a.kernel_path
    monkeypatch.setenv("ERL_FUSED_GAE", "1")
    assert agent().fused_gae is False
    a = agent(fused_gae=True)
    assert a.fused_gae is True and "inside the one-launch rollout" in a.kernel_path
    assert "needs the one-launch rollout" in agent(fused_gae=True, fused_rollout=False).kernel_path
    monkeypatch.setenv("ERL_FUSED_DISCRETE_GAE", "1")
    assert agent().fused_gae is True and agent(fused_gae=False).fused_gae is False
