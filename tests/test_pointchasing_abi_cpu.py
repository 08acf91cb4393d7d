"""CPU-side checks of the PointChasingVecEnv entry points (csrc/envs.hip, rollout_fused.hip, rollout_eval.hip, sac.hip): the seven symbols
in the header and the binding at an unchanged ABI version, the per-step entry's refusals before any launch, and the env class, its aliases
and the reference's import path without a device."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("erl_pointchasing_step_f32", "erl_rollout_pointchasing_f32", "erl_eval_pointchasing_f32", "erl_sac_rollout_pointchasing_f32",
         "erl_sac_rollout_mod_pointchasing_f32", "erl_sac_eval_pointchasing_f32", "erl_sac_eval_mod_pointchasing_f32")
# the SynVecEnv twin takes (env_state, Ws, Wa) where PointChasing takes (state, distance): one pointer more
TWINS = {n: n.replace("pointchasing", "synenv") for n in NAMES}


def test_seven_entries_declared_and_bound_with_equal_argument_counts():
    from elegantrl_amd import _hip
    txt = open(os.path.join(ROOT, "include", "erl_hip.h")).read()
    assert int(re.search(r"#define ERL_ABI_VERSION (\d+)", txt).group(1)) == _hip.ABI_VERSION == _hip.lib().erl_abi_version()
    for name in NAMES:
        assert name in _hip.EXPORTED_SYMBOLS and getattr(_hip.lib(), name) is not None
        proto = re.search(r"ERL_API int " + name + r"\(([^;]*)\);", txt).group(1)
        assert len(proto.split(",")) == len(_hip._SIGNATURES[name][1]), name
        twin = re.search(r"ERL_API int " + TWINS[name] + r"\(([^;]*)\);", txt).group(1)
        assert len(proto.split(",")) == len(twin.split(",")) - 1, name
        assert len(_hip._SIGNATURES[name][1]) == len(_hip._SIGNATURES[TWINS[name]][1]) - 1, name


def test_step_entry_refuses_before_any_launch():
    from elegantrl_amd import _hip
    L = _hip.lib()
    step, err = L.erl_pointchasing_step_f32, L.erl_last_error_string
    rc = step(None, None, None, None, None, None, None, None, 64, 8, 2, 5, 0, None)
    assert rc == -1 and err() == b"erl_pointchasing_step_f32: NULL tensor"
    buf = (ctypes.c_char * 4096)()          # dummy non-NULL host address: never dereferenced, nothing is launched
    p = ctypes.addressof(buf)
    for hole in range(8):                   # one NULL among the eight pointers is enough
        ptrs = [p] * 8
        ptrs[hole] = None
        rc = step(*ptrs, 64, 8, 2, 5, 0, None)
        assert rc == -1 and err() == b"erl_pointchasing_step_f32: NULL tensor", hole
    for n, s, a, ms in ((0, 8, 2, 5), (64, 8, 2, 0), (64, 0, 0, 5), (64, 20, 5, 5), (64, 8, 3, 5), (64, 7, 2, 5), (64, 16, 2, 5), (-1, 4, 1, 5)):
        rc = step(p, p, p, p, p, p, p, p, n, s, a, ms, 0, None)
        assert rc == -1 and err() == b"erl_pointchasing_step_f32: bad shape", (n, s, a, ms)


@pytest.mark.parametrize("name", NAMES[1:])
def test_one_launch_entries_refuse_bad_dims_and_null_buffers(name):
    """dim outside 1..4 or state_dim != 4 dim is "bad shape" whatever else is handed over; a NULL live buffer is named as the twin names it"""
    from elegantrl_amd import _hip
    L = _hip.lib()
    fn, err = getattr(L, name), L.erl_last_error_string
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    hidden = (ctypes.c_int * 2)(64, 64)
    sac, ev = "_sac_" in name, "_eval_" in name

    def call(S, A, distance):
        env = (p, distance, p, p, 5, 0, 64, 8)                                   # state, distance, step_count, episode, max_step, seed, N, H
        head = (p, S, A, hidden, 2) if sac else ((p, p, p) if ev else (p,) * 6) + (S, 64, 64, A)
        if ev:
            tail = (p, 1 << 20, None)
        elif sac:
            tail = (None, 0, 0, 1.0, p, p, p, p, p, None, None)
        else:
            tail = (None, 0, 0, 1.0) + (p,) * 8 + (None,) * 5 + (0, 0.99, 0.95, 0, None)
        return fn(*head, *env, *tail)

    for S, A in ((20, 5), (0, 0), (8, 3), (12, 2)):
        assert call(S, A, p) == -1 and err() == (name + ": bad shape").encode(), (S, A, err())
    assert call(8, 2, None) == -1
    assert err() == (name + (": NULL tensor" if sac else ": bad environment argument")).encode()


def test_env_class_without_a_device():
    from elegantrl_amd.envs import PointChasingVecEnv
    from elegantrl_amd.envs.vec_envs import _ContinuousGpuVecEnv
    assert issubclass(PointChasingVecEnv, _ContinuousGpuVecEnv) and not PointChasingVecEnv.if_discrete
    assert PointChasingVecEnv.env_name == "PointChasingVecEnv"
    assert (PointChasingVecEnv._stem, PointChasingVecEnv._action_at, PointChasingVecEnv._takes_dims) == ("pointchasing", 1, True)
    # nothing the base owns is defined a second time
    own = set(vars(PointChasingVecEnv))
    assert not own & {"step", "step_into", "raw_stepper", "fused_rollout", "fused_rollout_offpolicy", "fused_evaluate",
                      "fused_evaluate_offpolicy", "_env_args", "_ppo_args", "_sac_call", "_dims"}
    # the reference's spellings win where given
    assert PointChasingVecEnv._aliases(4096, 0, None, None) == (4096, 0)
    assert PointChasingVecEnv._aliases(4096, 0, 32, 1) == (32, 1)
    assert PointChasingVecEnv._aliases(7, 2, None, -1) == (7, -1)
    with pytest.raises(RuntimeError, match=r"PointChasingVecEnv is GPU resident \(HIP kernels\); no device available for gpu_id=-1"):
        PointChasingVecEnv(dim=2, env_num=8, sim_gpu_id=-1)
    # the reference's positional order is not this constructor's: its third positional (sim_gpu_id 0) would be a max_step of 0 here
    with pytest.raises(ValueError, match="max_step = 0"):
        PointChasingVecEnv(2, 32, 0)
    # the chase heuristic, on any tensor
    import torch as th
    s = th.arange(24, dtype=th.float32).reshape(2, 12)
    assert th.equal(PointChasingVecEnv.get_action(s), s[:, 0:3] - s[:, 6:9])


def test_reference_import_path_resolves_to_the_same_class():
    code = ("from elegantrl.envs.PointChasingEnv import PointChasingVecEnv\nimport elegantrl_amd.envs as real\n"
            "from elegantrl.envs import PointChasingVecEnv as B\n"
            "assert PointChasingVecEnv is real.PointChasingVecEnv is B\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", code], cwd="/", env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok")
