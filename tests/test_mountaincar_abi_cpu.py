"""CPU-side checks of the MountainCar entry points (csrc/rollout_discrete.hip, csrc/mountaincar_step.h): the four symbols in the header,
the binding and the library at ABI 23, argument validation before any launch, the agent's route text and the compat import of the new
env (no GPU)."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("erl_mountaincar_step_f32", "erl_rollout_discrete_mountaincar_f32", "erl_rollout_discrete_mountaincar_gae_f32",
         "erl_eval_discrete_mountaincar_f32")
UNSUPPORTED = ((2, 100, 32, 3), (65, 64, 32, 3), (2, 64, 32, 9), (2, 64, 32, 1), (2, 256, 64, 3))
TWINS = {"erl_mountaincar_step_f32": "erl_cartpole_step_f32", "erl_rollout_discrete_mountaincar_f32": "erl_rollout_discrete_cartpole_f32",
         "erl_rollout_discrete_mountaincar_gae_f32": "erl_rollout_discrete_cartpole_gae_f32",
         "erl_eval_discrete_mountaincar_f32": "erl_eval_discrete_cartpole_f32"}


def test_abi_is_still_23_with_the_four_symbols():
    from elegantrl_amd import _hip
    txt = open(os.path.join(ROOT, "include", "erl_hip.h")).read()
    assert int(re.search(r"#define ERL_ABI_VERSION (\d+)", txt).group(1)) == _hip.ABI_VERSION == _hip.lib().erl_abi_version() == 23
    for name in NAMES:
        assert name in _hip.EXPORTED_SYMBOLS and re.search(r"ERL_API int " + name + r"\(", txt)
        assert getattr(_hip.lib(), name) is not None
    # the header's parameter count is the binding's, and both are the CartPole twin's, type for type
    for name in NAMES:
        proto = re.search(r"ERL_API int " + name + r"\(([^;]*)\);", txt).group(1)
        twin = re.search(r"ERL_API int " + TWINS[name] + r"\(([^;]*)\);", txt).group(1)
        assert len(proto.split(",")) == len(_hip._SIGNATURES[name][1]), name
        assert [" ".join(a.split()) for a in proto.split(",")] == [" ".join(a.split()) for a in twin.split(",")], name
        assert _hip._SIGNATURES[name] == _hip._SIGNATURES[TWINS[name]], name
    # the shape queries are what they were: MountainCar's shape is inside both
    assert _hip.lib().erl_rollout_discrete_supported(2, 64, 32, 3) == 1
    assert _hip.lib().erl_ppo_discrete_supported(2, 64, 32, 3) == 1


def gae_call(fn, p, dims=(2, 64, 32, 3), n=64, ms=5, parts_bytes=1 << 20, state=True, critic=True):
    """erl_rollout_discrete_mountaincar_gae_f32 with `p` for every pointer but those named"""
    return fn(p, p, p, *dims, p if state else None, p, p, ms, 0, n, 8, None, 0, 0, 1.0, p, p, p, p, p, p, None, None,
              p if critic else None, p, p, p, p, p, p, p, parts_bytes, 0.99, 0.95, 1, None)


def test_entry_points_validate_before_any_launch():
    from elegantrl_amd import _hip
    L = _hip.lib()
    err = L.erl_last_error_string
    ro, ga, ev = L.erl_rollout_discrete_mountaincar_f32, L.erl_rollout_discrete_mountaincar_gae_f32, L.erl_eval_discrete_mountaincar_f32
    # NULL tensors
    rc = L.erl_mountaincar_step_f32(None, None, None, None, None, None, None, 64, 5, 0, None)
    assert rc == -1 and b"erl_mountaincar_step_f32" in err() and b"NULL" in err()
    rc = ro(None, None, None, 2, 64, 32, 3, None, None, None, 5, 0, 64, 8, None, 0, 0, 1.0, None, None, None, None, None, None, None, None,
            None)
    assert rc == -1 and b"erl_rollout_discrete_mountaincar_f32" in err() and b"NULL" in err()
    rc = gae_call(ga, None)
    assert rc == -1 and b"erl_rollout_discrete_mountaincar_gae_f32" in err() and b"NULL" in err()
    rc = ev(None, None, None, 2, 64, 32, 3, None, None, None, 5, 0, 64, 8, None, 0, None)
    assert rc == -1 and b"erl_eval_discrete_mountaincar_f32" in err() and b"NULL" in err()
    # dummy non-NULL host addresses: never dereferenced, nothing is launched
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    # one NULL among them is enough: the live state, an output row, the critic, the workspace
    rc = ro(p, p, p, 2, 64, 32, 3, None, p, p, 5, 0, 64, 8, None, 0, 0, 1.0, p, p, p, p, p, p, None, None, None)
    assert rc == -1 and b"erl_rollout_discrete_mountaincar_f32" in err() and b"NULL" in err()
    rc = ro(p, p, p, 2, 64, 32, 3, p, p, p, 5, 0, 64, 8, None, 0, 0, 1.0, p, p, p, None, p, p, None, None, None)
    assert rc == -1 and b"erl_rollout_discrete_mountaincar_f32" in err() and b"NULL" in err()
    rc = gae_call(ga, p, state=False)
    assert rc == -1 and b"erl_rollout_discrete_mountaincar_gae_f32" in err() and b"NULL" in err()
    rc = gae_call(ga, p, critic=False)
    assert rc == -1 and b"erl_rollout_discrete_mountaincar_gae_f32" in err() and b"NULL tensor (critic_params)" in err()
    rc = ev(p, p, p, 2, 64, 32, 3, None, p, p, 5, 0, 64, 8, p, 1 << 20, None)
    assert rc == -1 and b"erl_eval_discrete_mountaincar_f32" in err() and b"NULL" in err()
    rc = ev(p, p, p, 2, 64, 32, 3, p, p, p, 5, 0, 64, 8, None, 1 << 20, None)
    assert rc == -1 and b"erl_eval_discrete_mountaincar_f32" in err() and b"NULL" in err()
    rc = L.erl_mountaincar_step_f32(p, None, p, p, p, p, p, 64, 5, 0, None)
    assert rc == -1 and b"erl_mountaincar_step_f32" in err() and b"NULL" in err()
    # unsupported dims are refused whatever the pointers are
    for dims in UNSUPPORTED:
        rc = ro(p, p, p, *dims, p, p, p, 5, 0, 64, 8, None, 0, 0, 1.0, p, p, p, p, p, p, None, None, None)
        assert rc == -1 and b"erl_rollout_discrete_mountaincar_f32" in err() and b"unsupported dims" in err(), dims
        rc = gae_call(ga, p, dims=dims)
        assert rc == -1 and b"erl_rollout_discrete_mountaincar_gae_f32" in err() and b"unsupported dims" in err(), dims
        rc = ev(p, p, p, *dims, p, p, p, 5, 0, 64, 8, p, 1 << 20, None)
        assert rc == -1 and b"erl_eval_discrete_mountaincar_f32" in err() and b"unsupported dims" in err(), dims
    # a policy shape the kernel has, on an env that is not MountainCar's (state_dim 2, action_dim 3)
    for dims, msg in (((4, 64, 32, 3), b"state_dim is 2"), ((2, 64, 32, 2), b"action_dim is 3"), ((4, 64, 32, 2), b"state_dim is 2"),
                      ((6, 64, 32, 3), b"state_dim is 2")):
        rc = ro(p, p, p, *dims, p, p, p, 5, 0, 64, 8, None, 0, 0, 1.0, p, p, p, p, p, p, None, None, None)
        assert rc == -1 and b"erl_rollout_discrete_mountaincar_f32" in err() and msg in err(), (dims, err())
        rc = gae_call(ga, p, dims=dims)
        assert rc == -1 and b"erl_rollout_discrete_mountaincar_gae_f32" in err() and msg in err(), (dims, err())
        rc = ev(p, p, p, *dims, p, p, p, 5, 0, 64, 8, p, 1 << 20, None)
        assert rc == -1 and b"erl_eval_discrete_mountaincar_f32" in err() and msg in err(), (dims, err())
    # a workspace smaller than the query says
    need = L.erl_eval_workspace_bytes(64, 8)
    rc = ev(p, p, p, 2, 64, 32, 3, p, p, p, 5, 0, 64, 8, p, need - 1, None)
    assert rc == -1 and b"erl_eval_discrete_mountaincar_f32" in err() and b"erl_eval_workspace_bytes" in err()
    need = L.erl_rollout_discrete_gae_workspace_bytes(64)
    rc = gae_call(ga, p, parts_bytes=need - 1)
    assert rc == -1 and b"erl_rollout_discrete_mountaincar_gae_f32" in err() and b"erl_rollout_discrete_gae_workspace_bytes" in err()
    # bad shapes: N = 0, max_step = 0
    rc = L.erl_mountaincar_step_f32(p, p, p, p, p, p, p, 0, 5, 0, None)
    assert rc == -1 and b"erl_mountaincar_step_f32" in err() and b"bad shape" in err()
    rc = L.erl_mountaincar_step_f32(p, p, p, p, p, p, p, 64, 0, 0, None)
    assert rc == -1 and b"erl_mountaincar_step_f32" in err() and b"bad shape" in err()
    for n, ms in ((0, 5), (64, 0)):
        rc = ro(p, p, p, 2, 64, 32, 3, p, p, p, ms, 0, n, 8, None, 0, 0, 1.0, p, p, p, p, p, p, None, None, None)
        assert rc == -1 and b"erl_rollout_discrete_mountaincar_f32" in err() and b"bad shape" in err()
        rc = gae_call(ga, p, n=n, ms=ms)
        assert rc == -1 and b"erl_rollout_discrete_mountaincar_gae_f32" in err() and b"bad shape" in err()
        rc = ev(p, p, p, 2, 64, 32, 3, p, p, p, ms, 0, n, 8, p, 1 << 20, None)
        assert rc == -1 and b"erl_eval_discrete_mountaincar_f32" in err() and b"bad shape" in err()


def test_kernel_path_names_the_three_envs(monkeypatch):
    """the text is built without a device"""
    monkeypatch.delenv("ERL_FUSED_ROLLOUT", raising=False)
    from elegantrl_amd.agents import AgentDiscretePPO
    from elegantrl_amd.train import Config
    args = Config(AgentDiscretePPO, None, {"env_name": "MountainCar-v0", "num_envs": 8, "max_step": 10, "state_dim": 2, "action_dim": 3,
                                           "if_discrete": True})
    args.net_dims, args.quiet, args.fused_rollout = [64, 32], True, True
    path = AgentDiscretePPO(args.net_dims, 2, 3, gpu_id=-1, args=args).kernel_path
    assert "one-launch rollout and evaluation" in path
    assert "MountainCarGpuVecEnv" in path and "AcrobotGpuVecEnv" in path and "CartPoleGpuVecEnv" in path
    assert "fused minibatch kernel" in path          # (2, 64, 32, 3) has the fused update as well


def test_env_class_without_a_device():
    from elegantrl_amd.envs import MountainCarGpuVecEnv
    from elegantrl_amd.envs.vec_envs import _DiscreteGpuVecEnv
    assert issubclass(MountainCarGpuVecEnv, _DiscreteGpuVecEnv) and MountainCarGpuVecEnv.if_discrete
    assert MountainCarGpuVecEnv.env_name == "MountainCar-v0"
    assert (MountainCarGpuVecEnv._rollout_entry, MountainCarGpuVecEnv._gae_entry, MountainCarGpuVecEnv._eval_entry) == NAMES[1:]


def test_compat_import_of_the_new_env():
    code = ("from elegantrl.envs import MountainCarGpuVecEnv\nimport elegantrl_amd.envs as real\n"
            "assert MountainCarGpuVecEnv is real.MountainCarGpuVecEnv and MountainCarGpuVecEnv.if_discrete\n"
            "assert MountainCarGpuVecEnv.env_name == 'MountainCar-v0'\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", code], cwd="/", env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok")
