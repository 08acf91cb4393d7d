"""CPU-side checks of the discrete one-launch entry points (csrc/rollout_discrete.hip): ABI 22 in the header, the binding and the library,
the shape query, argument validation before any launch, and the compat import of the new env (no GPU)."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("erl_rollout_discrete_supported", "erl_cartpole_step_f32", "erl_rollout_discrete_cartpole_f32", "erl_eval_discrete_cartpole_f32")


def test_abi_22_and_the_four_symbols():
    from elegantrl_amd import _hip
    txt = open(os.path.join(ROOT, "include", "erl_hip.h")).read()
    assert int(re.search(r"#define ERL_ABI_VERSION (\d+)", txt).group(1)) == _hip.ABI_VERSION == _hip.lib().erl_abi_version() == 23
    for name in NAMES:
        assert name in _hip.EXPORTED_SYMBOLS and re.search(r"ERL_API int " + name + r"\(", txt)
        assert getattr(_hip.lib(), name) is not None


def test_supported_shapes():
    from elegantrl_amd import _hip, ops
    L = _hip.lib()
    for dims in ((4, 64, 32, 2), (4, 128, 128, 2), (64, 32, 32, 8)):
        assert L.erl_rollout_discrete_supported(*dims) == 1 and ops.rollout_discrete_supported(*dims), dims
    for dims in ((4, 100, 32, 2), (65, 64, 32, 2), (4, 64, 32, 9), (4, 64, 32, 1), (4, 256, 64, 2)):
        assert L.erl_rollout_discrete_supported(*dims) == 0 and not ops.rollout_discrete_supported(*dims), dims


def test_entry_points_validate_before_any_launch():
    from elegantrl_amd import _hip
    L = _hip.lib()
    err = L.erl_last_error_string
    # NULL tensors
    rc = L.erl_cartpole_step_f32(None, None, None, None, None, None, None, 64, 5, 0, None)
    assert rc == -1 and b"erl_cartpole_step_f32" in err() and b"NULL" in err()
    rc = L.erl_rollout_discrete_cartpole_f32(None, None, None, 4, 64, 32, 2, None, None, None, 5, 0, 64, 8, None, 0, 0, 1.0,
                                             None, None, None, None, None, None, None, None, None)
    assert rc == -1 and b"erl_rollout_discrete_cartpole_f32" in err() and b"NULL" in err()
    rc = L.erl_eval_discrete_cartpole_f32(None, None, None, 4, 64, 32, 2, None, None, None, 5, 0, 64, 8, None, 0, None)
    assert rc == -1 and b"erl_eval_discrete_cartpole_f32" in err() and b"NULL" in err()
    # unsupported dims are refused whatever the pointers are (dummy non-NULL host addresses: never dereferenced, nothing is launched)
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    for dims in ((4, 100, 32, 2), (65, 64, 32, 2), (4, 64, 32, 9), (4, 64, 32, 1), (4, 256, 64, 2)):
        rc = L.erl_rollout_discrete_cartpole_f32(p, p, p, *dims, p, p, p, 5, 0, 64, 8, None, 0, 0, 1.0, p, p, p, p, p, p, None, None, None)
        assert rc == -1 and b"erl_rollout_discrete_cartpole_f32" in err() and b"unsupported dims" in err(), dims
        rc = L.erl_eval_discrete_cartpole_f32(p, p, p, *dims, p, p, p, 5, 0, 64, 8, p, 1 << 20, None)
        assert rc == -1 and b"erl_eval_discrete_cartpole_f32" in err() and b"unsupported dims" in err(), dims
    # a policy shape the kernel has, on an env that is not CartPole's (state_dim 4)
    rc = L.erl_eval_discrete_cartpole_f32(p, p, p, 64, 32, 32, 8, p, p, p, 5, 0, 64, 8, p, 1 << 20, None)
    assert rc == -1 and b"erl_eval_discrete_cartpole_f32" in err() and b"state_dim is 4" in err()
    # a workspace smaller than the query says
    need = L.erl_eval_workspace_bytes(64, 8)
    rc = L.erl_eval_discrete_cartpole_f32(p, p, p, 4, 64, 32, 2, p, p, p, 5, 0, 64, 8, p, need - 1, None)
    assert rc == -1 and b"erl_eval_discrete_cartpole_f32" in err() and b"erl_eval_workspace_bytes" in err()
    # bad shapes
    rc = L.erl_cartpole_step_f32(p, p, p, p, p, p, p, 0, 5, 0, None)
    assert rc == -1 and b"erl_cartpole_step_f32" in err()
    rc = L.erl_rollout_discrete_cartpole_f32(p, p, p, 4, 64, 32, 2, p, p, p, 0, 0, 64, 8, None, 0, 0, 1.0, p, p, p, p, p, p, None, None, None)
    assert rc == -1 and b"erl_rollout_discrete_cartpole_f32" in err() and b"bad shape" in err()


def test_kernel_path_names_the_route(monkeypatch):
    monkeypatch.delenv("ERL_FUSED_ROLLOUT", raising=False)
    """the text is built without a device: the discrete agents say which rollout route their shape gets"""
    from elegantrl_amd.agents import AgentDiscreteA2C, AgentDiscretePPO
    from elegantrl_amd.train import Config
    for cls in (AgentDiscretePPO, AgentDiscreteA2C):
        def path(net, fused=True):
            args = Config(cls, None, {"env_name": "CartPole-v1", "num_envs": 8, "max_step": 10, "state_dim": 4, "action_dim": 2,
                                      "if_discrete": True})
            args.net_dims, args.quiet = list(net), True
            if fused is not None:
                args.fused_rollout = fused
            return cls(args.net_dims, 4, 2, gpu_id=-1, args=args).kernel_path
        assert "one-launch rollout and evaluation" in path((64, 32))
        assert "per-step rollout loop (args.fused_rollout is off" in path((64, 32), fused=False)
        assert "per-step rollout loop (args.fused_rollout is off" in path((64, 32), fused=None)          # the discrete agents' default
        assert "per-step rollout loop (the one-launch discrete rollout needs" in path((256, 128))
        assert "per-step rollout loop (the one-launch discrete rollout needs" in path((64, 64, 32))


def test_compat_import_of_the_new_env():
    code = ("from elegantrl.envs import CartPoleGpuVecEnv\nimport elegantrl_amd.envs as real\n"
            "assert CartPoleGpuVecEnv is real.CartPoleGpuVecEnv and CartPoleGpuVecEnv.if_discrete and CartPoleGpuVecEnv.env_name == 'CartPole-v1'\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", code], cwd="/", env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("ok")
