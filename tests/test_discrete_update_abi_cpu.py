"""CPU-side checks of the fused discrete minibatch kernel's entry points (csrc/ppo_step_discrete.hip): the four symbols in the header,
the binding and the library with the ABI still 22, the shape query against the one-launch rollout's, the slab stride, argument
validation before any launch, and the update route in the agents' `kernel_path` (no GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("erl_ppo_discrete_supported", "erl_ppo_discrete_slab_stride", "erl_ppo_step_discrete_f32", "erl_ppo_update_discrete_f32")
GOOD = ((4, 64, 32, 2), (4, 128, 128, 2), (64, 32, 32, 8))
BAD = ((4, 100, 32, 2), (65, 64, 32, 2), (4, 64, 32, 9), (4, 64, 32, 1), (4, 256, 64, 2))


def test_the_four_symbols_and_abi_22():
    from elegantrl_amd import _hip
    txt = open(os.path.join(ROOT, "include", "erl_hip.h")).read()
    assert int(re.search(r"#define ERL_ABI_VERSION (\d+)", txt).group(1)) == _hip.ABI_VERSION == _hip.lib().erl_abi_version() == 23
    for name in NAMES:
        assert name in _hip.EXPORTED_SYMBOLS and re.search(r"ERL_API (int|int64_t) " + name + r"\(", txt), name
        assert getattr(_hip.lib(), name) is not None


def test_supported_shapes_are_the_one_launch_rollouts():
    from elegantrl_amd import _hip, ops
    L = _hip.lib()
    for dims in GOOD:
        assert L.erl_ppo_discrete_supported(*dims) == 1 == L.erl_rollout_discrete_supported(*dims) and ops.ppo_discrete_supported(*dims), dims
    for dims in BAD:
        assert L.erl_ppo_discrete_supported(*dims) == 0 == L.erl_rollout_discrete_supported(*dims) and not ops.ppo_discrete_supported(*dims), dims
        assert L.erl_ppo_discrete_slab_stride(*dims) == -1 == ops.ppo_discrete_slab_stride(*dims), dims


@pytest.mark.parametrize("dims", GOOD + ((6, 64, 32, 4), (17, 32, 32, 3), (5, 96, 64, 5)))
def test_slab_stride(dims):
    from elegantrl_amd import ops
    S, h1, h2, A = dims
    Pa, Pc = ops.MlpSpecN([S, h1, h2, A], False).count, ops.MlpSpecN([S, h1, h2, 1], False).count
    stride = ops.ppo_discrete_slab_stride(*dims)
    assert stride == -(-(Pa + Pc + 4) // 32) * 32 and stride % 32 == 0 and 0 <= stride - (Pa + Pc + 4) < 32


def step_args(p, dims, B=200, n_slabs=2, H=8, N=64):
    return [p] * 6 + list(dims) + [p] * 6 + [H, N, p, B, 0.25, 0.01, 1.0 / max(B, 1), p, n_slabs, None]


def update_args(p, dims, B=200, n_slabs=2, H=8, N=64, update_times=3, first_step=1):
    return [p] * 7 + list(dims) + [p] * 6 + [H, N, p, B, update_times, 0.25, 0.01, p, n_slabs, p, first_step, 1e-3, 0.9, 0.999, 1e-8, 3.0, None]


def test_entry_points_validate_before_any_launch():
    from elegantrl_amd import _hip
    L = _hip.lib()
    err = L.erl_last_error_string
    entries = (("erl_ppo_step_discrete_f32", step_args), ("erl_ppo_update_discrete_f32", update_args))
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)          # a dummy non-NULL host address: never dereferenced, nothing is launched
    for name, mk in entries:
        fn, bname = getattr(L, name), name.encode()
        # NULL tensors
        rc = fn(*mk(None, (4, 64, 32, 2)))
        assert rc == -1 and bname in err() and b"NULL" in err(), name
        # unsupported dims are refused whatever the pointers are
        for dims in BAD:
            rc = fn(*mk(p, dims))
            assert rc == -1 and bname in err() and b"unsupported dims" in err(), (name, dims)
        # bad shapes
        rc = fn(*mk(p, (4, 64, 32, 2), B=0, n_slabs=0))
        assert rc == -1 and bname in err() and b"bad shape" in err(), name
        rc = fn(*mk(p, (4, 64, 32, 2), H=0))
        assert rc == -1 and bname in err() and b"bad shape" in err(), name
        # n_slabs must be erl_ppo_num_slabs(B) = ceil(200 / 128) = 2
        for wrong in (1, 3):
            rc = fn(*mk(p, (4, 64, 32, 2), n_slabs=wrong))
            assert rc == -1 and bname in err() and b"n_slabs" in err() and b"erl_ppo_num_slabs" in err(), (name, wrong)
    rc = L.erl_ppo_update_discrete_f32(*update_args(p, (4, 64, 32, 2), update_times=0))
    assert rc == -1 and b"erl_ppo_update_discrete_f32" in err() and b"bad argument" in err()
    rc = L.erl_ppo_update_discrete_f32(*update_args(p, (4, 64, 32, 2), first_step=0))
    assert rc == -1 and b"erl_ppo_update_discrete_f32" in err() and b"bad argument" in err()


def test_kernel_path_names_the_update_route(monkeypatch):
    """the text is built without a device: flag on / off / default (the class's `_fused_update_default`, which follows the route's A/B record), and shapes without the kernel"""
    monkeypatch.delenv("ERL_FUSED_DISCRETE_UPDATE", raising=False)
    from elegantrl_amd.agents import AgentDiscreteA2C, AgentDiscretePPO
    from elegantrl_amd.train import Config
    for cls in (AgentDiscretePPO, AgentDiscreteA2C):
        def agent(net, fused=None):
            args = Config(cls, None, {"env_name": "CartPole-v1", "num_envs": 8, "max_step": 10, "state_dim": 4, "action_dim": 2,
                                      "if_discrete": True})
            args.net_dims, args.quiet = list(net), True
            if fused is not None:
                args.fused_update = fused
            return cls(args.net_dims, 4, 2, gpu_id=-1, args=args)
        on, off, default = agent((64, 32), True), agent((64, 32), False), agent((64, 32))
        assert on.fused_update_discrete and "update: fused minibatch kernel" in on.kernel_path and "ppo_step_discrete" in on.kernel_path
        assert not off.fused_update_discrete and "update: layered minibatch loop (args.fused_update is off" in off.kernel_path
        assert default.fused_update_discrete == (cls._fused_update_default != "0")
        assert ("update: fused minibatch kernel" if default.fused_update_discrete else "update: layered minibatch loop") in default.kernel_path
        assert on.update_path is None and not on._fused                        # set by update_net; the parameter layout stays the layered one
        for net in ((256, 128), (64, 64, 32)):
            assert "update: layered minibatch loop (the fused discrete minibatch kernel covers" in agent(net, True).kernel_path
        # the rollout's wording is untouched
        assert "; rollout: " in on.kernel_path and on.kernel_path.index("; rollout: ") < on.kernel_path.index("; update: ")
    monkeypatch.setenv("ERL_FUSED_DISCRETE_UPDATE", "1")
    assert "update: fused minibatch kernel" in agent((64, 32)).kernel_path
    monkeypatch.setenv("ERL_FUSED_DISCRETE_UPDATE", "0")
    assert "update: layered minibatch loop" in agent((64, 32)).kernel_path
