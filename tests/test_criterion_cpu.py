"""args.criterion without a GPU: the parse in AgentBase (the three supported modules, what is refused and how), the closed forms of
csrc/critic_loss.h against torch's own modules and autograd in fp64, the `criterion=` argument of every update wrapper in ops.py, and
the library entries' refusal of a bad criterion before any launch (null tensors: validation comes first, as in the other ABI CPU
tests)."""
import inspect

import numpy as np
import pytest
import torch as th

from tests import criterion_cases as K

UPDATE_ENTRIES = K.UPDATE_ENTRIES
WRAPPERS = ("ppo_step", "ppo_update", "mlpn_ppo_step", "mlpn_ppo_step_discrete", "ppo_step_discrete", "ppo_update_discrete", "sac_update",
            "sac_update_from_ring", "sac_update_ring_loop", "sac_update_mod", "sac_update_mod_from_ring", "sac_update_mod_ring_loop",
            "sac_update_per_loop", "sac_update_mod_per_loop", "sac_update_per_draw_loop")


def _agent(cls_name, criterion=None):
    from elegantrl_amd import agents
    from elegantrl_amd.train import Config
    cls = getattr(agents, cls_name)
    discrete = "Discrete" in cls_name
    args = Config(cls, None, {"env_name": "x", "num_envs": 1 if "A2C" in cls_name else 8, "max_step": 10, "state_dim": 4, "action_dim": 2, "if_discrete": discrete})
    args.net_dims, args.quiet = [64, 32], True
    if criterion is not None:
        args.criterion = criterion
    return cls(args.net_dims, 4, 2, gpu_id=-1, args=args)


@pytest.mark.parametrize("crit,code", [
    (None, (0, 1.0)), (th.nn.MSELoss(reduction="none"), (0, 1.0)),
    (th.nn.SmoothL1Loss(reduction="none"), (1, 1.0)), (th.nn.SmoothL1Loss(reduction="none", beta=0.5), (1, 0.5)),
    (th.nn.HuberLoss(reduction="none"), (2, 1.0)), (th.nn.HuberLoss(reduction="none", delta=0.25), (2, 0.25))])
def test_the_three_modules_map_to_their_codes(crit, code):
    from elegantrl_amd.agents.AgentBase import criterion_code
    if crit is not None:
        assert criterion_code(crit) == code
    agent = _agent("AgentPPO", crit)
    assert agent.criterion_code == code
    assert isinstance(agent.criterion, th.nn.MSELoss) if crit is None else agent.criterion is crit     # the reference protocol: the module stays


@pytest.mark.parametrize("cls_name", ["AgentPPO", "AgentA2C", "AgentDiscretePPO", "AgentDiscreteA2C", "AgentSAC", "AgentModSAC"])
def test_what_is_refused_is_refused_at_construction(cls_name):
    for crit in (th.nn.MSELoss(), th.nn.SmoothL1Loss(reduction="mean"), th.nn.HuberLoss(reduction="sum")):
        with pytest.raises(ValueError, match="unmask"):
            _agent(cls_name, crit)
    for crit in (th.nn.SmoothL1Loss(reduction="none", beta=0.0), th.nn.L1Loss(reduction="none"), th.nn.BCELoss(reduction="none"),
                 lambda a, b: (a - b) ** 2):
        with pytest.raises(NotImplementedError, match="MSELoss.*SmoothL1Loss.*HuberLoss"):
            _agent(cls_name, crit)
    assert _agent(cls_name, th.nn.SmoothL1Loss(reduction="none", beta=0.5)).criterion_code == (1, 0.5)


@pytest.mark.parametrize("kind", [K.MSE, K.SMOOTH_L1, K.HUBER])
@pytest.mark.parametrize("beta", [1.0, 0.5])
def test_closed_forms_equal_torch_autograd_in_fp64(kind, beta):
    rng = np.random.default_rng(kind * 10 + int(beta * 2))
    d = np.concatenate([3.0 * rng.standard_normal(994), [0.0, beta, -beta, np.nextafter(beta, 0), np.nextafter(beta, 2), -3.0 * beta]])
    target = rng.standard_normal(d.size)
    loss, grad = K.module_loss_and_grad(K.module(kind, beta), target + d, target)
    d_exact = (target + d) - target                                        # what the module sees
    l, dl = K.closed_form(kind, beta, d_exact)
    np.testing.assert_array_equal(loss, l)
    np.testing.assert_array_equal(grad, dl)


def test_every_update_wrapper_takes_the_criterion_by_keyword():
    from elegantrl_amd import _hip, ops
    for name in WRAPPERS:
        p = inspect.signature(getattr(ops, name)).parameters["criterion"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == _hip.CRITERION_MSE == (0, 1.0), name


def _null_args(argtypes):
    import ctypes
    out = []
    for t in argtypes:
        if t in (ctypes.c_float, ctypes.c_double):
            out.append(0.0)
        elif t in (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64):
            out.append(0)
        else:
            out.append(None)
    return out


@pytest.mark.parametrize("entry", UPDATE_ENTRIES)
def test_every_update_entry_refuses_a_bad_criterion_under_its_own_name(entry):
    from elegantrl_amd import _hip
    L = _hip.lib()
    fn, args = getattr(L, entry), _null_args(_hip._SIGNATURES[entry][1])
    for kind, beta, word in ((7, 1.0, b"unknown criterion 7"), (1, 0.0, b"criterion_beta"), (2, -1.0, b"criterion_beta"),
                             (1, float("nan"), b"criterion_beta"), (0, float("inf"), b"criterion_beta")):
        assert L.erl_criterion_next_call(kind, beta) == 0
        rc, msg = fn(*args), L.erl_last_error_string()
        assert rc == -1 and entry.encode() + b":" in msg and word in msg, (entry, kind, beta, msg)
        # the entry took the criterion: the next call is an MSE call again and fails on its null tensors, not on the criterion
        rc, msg = fn(*args), L.erl_last_error_string()
        assert rc == -1 and b"criterion" not in msg, (entry, msg)
    assert L.erl_criterion_next_call(1, 0.5) == 0                       # a good one passes the check: the refusal is about the tensors
    rc, msg = fn(*args), L.erl_last_error_string()
    assert rc == -1 and b"criterion" not in msg, (entry, msg)


def test_a_call_that_never_reaches_its_entry_leaves_no_criterion_behind():
    """ctypes refuses an argument while it converts them: the entry is never entered, and the Smooth-L1 named for it must not fall to the
    next update call of the thread"""
    import ctypes
    from elegantrl_amd import _hip
    L = _hip.lib()
    args = _null_args(_hip._SIGNATURES["erl_ppo_step_f32"][1])
    bad = list(args)
    bad[6] = "not an int"
    with pytest.raises(ctypes.ArgumentError):
        _hip.call_with_criterion(L.erl_ppo_step_f32, (1, 0.0), *bad)          # (a threshold the entry would refuse by name)
    assert L.erl_ppo_step_f32(*args) == -1 and b"criterion" not in L.erl_last_error_string()

