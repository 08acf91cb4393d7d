"""Checkpoints written before the off-policy agents shared a base (`_OffPolicyFlatAgent`, agents/AgentBase.py) load into the agents of
today: tests/golden/offpolicy_ckpt_parent/{sac,modsac,td3,ddpg}/ hold `save_or_load_agent(if_save=True)` of stamped agents, recorded on
the commit before that change by tools/record_offpolicy_digests.py (`checkpoints`), never from the tree under test.  A save of today stores
the same values under the same attributes.  The fixtures are the agents' `<attr>.pth` files kept as `<attr>.ckpt` (a `.pth` file in a source
tree reads as a path-configuration file of the interpreter); the test copies them back under their names before it loads."""
import os
import shutil
import tempfile

import pytest
import torch as th

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "offpolicy_ckpt_parent")
KINDS = {"sac": "AgentSAC", "modsac": "AgentModSAC", "td3": "AgentTD3", "ddpg": "AgentDDPG"}
S, A, NET = 3, 1, (8, 8)
STEP, ACTOR_STEP, RNG_COUNTER, ALPHA_LOG = 7, 5, 11, 0.375
BLOCKS = ("_actor_flat", "_critic_flat", "_target_flat", "_actor_target_flat", "_critic_target_flat")
OPTIMIZERS = ("act_optimizer", "cri_optimizer", "alpha_optim")


def make(kind):
    import elegantrl_amd.agents as agents
    from elegantrl_amd.train import Config
    cls = getattr(agents, KINDS[kind])
    args = Config(cls, None, {"env_name": "stub", "num_envs": 4, "max_step": 5, "state_dim": S, "action_dim": A, "if_discrete": False})
    args.net_dims, args.quiet = list(NET), True
    with th.random.fork_rng(devices=[]):
        return cls(args.net_dims, S, A, gpu_id=-1, args=args)


def ramp(n, k):
    """a ramp no two blocks share: block k starts at k and climbs by 2^-8 (exact in fp32 at these sizes)"""
    return th.arange(n, dtype=th.float32) / 256 + k


def expected(agent):
    """name -> tensor of everything `stamp` fills, by the same rule"""
    out = {}
    for k, name in enumerate(BLOCKS):
        if hasattr(agent, name):
            out[name] = ramp(getattr(agent, name).numel(), k)
    for k, name in enumerate(OPTIMIZERS):
        if hasattr(agent, name):
            n = getattr(agent, name).exp_avg.numel()
            out[name + ".exp_avg"], out[name + ".exp_avg_sq"] = ramp(n, 10 + 2 * k), ramp(n, 11 + 2 * k)
    return out


def stamp(agent):
    """distinct non-zero counters, ramps in every flat block (the modules' parameters are views of them) and in every moment"""
    agent._step, agent.rng_counter = STEP, RNG_COUNTER
    if hasattr(agent, "_actor_step"):
        agent._actor_step = ACTOR_STEP
    if hasattr(agent, "alpha_log"):
        agent.alpha_log.fill_(ALPHA_LOG)
    for name, want in expected(agent).items():
        owner, _, attr = name.rpartition(".")
        (getattr(getattr(agent, owner), attr) if owner else getattr(agent, name)).copy_(want)


def record(root=GOLDEN):
    for kind in KINDS:
        os.makedirs(os.path.join(root, kind), exist_ok=True)
        agent = make(kind)
        stamp(agent)
        with tempfile.TemporaryDirectory() as cwd:
            agent.save_or_load_agent(cwd, if_save=True)
            for name in os.listdir(cwd):
                shutil.copyfile(os.path.join(cwd, name), os.path.join(root, kind, name[:-len(".pth")] + ".ckpt"))


def checkpoint_dir(kind, where) -> str:
    """the fixture of `kind` under the file names save_or_load_agent reads"""
    os.makedirs(where)
    for name in os.listdir(os.path.join(GOLDEN, kind)):
        shutil.copyfile(os.path.join(GOLDEN, kind, name), os.path.join(where, name[:-len(".ckpt")] + ".pth"))
    return str(where)


def test_the_adam_state_class_kept_its_old_module_path():
    import importlib
    old, new = (importlib.import_module("elegantrl_amd.agents." + m) for m in ("AgentSAC", "AgentBase"))      # (pickle looks modules up so)
    assert old._FlatAdamState is new._FlatAdamState
    assert ".AgentSAC import" not in open(importlib.import_module("elegantrl_amd.agents.AgentDDPG").__file__).read()


@pytest.mark.parametrize("kind", list(KINDS))
def test_parent_checkpoint_loads(kind, tmp_path):
    agent, parent, today = make(kind), checkpoint_dir(kind, tmp_path / "parent"), str(tmp_path / "today")
    agent.save_or_load_agent(parent, if_save=False)
    assert agent._step == STEP and agent.rng_counter == RNG_COUNTER
    assert getattr(agent, "_actor_step", None) == (None if kind == "sac" else ACTOR_STEP)
    if kind in ("sac", "modsac"):
        assert agent.alpha_log.tolist() == [ALPHA_LOG] and agent.alpha_log.dtype == th.float32
    want = expected(agent)
    assert len(want) == {"sac": 9, "modsac": 10, "td3": 8, "ddpg": 8}[kind]
    for name, w in want.items():
        owner, _, attr = name.rpartition(".")
        got = getattr(getattr(agent, owner), attr) if owner else getattr(agent, name)
        assert th.equal(got, w), name
    # the loaded modules are bound: their parameters are the flat blocks' memory
    for name, bind in agent._binds.items():
        assert bind.is_bound(getattr(agent, name)), name
    assert sorted(agent._binds) == sorted({"sac": ["_act", "cri", "cri_target"]}.get(kind, ["_act", "act_target", "cri", "cri_target"]))
    # a save of today: the same files, and the optimisers carry the same counters under the same attributes
    os.makedirs(today)
    agent.save_or_load_agent(today, if_save=True)
    assert sorted(os.listdir(today)) == sorted(os.listdir(parent))
    for name in OPTIMIZERS:
        if os.path.isfile(os.path.join(parent, name + ".pth")):
            old, new = (th.load(os.path.join(d, name + ".pth"), weights_only=False).__dict__ for d in (parent, today))
            assert sorted(old) == sorted(new), name
            scalars = [k for k in old if not isinstance(old[k], th.Tensor)]
            assert {k: old[k] for k in scalars} == {k: new[k] for k in scalars}, name
            assert all(th.equal(old[k], new[k]) for k in old if k not in scalars), name
