"""The two places where the agents decide which kernels run, driven without a GPU: `AgentPPO._update_route` (which minibatch loop an
`update_net` takes and what follows from it) against the table written out below, and `AgentBase._one_launch_reason` (does this agent /
env pair take the one-launch rollout or evaluation) on a stub env: each condition broken alone, and the rollout and the evaluation of
one agent giving the same answer."""
import pytest
import torch as th

CUDA = th.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_the_global_rng_alone():
    """every agent built here draws its initial weights from torch's global generator, and tests that run later in the same session
    (those that build an agent without seeding first) would see other weights than without this module: put the state back"""
    with th.random.fork_rng(devices=[]):
        yield


def make(cls_name, net, S, A, **flags):
    import elegantrl_amd.agents as agents
    from elegantrl_amd.train import Config
    cls = getattr(agents, cls_name)
    discrete = "Discrete" in cls_name
    args = Config(cls, None, {"env_name": "stub", "num_envs": 48, "max_step": 5, "state_dim": S, "action_dim": A, "if_discrete": discrete})
    args.net_dims, args.quiet = list(net), True
    for k, v in flags.items():
        setattr(args, k, v)
    return cls(args.net_dims, S, A, gpu_id=-1, args=args)


# ---- the route table ------------------------------------------------------------------------------------------------------------------
# gradient-row strides, by hand: a dense layer has in * out + out parameters, the Gaussian actor its A log-stds on top, the row ends in 4
# logged values; the fused kernels round it up to whole 128-byte lines (32 floats)
#   (128, 128), S 8, A 2:   actor 1152 + 16512 + 258 + 2 = 17924, critic 1152 + 16512 + 129 = 17793, + 4 = 35721 -> 35744
#   (256, 128), S 8, A 2:   actor 2304 + 32896 + 258 + 2 = 35460, critic 2304 + 32896 + 129 = 35329, + 4 = 70793 -> 70816
#   (64, 64, 32), S 8, A 2: actor 576 + 4160 + 2080 + 66 + 2 = 6884, critic 576 + 4160 + 2080 + 33 = 6849, + 4 = 13737
#   discrete (64, 32), S 4, A 2:   actor 320 + 2080 + 66 = 2466, critic 320 + 2080 + 33 = 2433, + 4 = 4903 -> 4928
#   discrete (256, 128), S 4, A 2: actor 1280 + 32896 + 258 = 34434, critic 1280 + 32896 + 129 = 34305, + 4 = 68743
C_LOOP = lambda stride: ("c_loop", stride, True, True, True)            # noqa: E731
TORCH_DP = lambda stride: ("torch_dp", stride, True, False, False)      # noqa: E731
LAYERED = lambda stride: ("layered", stride, False, False, False)       # noqa: E731
DISCRETE_FUSED = lambda stride: ("discrete_fused", stride, True, False, True)   # noqa: E731
#                                                         (dp, comm) = (F, F)           (T, T)           (T, F)
TABLE = {
    "fused (128, 128)": (("AgentPPO", (128, 128), 8, 2, {}), C_LOOP(35744), C_LOOP(35744), TORCH_DP(35744)),
    "wide (256, 128)": (("AgentPPO", (256, 128), 8, 2, {}), C_LOOP(70816), C_LOOP(70816), TORCH_DP(70816)),
    "wide, ppo_arith f32": (("AgentPPO", (256, 128), 8, 2, {"ppo_arith": "f32"}), LAYERED(70793), LAYERED(70793), LAYERED(70793)),
    "three layers": (("AgentPPO", (64, 64, 32), 8, 2, {}), LAYERED(13737), LAYERED(13737), LAYERED(13737)),
    "discrete, flag on": (("AgentDiscretePPO", (64, 32), 4, 2, {"fused_update": True}), DISCRETE_FUSED(4928), LAYERED(4903), LAYERED(4903)),
    "discrete, flag off": (("AgentDiscretePPO", (64, 32), 4, 2, {"fused_update": False}), LAYERED(4903), LAYERED(4903), LAYERED(4903)),
    "discrete, no kernel": (("AgentDiscretePPO", (256, 128), 4, 2, {"fused_update": True}), LAYERED(68743), LAYERED(68743), LAYERED(68743)),
}
FIELDS = ("name", "stride", "slabs", "normalises_in_kernel", "takes_rollout_advantages")


@pytest.mark.parametrize("case", list(TABLE))
def test_route_table(case):
    (cls_name, net, S, A, flags), *rows = TABLE[case]
    agent = make(cls_name, net, S, A, **flags)
    for (dp, has_comm), want in zip(((False, False), (True, True), (True, False)), rows):
        route = agent._update_route(dp, has_comm)
        assert route._fields == FIELDS
        assert tuple(route) == want, (case, dp, has_comm, route)
        assert all(type(x) is type(y) for x, y in zip(route, want)), route


# ---- the env-pairing rule -------------------------------------------------------------------------------------------------------------
class StubEnv:
    def __init__(self, agent, methods, **over):
        self.device, self.num_envs, self.state_dim, self.action_dim = CUDA, agent.num_envs, agent.state_dim, agent.action_dim
        for m in methods:
            setattr(self, m, lambda *a, **k: None)
        for k, v in over.items():
            setattr(self, k, v)


# class, net, S, A, (rollout method, evaluation method), a shape of the same agent class without the one-launch route and its reason
PAIRS = {
    "AgentPPO": ((128, 128), 8, 2, ("fused_rollout", "fused_evaluate"), (256, 128), "fused path"),
    "AgentDiscretePPO": ((64, 32), 4, 2, ("fused_rollout_discrete", "fused_evaluate_discrete"), (256, 128), "outside"),
    "AgentSAC": ((64, 64), 8, 2, ("fused_rollout_offpolicy", "fused_evaluate_offpolicy"), (64, 64, 64), "outside"),
}


def on_cuda(cls_name, net=None, **flags):
    dims, S, A, methods, _, _ = PAIRS[cls_name]
    agent = make(cls_name, net or dims, S, A, fused_rollout=True, **flags)
    agent.device = CUDA                # (a device object: no GPU is touched)
    return agent, methods


@pytest.mark.parametrize("cls_name", list(PAIRS))
def test_env_pairing_rule(cls_name):
    agent, methods = on_cuda(cls_name)
    intact = StubEnv(agent, methods)
    for what in methods:
        assert agent._one_launch_reason(intact, what) is None
    assert agent._fused_eval_reason(intact) is None
    # each condition broken alone -> its reason, the same for the rollout and the evaluation
    broken = [(dict(device=th.device("cpu")), "lives on"), (dict(device=th.device("cuda:1")), "lives on"), (dict(num_envs=32), "envs"),
              (dict(state_dim=agent.state_dim + 1), "dims are not the agent's"), (dict(action_dim=agent.action_dim + 1), "dims are not the agent's")]
    for over, why in broken:
        env = StubEnv(agent, methods, **over)
        reasons = [agent._one_launch_reason(env, what) for what in methods]
        assert why in reasons[0] and reasons[0] == reasons[1] == agent._fused_eval_reason(env), (over, reasons)
    for what in methods:               # an env without the method: the one line that names `what`
        env = StubEnv(agent, [m for m in methods if m != what])
        assert agent._one_launch_reason(env, what) == f"StubEnv has no {what}"
    # the agent's own conditions, on the intact env
    agent.fused_rollout = False
    assert all("fused_rollout is off" in agent._one_launch_reason(intact, what) for what in methods)
    agent.fused_rollout = True
    agent.device = th.device("cpu")
    assert all(agent._one_launch_reason(intact, what) == "no GPU" for what in methods)
    _, _, _, _, other_net, why = PAIRS[cls_name]
    other, _ = on_cuda(cls_name, net=other_net)
    env = StubEnv(other, methods)
    reasons = [other._one_launch_reason(env, what) for what in methods]
    assert why in reasons[0] and reasons[0] == reasons[1], reasons


def test_modsac_has_no_one_launch_route():
    from elegantrl_amd.agents import AgentModSAC  # noqa: F401
    agent = make("AgentModSAC", (64, 64), 8, 2, fused_rollout=True)
    agent.device = CUDA
    env = StubEnv(agent, PAIRS["AgentSAC"][3])
    assert all("ActorFixSAC" in agent._one_launch_reason(env, what) for what in PAIRS["AgentSAC"][3])


@pytest.mark.parametrize("cls_name", ["AgentPPO", "AgentSAC"])
def test_rollout_refuses_an_env_built_for_another_action_dim(cls_name):
    """the check the PPO and the SAC rollout did not make before they shared the rule: such an env's `Wa` has another shape"""
    agent, (rollout, _) = on_cuda(cls_name)
    env = StubEnv(agent, [rollout], action_dim=agent.action_dim + 1)
    assert "dims are not the agent's" in agent._one_launch_reason(env, rollout)
