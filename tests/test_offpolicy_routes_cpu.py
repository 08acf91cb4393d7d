"""`_OffPolicyFlatAgent._update_net_route` -- which route an off-policy `update_net` takes and what `update_path` / `per_path` say about
it -- driven without a GPU on stub buffers, against the table written out below: the four agent classes, every condition broken alone.
The strings are the ones the agents wrote before the decision had a place of its own.  The decision launches nothing and draws nothing."""
import pytest
import torch as th

S, A, B = 5, 2, 32
FUSED, LAYERED = (32, 32), (32, 32, 16)


@pytest.fixture(autouse=True)
def _leave_the_global_rng_alone():
    """(as in test_agent_routes_cpu.py: the agents built here draw their initial weights from torch's global generator)"""
    with th.random.fork_rng(devices=[]):
        yield


@pytest.fixture(autouse=True)
def _no_switches_from_the_environment(monkeypatch):
    for name in ("ERL_SAC_FUSED", "ERL_SAC_SAMPLE_IN_STEP", "ERL_SAC_LOOP_IN_C", "ERL_SAC_PER_LOOP_IN_C", "ERL_SAC_PER_DRAW_IN_STEP",
                 "ERL_SAC_MOD_PER_LOOP_IN_C", "ERL_FUSED_MODSAC_STEP", "ERL_TD3_LOOP_IN_C"):
        monkeypatch.delenv(name, raising=False)


def make(cls_name, net=FUSED, **flags):
    import elegantrl_amd.agents as agents
    from elegantrl_amd.train import Config
    cls = getattr(agents, cls_name)
    args = Config(cls, None, {"env_name": "stub", "num_envs": 4, "max_step": 5, "state_dim": S, "action_dim": A, "if_discrete": False})
    args.net_dims, args.quiet, args.batch_size, args.repeat_times = list(net), True, B, 4
    for k, v in flags.items():
        setattr(args, k, v)
    return cls(args.net_dims, S, A, gpu_id=-1, args=args)


class StubBuffer:
    """cur_size / num_seqs and, where `ring` / `per` are given, the two calls the decision asks the buffer through; each counts its calls"""

    def __init__(self, ring="absent", per="absent", cur_size=40):
        self.cur_size, self.num_seqs, self.asked = cur_size, 4, []
        if ring != "absent":
            self.ring_for_fused_sample = lambda batch_size: self.asked.append(("ring", batch_size)) or ring
        if per != "absent":
            self.per_for_fused_loop = lambda batch_size: self.asked.append(("per", batch_size)) or per


def ring_of(kind):
    """what ReplayBuffer.ring_for_fused_sample returns: (arrays, sample_len, stage) with `arrays` a ReplayRing or five planar tensors"""
    from elegantrl_amd import ops
    if kind is None:
        return None
    arrays = ops.ReplayRing.__new__(ops.ReplayRing) if kind == "interleaved" else (object(),) * 5
    return arrays, 39, object()


PER = (object(),) * 8                   # per_for_fused_loop's tuple: the decision hands it on unopened

# ---- the table ------------------------------------------------------------------------------------------------------------------------
SAC_LOOP = "one C call (erl_sac_update_ring_loop_f32: the sample inside every step's first launch)"
MOD_LOOP = "one C call (erl_sac_update_mod_ring_loop_f32: the sample inside every step's first launch, the two-time-scale rule in C)"
TD3_LOOP = "one C call (erl_td3_update_ring_loop_f32: sample, step and the actor's delay rule per step inside the call)"
NO_RING_SAC = "per step: StubBuffer offers no continuous-action ring of >= 2 rows for the sample inside the step"
NO_RING_TD3 = "per step: StubBuffer offers no continuous-action ring of >= 2 rows"
FUSED_OFF = "args.fused_step is off (ERL_FUSED_MODSAC_STEP; profiles/modsac_update_ab.txt)"
SAC_PER = "per step: prioritised replay (per_path names its route)"
TD3_PER = "per step: prioritised replay (a prioritised one-call loop is out of scope): sample_for_per, erl_td3_update_f32, tree update per step"
PER_STEPS = "prioritised update loop per step (_per_step: six host-driven calls): "
PER_LOOP = "prioritised update loop in one C call (erl_sac_update_per_loop_f32: draw + gather, step, tree update per step)"
PER_DRAW_LOOP = ("prioritised update loop in one C call (erl_sac_update_per_draw_loop_f32: draw + gather inside the step's first launch, "
                 "tree update behind every step)")
MOD_PER_LOOP = ("prioritised update loop in one C call (erl_sac_update_mod_per_loop_f32: draw + gather, step, tree update behind every step, "
                "the two-time-scale rule in C)")
MOD_PER_DRAW_LOOP = ("prioritised update loop in one C call (erl_sac_update_mod_per_loop_f32: draw + gather inside the step's first launch, "
                     "tree update behind every step, the two-time-scale rule in C)")
MOD_PER_HOST = ("ActorFixSAC / two-time-scale options (AgentModSAC) are decided per step by the host unless args.mod_per_loop_in_c is on "
                "(ERL_SAC_MOD_PER_LOOP_IN_C; profiles/sac_per_loop_ab.txt)")
NOT_OFFERED = "the buffer is not an interleaved continuous-action ring of >= 2 rows, or batch_size is no multiple of num_seqs"
ON = dict(if_use_per=True)

# case: (class, net, flags, ring kind or "absent", per tuple / None / "absent") -> (route, update_path, per_path, what the buffer was asked)
TABLE = {
    # AgentSAC, uniform replay
    "sac, interleaved ring": (("AgentSAC", FUSED, {}, "interleaved", "absent"), ("ring_loop", SAC_LOOP, None, ["ring"])),
    "sac, layered net, interleaved ring": (("AgentSAC", LAYERED, {}, "interleaved", "absent"), ("ring_loop", SAC_LOOP, None, ["ring"])),
    "sac, planar ring": (("AgentSAC", FUSED, {}, "planar", "absent"), ("ring_loop", SAC_LOOP, None, ["ring"])),
    "sac, the buffer offers no ring": (("AgentSAC", FUSED, {}, None, "absent"), ("batch_step", NO_RING_SAC, None, ["ring"])),
    "sac, a buffer without the call": (("AgentSAC", FUSED, {}, "absent", "absent"), ("batch_step", NO_RING_SAC, None, [])),
    "sac, update_loop_in_c off": (("AgentSAC", FUSED, dict(update_loop_in_c=False), "interleaved", "absent"),
                                  ("ring_step", "per step: args.update_loop_in_c is off", None, ["ring"])),
    "sac, sample_in_step off": (("AgentSAC", FUSED, dict(sample_in_step=False), "interleaved", "absent"),
                                ("batch_step", "per step: args.sample_in_step is off", None, [])),
    "sac, sample_ids_ahead off": (("AgentSAC", FUSED, dict(sample_ids_ahead=False), "interleaved", "absent"),
                                  ("batch_step", "per step: args.sample_ids_ahead is off", None, [])),
    "sac, lambda_fit_cum_r": (("AgentSAC", FUSED, dict(lambda_fit_cum_r=0.5), "interleaved", "absent"),
                              ("batch_step", "per step: lambda_fit_cum_r needs ids0 / ids1 on the host side of every step", None, [])),
    # AgentModSAC, uniform replay
    "modsac, fused_step off": (("AgentModSAC", FUSED, dict(fused_step=False), "interleaved", "absent"),
                               ("batch_step", "per step: layered ModSAC step, which reads a finished batch: " + FUSED_OFF, None, [])),
    "modsac, fused_step on": (("AgentModSAC", FUSED, dict(fused_step=True), "interleaved", "absent"), ("ring_loop", MOD_LOOP, None, ["ring"])),
    "modsac, fused_step on, update_loop_in_c off": (("AgentModSAC", FUSED, dict(fused_step=True, update_loop_in_c=False), "interleaved", "absent"),
                                                    ("ring_step", "per step: args.update_loop_in_c is off", None, ["ring"])),
    "modsac, fused_step on, no ring": (("AgentModSAC", FUSED, dict(fused_step=True), None, "absent"), ("batch_step", NO_RING_SAC, None, ["ring"])),
    # AgentSAC, prioritised replay
    "sac per, the buffer offers the loop": (("AgentSAC", FUSED, ON, "absent", PER), ("per_loop", SAC_PER, PER_LOOP, ["per"])),
    "sac per, per_draw_in_step": (("AgentSAC", FUSED, dict(ON, per_draw_in_step=True), "absent", PER), ("per_loop", SAC_PER, PER_DRAW_LOOP, ["per"])),
    "sac per, per_draw_in_step on a layered net": (
        ("AgentSAC", LAYERED, dict(ON, per_draw_in_step=True), "absent", PER),
        ("per_loop", SAC_PER, PER_LOOP + "; args.per_draw_in_step ignored: net_dims [32, 32, 16], batch 32 take the layered step, which reads a "
         "finished batch (the stand-alone draw runs)", ["per"])),
    "sac per, the buffer declines": (("AgentSAC", FUSED, ON, "absent", None), ("per_step", SAC_PER, PER_STEPS + NOT_OFFERED, ["per"])),
    "sac per, a buffer without the call": (("AgentSAC", FUSED, ON, "absent", "absent"),
                                           ("per_step", SAC_PER, PER_STEPS + "StubBuffer has no per_for_fused_loop", [])),
    "sac per, per_loop_in_c off": (("AgentSAC", FUSED, dict(ON, per_loop_in_c=False), "absent", PER),
                                   ("per_step", SAC_PER, PER_STEPS + "args.per_loop_in_c is off", [])),
    "sac per, update_loop_in_c off": (("AgentSAC", FUSED, dict(ON, update_loop_in_c=False), "absent", PER),
                                      ("per_step", SAC_PER, PER_STEPS + "args.update_loop_in_c is off", [])),
    "sac per, lambda_fit_cum_r": (("AgentSAC", FUSED, dict(ON, lambda_fit_cum_r=0.5), "absent", PER),
                                  ("per_step", SAC_PER, PER_STEPS + "lambda_fit_cum_r needs ids0 / ids1 on the host side of every step", [])),
    # AgentModSAC, prioritised replay
    "modsac per, mod_per_loop_in_c off": (("AgentModSAC", FUSED, dict(ON, fused_step=True, mod_per_loop_in_c=False), "absent", PER),
                                          ("per_step", SAC_PER, PER_STEPS + MOD_PER_HOST, [])),
    "modsac per, mod_per_loop_in_c on": (("AgentModSAC", FUSED, dict(ON, fused_step=True, mod_per_loop_in_c=True), "absent", PER),
                                         ("per_loop", SAC_PER, MOD_PER_LOOP, ["per"])),
    "modsac per, mod_per_loop_in_c and per_draw_in_step": (
        ("AgentModSAC", FUSED, dict(ON, fused_step=True, mod_per_loop_in_c=True, per_draw_in_step=True), "absent", PER),
        ("per_loop", SAC_PER, MOD_PER_DRAW_LOOP, ["per"])),
    "modsac per, mod_per_loop_in_c on, fused_step off": (
        ("AgentModSAC", FUSED, dict(ON, fused_step=False, mod_per_loop_in_c=True), "absent", PER),
        ("per_step", SAC_PER, PER_STEPS + "AgentModSAC's prioritised loop (erl_sac_update_mod_per_loop_f32) has no layered form: " + FUSED_OFF, [])),
    "modsac per, mod_per_loop_in_c on, the buffer declines": (
        ("AgentModSAC", FUSED, dict(ON, fused_step=True, mod_per_loop_in_c=True), "absent", None), ("per_step", SAC_PER, PER_STEPS + NOT_OFFERED, ["per"])),
    # AgentTD3 / AgentDDPG
    "td3, td3_loop_in_c on": (("AgentTD3", FUSED, dict(td3_loop_in_c=True), "interleaved", "absent"), ("ring_loop", TD3_LOOP, None, ["ring"])),
    "td3, td3_loop_in_c off": (("AgentTD3", FUSED, dict(td3_loop_in_c=False), "interleaved", "absent"),
                               ("ring_step", "per step: args.td3_loop_in_c is off (ERL_TD3_LOOP_IN_C; profiles/td3_update_ab.txt): "
                                "erl_td3_update_ring_f32 per step", None, ["ring"])),
    "td3, planar ring": (("AgentTD3", FUSED, dict(td3_loop_in_c=True), "planar", "absent"),
                         ("ring_step", "per step: planar replay ring (args.replay_interleaved is off): erl_td3_update_ring_f32 per step", None,
                          ["ring"])),
    "td3, no ring": (("AgentTD3", LAYERED, dict(td3_loop_in_c=True), None, "absent"), ("batch_step", NO_RING_TD3, None, ["ring"])),
    "td3, a buffer without the call": (("AgentTD3", FUSED, dict(td3_loop_in_c=True), "absent", "absent"), ("batch_step", NO_RING_TD3, None, [])),
    "td3 per": (("AgentTD3", FUSED, dict(ON, td3_loop_in_c=True), "interleaved", PER), ("per_step", TD3_PER, None, [])),
    "ddpg, td3_loop_in_c on": (("AgentDDPG", FUSED, dict(td3_loop_in_c=True), "interleaved", "absent"), ("ring_loop", TD3_LOOP, None, ["ring"])),
    "ddpg, td3_loop_in_c off": (("AgentDDPG", FUSED, dict(td3_loop_in_c=False), "interleaved", "absent"),
                                ("ring_step", "per step: args.td3_loop_in_c is off (ERL_TD3_LOOP_IN_C; profiles/td3_update_ab.txt): "
                                 "erl_td3_update_ring_f32 per step", None, ["ring"])),
    "ddpg, planar ring": (("AgentDDPG", FUSED, {}, "planar", "absent"),
                          ("ring_step", "per step: planar replay ring (args.replay_interleaved is off): erl_td3_update_ring_f32 per step", None,
                           ["ring"])),
    "ddpg per": (("AgentDDPG", FUSED, ON, "absent", "absent"), ("per_step", TD3_PER, None, [])),
}


def _forbid_launches(monkeypatch, agent):
    """anything that would enqueue work, allocate a workspace or run a step raises"""
    from elegantrl_amd import _hip, ops

    def refuse(*a, **k):
        raise AssertionError("the route decision reached a launch")
    for mod, name in ((ops, "_update_call"), (ops, "_workspace"), (_hip, "ptr"), (_hip, "stream_ptr")):
        monkeypatch.setattr(mod, name, refuse)
    for name in ("_update_ring_loop", "_update_per_loop", "_update_from_ring", "_update_on_batch", "_per_step", "_sync_modules"):
        monkeypatch.setattr(agent, name, refuse, raising=False)        # (AgentTD3 has no _update_per_loop)


@pytest.mark.parametrize("case", list(TABLE))
def test_route_table(case, monkeypatch):
    (cls_name, net, flags, ring_kind, per), (route, update_path, per_path, asked) = TABLE[case]
    agent = make(cls_name, net, **flags)               # (gpu_id = -1: the agent lives on the CPU whether or not a GPU is present)
    ring = "absent" if ring_kind == "absent" else ring_of(ring_kind)
    buffer = StubBuffer(ring=ring, per=per)
    _forbid_launches(monkeypatch, agent)
    rng, counters = th.random.get_rng_state(), (agent._step, agent.rng_counter, agent.update_path, agent.per_path)
    got = agent._update_net_route(buffer)
    assert got._fields == ("route", "update_path", "per_path", "source")
    assert tuple(got[:3]) == (route, update_path, per_path), (case, got)
    assert [what for what, _ in buffer.asked] == asked and all(b == B for _, b in buffer.asked), buffer.asked
    # what the buffer handed over travels with the route, unopened; nothing was drawn and nothing on the agent moved
    want_source = ring if route in ("ring_loop", "ring_step") else per if route == "per_loop" else None
    assert got.source is want_source
    assert th.equal(rng, th.random.get_rng_state())
    assert counters == (agent._step, agent.rng_counter, agent.update_path, agent.per_path)


def test_the_four_classes_decide_in_one_place():
    from elegantrl_amd.agents import AgentDDPG, AgentModSAC, AgentSAC, AgentTD3
    from elegantrl_amd.agents.AgentBase import _OffPolicyFlatAgent
    for cls in (AgentSAC, AgentModSAC, AgentTD3, AgentDDPG):
        assert issubclass(cls, _OffPolicyFlatAgent)
        for name in ("_update_net_route", "update_net", "save_or_load_agent", "_per_step", "_sync_modules", "_on_act_replaced"):
            assert getattr(cls, name) is getattr(_OffPolicyFlatAgent, name), (cls.__name__, name)


@pytest.mark.parametrize("cls_name", ["AgentSAC", "AgentModSAC", "AgentTD3", "AgentDDPG"])
def test_fewer_rows_than_one_step_needs(cls_name, monkeypatch):
    """update_times = int(cur_size * repeat_times / batch_size) < 1: (0.0, 0.0), no route taken, nothing drawn"""
    agent = make(cls_name)
    buffer = StubBuffer(ring=ring_of("interleaved"), cur_size=7)             # 7 * 4 / 32 < 1
    for name in ("_update_net_route", "_update_ring_loop", "_update_from_ring", "_update_on_batch", "_per_step"):
        monkeypatch.setattr(agent, name, lambda *a, **k: pytest.fail(f"{name} ran"))
    rng = th.random.get_rng_state()
    assert agent.update_net(buffer) == (0.0, 0.0)
    assert agent.objs_all is None and agent.update_path is None and buffer.asked == []
    assert th.equal(rng, th.random.get_rng_state())
