"""`update_net` of the four off-policy agents on every route keeps the BITS the agents left before the loop, its route decision and the
checkpoint round trip moved into one base class (`_OffPolicyFlatAgent`): tests/golden/offpolicy_update_digests.json, recorded on the
commit before that change by tools/record_offpolicy_digests.py through `run_case` below, never from the tree under test.

Shape: S = 5, A = 2, 4 envs, a ring of 64 rows with 40 filled, batch 32, repeat_times 4 -> 5 steps per update_net: the fewest at which
TD3's delay (update_freq 2 and 3) skips steps and AgentModSAC's two-time-scale rule skips its first (t = 3).  Per case: update_net, save,
load into a fresh agent, update_net again.  The CUDA generator's state after each call pins the order and the size of the draws."""
import hashlib
import json
import os
import tempfile

import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "offpolicy_update_digests.json")
S, A, N, MAX_SIZE, ROWS, B, REPEAT = 5, 2, 4, 64, 40, 32, 4
FUSED, LAYERED = (32, 32), (32, 32, 16)
PER = dict(if_use_per=True)
MOD = dict(fused_step=True)

# name: (agent class, net_dims, args)
CASES = {
    "sac ring loop in C": ("AgentSAC", FUSED, {}),
    "sac ring loop in C, layered": ("AgentSAC", LAYERED, {}),
    "sac per step from the ring": ("AgentSAC", FUSED, dict(update_loop_in_c=False)),
    "sac planar ring": ("AgentSAC", FUSED, dict(replay_interleaved=False)),
    "sac sample_ids_ahead off": ("AgentSAC", FUSED, dict(sample_ids_ahead=False)),
    "sac lambda_fit_cum_r": ("AgentSAC", FUSED, dict(lambda_fit_cum_r=0.5)),
    "sac prioritised loop in C": ("AgentSAC", FUSED, dict(PER)),
    "sac prioritised per step": ("AgentSAC", FUSED, dict(PER, per_loop_in_c=False)),
    "sac per_draw_in_step": ("AgentSAC", FUSED, dict(PER, per_draw_in_step=True)),
    "modsac layered": ("AgentModSAC", LAYERED, {}),
    "modsac fused ring loop": ("AgentModSAC", FUSED, dict(MOD)),
    "modsac fused per step": ("AgentModSAC", FUSED, dict(MOD, update_loop_in_c=False)),
    "modsac mod_per_loop_in_c": ("AgentModSAC", FUSED, dict(MOD, **PER, mod_per_loop_in_c=True)),
    "td3 loop in C": ("AgentTD3", FUSED, dict(td3_loop_in_c=True, update_freq=2)),
    "td3 per step": ("AgentTD3", LAYERED, dict(td3_loop_in_c=False, update_freq=3)),
    "td3 planar": ("AgentTD3", FUSED, dict(td3_loop_in_c=True, update_freq=2, replay_interleaved=False)),
    "td3 prioritised": ("AgentTD3", FUSED, dict(PER, update_freq=3)),
    "ddpg buffer_init_size 40": ("AgentDDPG", FUSED, dict(td3_loop_in_c=True, buffer_init_size=40)),
    "ddpg buffer_init_size 41": ("AgentDDPG", FUSED, dict(td3_loop_in_c=True, buffer_init_size=41)),
}
BLOCKS = ("_actor_flat", "_critic_flat", "_target_flat", "_actor_target_flat", "_critic_target_flat", "alpha_log")
OPTIMIZERS = ("act_optimizer", "cri_optimizer", "alpha_optim")
COUNTERS = ("_step", "_actor_step", "update_a", "rng_counter", "update_path", "per_path")


def _sha(x) -> str:
    if isinstance(x, th.Tensor):
        x = x.detach().cpu().contiguous().numpy().tobytes()
    return hashlib.sha256(x if isinstance(x, bytes) else repr(x).encode()).hexdigest()[:20]


def _state(agent, buffer, returned) -> dict:
    th.cuda.synchronize()
    out = {name: _sha(getattr(agent, name)) for name in BLOCKS if hasattr(agent, name)}
    for name in OPTIMIZERS:
        if hasattr(agent, name):
            out[name] = _sha(getattr(agent, name).exp_avg) + _sha(getattr(agent, name).exp_avg_sq)
    out.update(objs_all=_sha(agent.objs_all), returned=_sha(tuple(float(x) for x in returned)), ids0=_sha(buffer.ids0), ids1=_sha(buffer.ids1),
               cuda_generator=_sha(th.cuda.get_rng_state(0)))
    out.update({name: repr(getattr(agent, name, None)) for name in COUNTERS})
    return out


def run_case(name) -> dict:
    """{"first": ..., "resumed": ...}: digests of everything update_net leaves, after the first call and after the second one on a fresh
    agent that loaded the first one's checkpoint"""
    import elegantrl_amd.agents as agents
    from elegantrl_amd.train import Config, ReplayBuffer
    cls_name, net, flags = CASES[name]
    cls = getattr(agents, cls_name)
    args = Config(cls, None, {"env_name": "stub", "num_envs": N, "max_step": 50, "state_dim": S, "action_dim": A, "if_discrete": False})
    args.net_dims, args.quiet, args.batch_size, args.repeat_times, args.random_seed = list(net), True, B, REPEAT, 3
    for k, v in flags.items():
        setattr(args, k, v)
    dev = th.device("cuda:0")
    rng = np.random.default_rng(2025)
    items = [rng.standard_normal((ROWS, N, S)), np.tanh(rng.standard_normal((ROWS, N, A))), rng.standard_normal((ROWS, N)),
             rng.random((ROWS, N)) > 0.1, rng.random((ROWS, N)) > 0.05]
    last_state = th.from_numpy(rng.standard_normal((N, S)).astype(np.float32)).to(dev)
    buffer = ReplayBuffer(MAX_SIZE, S, A, gpu_id=0, num_seqs=N, if_use_per=bool(flags.get("if_use_per")), args=args)
    buffer.update(tuple(th.from_numpy(x.astype(np.float32)).to(dev) for x in items))

    def agent_of(seed):
        th.manual_seed(seed)
        agent = cls(args.net_dims, S, A, gpu_id=0, args=args)
        agent.last_state = last_state.clone()
        return agent
    out = {}
    first = agent_of(11)
    th.manual_seed(5)                                     # (seeds the CUDA generator too)
    out["first"] = _state(first, buffer, first.update_net(buffer))
    with tempfile.TemporaryDirectory() as cwd:
        first.save_or_load_agent(cwd, if_save=True)
        resumed = agent_of(12)                            # other initial weights: everything it ends with came through the files
        resumed.save_or_load_agent(cwd, if_save=False)
    out["resumed"] = _state(resumed, buffer, resumed.update_net(buffer))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_update_net_matches_parent_digests(name):
    with open(DIGESTS) as f:
        want = json.load(f)["digests"][name]
    got = run_case(name)
    for stage in ("first", "resumed"):
        assert sorted(got[stage]) == sorted(want[stage]), stage
        for field in want[stage]:
            assert got[stage][field] == want[stage][field], (stage, field)
    assert got["first"]["_step"] == "5" and got["resumed"]["_step"] == "10" and got["first"]["objs_all"] != got["resumed"]["objs_all"]
