"""CPU-side checks of the evaluation entry points (csrc/rollout_eval.hip, csrc/sac.hip): the workspace query, argument validation
before any launch, the Config default and an Evaluator without an agent (no GPU)."""
import ctypes

import torch as th

from tests.helpers import ToyActor, ToyVecEnv


def test_eval_workspace_bytes():
    from elegantrl_amd import _hip
    L = _hip.lib()
    sizes = [(n, h, L.erl_eval_workspace_bytes(n, h)) for n, h in ((16, 8), (16, 16), (4096, 200), (4096, 1000), (8192, 1000))]
    for n, h, b in sizes:
        assert b >= n * h * 8 + n * 4 and b % 256 == 0, (n, h, b)          # records (return, length) + per-env counts
    assert [b for _, _, b in sizes] == sorted(b for _, _, b in sizes) and len({b for _, _, b in sizes}) == len(sizes)
    assert L.erl_eval_workspace_bytes(4096, 400) >= 2 * L.erl_eval_workspace_bytes(4096, 200) - 256 - 4 * 4096
    assert L.erl_eval_workspace_bytes(0, 8) == -1 and L.erl_eval_workspace_bytes(8, 0) == -1
    assert L.erl_eval_workspace_bytes(1 << 20, 1 << 20) == -1            # N * H beyond the int32 episode total


def test_eval_entry_points_validate_before_any_launch():
    from elegantrl_amd import _hip
    L = _hip.lib()
    hid = (ctypes.c_int * 2)(256, 256)
    rc = L.erl_eval_synenv_f32(None, None, None, 64, 128, 128, 8, None, None, None, None, None, 5, 0, 64, 8, None, 0, None)
    assert rc == -1 and b"erl_eval_synenv_f32" in L.erl_last_error_string()
    rc = L.erl_eval_pendulum_f32(None, None, None, 128, 64, None, None, None, None, 5, 0, 64, 8, None, 0, None)
    assert rc == -1 and b"erl_eval_pendulum_f32" in L.erl_last_error_string()
    rc = L.erl_sac_eval_synenv_f32(None, 17, 3, hid, 2, None, None, None, None, None, 5, 0, 64, 8, None, 0, None)
    assert rc == -1 and b"erl_sac_eval_synenv_f32" in L.erl_last_error_string()
    rc = L.erl_sac_eval_pendulum_f32(None, hid, 2, None, None, None, None, 5, 0, 64, 8, None, 0, None)
    assert rc == -1 and b"erl_sac_eval_pendulum_f32" in L.erl_last_error_string()
    rc = L.erl_eval_episodes_compact_f32(None, 0, 64, 8, None, 0, None, None)
    assert rc == -1 and b"erl_eval_episodes_compact_f32" in L.erl_last_error_string()
    # an unsupported shape is refused on its dims, whatever the pointers are (dummy non-NULL host addresses: never dereferenced,
    # nothing is launched)
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    assert not L.erl_rollout_fused_supported(65, 128, 128, 8)
    rc = L.erl_eval_synenv_f32(p, p, p, 65, 128, 128, 8, p, p, p, p, p, 5, 0, 64, 8, p, 1 << 20, None)
    assert rc == -1 and b"unsupported dims" in L.erl_last_error_string()
    rc = L.erl_eval_pendulum_f32(p, p, p, 100, 64, p, p, p, p, 5, 0, 64, 8, p, 1 << 20, None)
    assert rc == -1 and b"unsupported dims" in L.erl_last_error_string()
    assert not L.erl_sac_rollout_synenv_supported(60, 8, hid, 2, 64)
    rc = L.erl_sac_eval_synenv_f32(p, 60, 8, hid, 2, p, p, p, p, p, 5, 0, 64, 8, p, 1 << 20, None)
    assert rc == -1 and b"unsupported dims" in L.erl_last_error_string()
    rc = L.erl_sac_eval_pendulum_f32(p, hid, 2, p, p, p, p, 5, 0, 5000, 8, p, 1 << 30, None)          # N > 4096
    assert rc == -1 and b"unsupported dims" in L.erl_last_error_string()
    # a workspace smaller than the query says
    rc = L.erl_eval_synenv_f32(p, p, p, 64, 128, 128, 8, p, p, p, p, p, 5, 0, 64, 8, p, 64 * 8 * 8, None)
    assert rc == -1 and b"erl_eval_workspace_bytes" in L.erl_last_error_string()
    rc = L.erl_eval_episodes_compact_f32(p, 100, 64, 8, p, 10, p, None)
    assert rc == -1 and b"erl_eval_workspace_bytes" in L.erl_last_error_string()


def test_config_default_and_evaluator_without_an_agent(tmp_path, capsys):
    from elegantrl_amd.train import Config
    from elegantrl_amd.train.evaluator import Evaluator
    assert Config().fused_eval is True
    env = ToyVecEnv(6)
    args = Config()
    args.gpu_id, args.eval_times, args.eval_per_step, args.eval_record_step = 0, 12, 150, 0
    actor = ToyActor.build(env.state_dim, env.action_dim)
    with th.no_grad():
        ev = Evaluator(str(tmp_path), env, args)
        assert ev.agent is None
        rs = ev.get_cumulative_rewards_and_step(actor)
    assert rs.ndim == 2 and rs.shape[1] == 2 and rs.shape[0] >= 6 and rs.dtype == th.float32
    assert ev.eval_path.startswith("loop evaluation") and "no agent" in ev.eval_path
    assert "| Evaluator: loop evaluation" in capsys.readouterr().out
