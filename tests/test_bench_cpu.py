"""bench.py's launcher logic on CPU (no kernels run): `--gpus N` without WORLD_SIZE starts its own ranks through torch.distributed.run
with the driver's documented arguments; with WORLD_SIZE set (the driver's own torchrun form) it does not."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gpus_n_without_a_launcher_starts_its_own_ranks(monkeypatch):
    bench = _bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0

    import subprocess
    monkeypatch.setattr(subprocess, "call", fake_call)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1", "--config", "cr"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nnodes=1" in cmd
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert 0 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1", "--config", "cr"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def test_a_failing_rank_fails_the_launcher(monkeypatch):
    bench = _bench()
    import subprocess
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: 3)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 3


def test_dump_outputs_keeps_to_its_budget_with_one_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: float32 / float64 files; past the budget every (horizon, envs) array keeps the SAME seeded rows, run after run"""
    import numpy as np
    import torch as th
    bench = _bench()
    H, N = 16, 4096
    row = th.arange(H * N, dtype=th.float32).reshape(H, N)
    arrays = {"states": th.stack([row, -row], dim=2), "rewards": row, "undones": row.remainder(2) == 0,
              "objectives": th.tensor([0.5, -1.25, 3.0], dtype=th.float64), "params": th.linspace(-1, 1, 1000)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays)                # 0.9 MB: under the budget, written whole
    whole = {f[:-4]: np.load(tmp_path / "whole" / f) for f in os.listdir(tmp_path / "whole")}
    assert set(whole) == set(arrays) and whole["states"].shape == (H, N, 2) and whole["undones"].dtype == np.float32
    np.testing.assert_array_equal(whole["rewards"], row.numpy())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 200_000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sum(x.nbytes for x in a.values()) <= 200_000 and a["objectives"].dtype == np.float64 and a["params"].shape == (1000,)
    k = a["rewards"].shape[0]
    assert 0 < k < H * N and a["states"].shape == (k, 2) and a["undones"].shape == (k,)
    np.testing.assert_array_equal(a["states"][:, 0], a["rewards"])    # the same (step, env) rows in every array
    np.testing.assert_array_equal(a["undones"], (a["rewards"] % 2 == 0).astype(np.float32))
    assert len(np.unique(a["rewards"])) == k
    for name, x in a.items():
        np.testing.assert_array_equal(x, np.load(tmp_path / "b" / f"{name}.npy"))
