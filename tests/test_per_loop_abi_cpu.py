"""CPU-side checks of the prioritised-replay loop's entry points (csrc/per.hip, csrc/sac.hip): erl_per_sample_rows_f32,
erl_per_update_index_f32 and erl_sac_update_per_loop_f32 are exported, bound, and refuse bad arguments before any launch, each under
its own name (no GPU: the pointers are dummy host addresses that are never dereferenced)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("erl_per_sample_rows_f32", "erl_per_update_index_f32", "erl_sac_update_per_loop_f32")


def test_symbols_are_exported_and_the_versions_agree():
    from elegantrl_amd import _hip
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), f"liberl_hip.so does not export {name}"
        assert name in _hip.EXPORTED_SYMBOLS
    txt = open(os.path.join(ROOT, "include", "erl_hip.h")).read()
    assert int(re.search(r"#define ERL_ABI_VERSION (\d+)", txt).group(1)) == _hip.ABI_VERSION == _hip.lib().erl_abi_version()
    for name in NEW + ("ErlPerSample",):
        assert name in txt


class _Args:
    """valid arguments of the three entry points at S = 5, A = 2 (row_floats 12), a ring of 40 rows x 2 sequences holding 17, batch 16"""

    def __init__(self):
        from elegantrl_amd import ops
        self.buf = (ctypes.c_char * 4096)()
        self.p = ctypes.addressof(self.buf)                  # 16-byte aligned or not: made so below
        self.p += (-self.p) % 16
        self.S, self.A, self.rw = 5, 2, 12
        self.max_size, self.num_seqs, self.cur_size, self.cursor, self.n_per_seq = 40, 2, 17, -1, 8
        self.sum = self.min = self.ring = self.p
        self.n_steps, self.B = 3, 16
        self.hidden = (ctypes.c_int * 2)(64, 32)
        self.ws_bytes = ops.SacSpec(self.S, self.A, [64, 32], 2).workspace_bytes(self.B)

    def sample_rows(self, L):
        p = self.p
        return L.erl_per_sample_rows_f32(self.sum, self.min, self.max_size, self.num_seqs, p, self.n_per_seq, self.cur_size, self.cursor, 0.4,
                                         self.ring, self.S, self.A, self.rw, p, p, p, p, p, p, p, p, p, p, None)

    def update_index(self, L):
        return L.erl_per_update_index_f32(self.sum, self.min, self.max_size, self.num_seqs, self.p, self.cur_size, self.p, self.B, 0.6, None)

    def loop(self, L):
        from elegantrl_amd.ops import _PerSample, _RingSample
        p = self.p
        rs = _RingSample(self.ring, None, None, None, None, self.max_size, self.num_seqs, None, 0, p, p, self.rw)
        pr = _PerSample(self.sum, self.min, self.max_size, self.num_seqs, self.cur_size, self.cursor, 0.6, 0.4, p, p, p, p)
        return L.erl_sac_update_per_loop_f32(*([p] * 10), self.S, self.A, self.hidden, 2, 2, ctypes.addressof(rs), ctypes.addressof(pr),
                                             self.n_steps, *([p] * 6), self.B, 1, 1, 0.99, 1.0, 0.005, 1e-3, 0.9, 0.999, 1e-8, 3.0, 1, p, p,
                                             self.ws_bytes, None)


def _null_trees(a):
    a.sum = None


def _null_min_tree(a):
    a.min = None


def _cur_size_one(a):
    a.cur_size = 1


def _no_draws(a):
    a.n_per_seq, a.B = 0, 0


def _no_steps(a):
    a.n_steps = 0


def _ragged_batch(a):
    a.B = 15


def _planar_ring(a):
    a.rw = 0


def _negative_row(a):
    a.rw = -12


CASES = [  # (what is wrong, the entry points it applies to)
    (_null_trees, ("sample_rows", "update_index", "loop")),
    (_null_min_tree, ("sample_rows", "update_index", "loop")),
    (_cur_size_one, ("sample_rows", "update_index", "loop")),
    (_no_draws, ("sample_rows", "loop")),
    (_no_steps, ("loop",)),
    (_ragged_batch, ("loop",)),
    (_planar_ring, ("sample_rows", "loop")),
    (_negative_row, ("sample_rows", "loop")),
]
NAMES = {"sample_rows": b"erl_per_sample_rows_f32", "update_index": b"erl_per_update_index_f32", "loop": b"erl_sac_update_per_loop_f32"}


@pytest.mark.parametrize("spoil,entries", CASES, ids=[c[0].__name__.lstrip("_") for c in CASES])
def test_bad_arguments_are_refused_before_any_launch(spoil, entries):
    from elegantrl_amd import _hip
    L = _hip.lib()
    for entry in entries:
        a = _Args()
        spoil(a)
        rc = getattr(a, entry)(L)
        msg = L.erl_last_error_string()
        assert rc == -1 and NAMES[entry] in msg, (entry, rc, msg)


def test_ring_and_trees_must_agree_and_the_workspace_must_fit():
    from elegantrl_amd import _hip
    L = _hip.lib()
    a = _Args()
    a.ws_bytes -= 1
    assert a.loop(L) == -1 and b"erl_sac_update_per_loop_f32: workspace too small" in L.erl_last_error_string()
    a = _Args()
    a.cur_size = a.max_size + 1
    for entry in ("sample_rows", "update_index", "loop"):
        assert getattr(a, entry)(L) == -1 and NAMES[entry] in L.erl_last_error_string()
    a = _Args()
    a.ring += 4                                            # a block that is not 16-byte aligned
    for entry in ("sample_rows", "loop"):
        assert getattr(a, entry)(L) == -1 and NAMES[entry] in L.erl_last_error_string()


def test_switch_default_and_buffer_twin_without_a_device():
    """per_for_fused_loop declines on a buffer that has no interleaved ring (no GPU here: planar CPU tensors), like ring_for_fused_sample
    declines for PER"""
    from elegantrl_amd.train import ReplayBuffer
    buf = ReplayBuffer(max_size=8, state_dim=3, action_dim=2, gpu_id=-1, num_seqs=2, if_use_per=False)
    assert buf.per_for_fused_loop(4) is None
