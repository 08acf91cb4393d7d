"""CPU-side checks of the two further prioritised loops (csrc/sac.hip): erl_sac_update_mod_per_loop_f32 (AgentModSAC: the prioritised loop and
the two-time-scale rule from one call) and erl_sac_update_per_draw_loop_f32 (AgentSAC: the draw inside the step's first launch) are
exported, bound, declared in the header within ABI 23, and refuse bad arguments before any launch, each under its own name (no GPU: the
pointers are dummy host addresses that are never dereferenced)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("erl_sac_update_mod_per_loop_f32", "erl_sac_update_per_draw_loop_f32")


def test_symbols_are_exported_and_the_abi_is_still_23():
    from elegantrl_amd import _hip
    raw = ctypes.CDLL(_hip.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "erl_hip.h")).read()
    for name in NEW:
        assert hasattr(raw, name), f"liberl_hip.so does not export {name}"
        assert name in _hip.EXPORTED_SYMBOLS
        assert re.search(r"\bERL_API\s+int\s+%s\s*\(" % name, txt), f"{name} has no prototype in include/erl_hip.h"
    assert int(re.search(r"#define ERL_ABI_VERSION (\d+)", txt).group(1)) == _hip.ABI_VERSION == _hip.lib().erl_abi_version() == 23


def test_the_wrappers_are_new_functions():
    from elegantrl_amd import ops
    assert callable(ops.sac_update_mod_per_loop) and callable(ops.sac_update_per_draw_loop)
    assert ops.sac_update_mod_per_loop is not ops.sac_update_per_loop and ops.sac_update_per_draw_loop is not ops.sac_update_per_loop


class _Args:
    """valid arguments of both entries at S = 5, A = 2 (row_floats 12), a ring of 40 rows x 2 sequences holding 17, batch 16, net (64, 32)"""

    def __init__(self):
        self.buf = (ctypes.c_char * 4096)()
        self.p = ctypes.addressof(self.buf)
        self.p += (-self.p) % 16
        self.S, self.A, self.rw = 5, 2, 12
        self.max_size, self.num_seqs, self.cur_size, self.cursor = 40, 2, 17, -1
        self.sum = self.min = self.ring = self.p
        self.n_steps, self.B = 3, 16
        self.net = [64, 32]
        self.actor_step0, self.critic_value, self.draw_in_step = 0, 1.0, 0
        self.ws_short = 0

    def _common(self):
        from elegantrl_amd import ops
        from elegantrl_amd.ops import _PerSample, _RingSample
        p = self.p
        hidden = (ctypes.c_int * len(self.net))(*self.net)
        ws_bytes = ops.SacSpec(self.S, self.A, self.net, 2).workspace_bytes(max(self.B, 1)) - self.ws_short
        rs = _RingSample(self.ring, None, None, None, None, self.max_size, self.num_seqs, None, 0, p, p, self.rw)
        pr = _PerSample(self.sum, self.min, self.max_size, self.num_seqs, self.cur_size, self.cursor, 0.6, 0.4, p, p, p, p)
        head = (*([p] * 10), self.S, self.A, hidden, len(self.net), 2, ctypes.addressof(rs), ctypes.addressof(pr), self.n_steps, *([p] * 6),
                self.B, 1, 1, 0.99, 1.0, 0.005, 1e-3, 0.9, 0.999, 1e-8, 3.0, 1)
        return head, (p, ws_bytes, None), (rs, pr, hidden)                      # (the structs stay alive until the call returns)

    def mod(self, L):
        head, tail, keep = self._common()
        n_upd = ctypes.c_int32(-7)
        return L.erl_sac_update_mod_per_loop_f32(*head, self.actor_step0, self.critic_value, self.p, self.p, ctypes.byref(n_upd),
                                                 self.draw_in_step, *tail)

    def draw(self, L):
        head, tail, keep = self._common()
        return L.erl_sac_update_per_draw_loop_f32(*head, self.p, *tail)


NAMES = {"mod": b"erl_sac_update_mod_per_loop_f32", "draw": b"erl_sac_update_per_draw_loop_f32"}
BOTH = ("mod", "draw")


def _set(**kw):
    def spoil(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return spoil


def _unaligned_ring(a):
    a.ring += 4


CASES = {  # what is wrong: (how, the entries it applies to, a word of the refusal)
    "null-trees": (_set(sum=None), BOTH, b"NULL trees"),
    "null-min-tree": (_set(min=None), BOTH, b"NULL trees"),
    "cur_size-one": (_set(cur_size=1), BOTH, b"cur_size=1"),
    "cur_size-beyond-the-ring": (_set(cur_size=41), BOTH, b"cur_size=41"),
    "no-steps": (_set(n_steps=0), BOTH, b"n_steps=0"),
    "ragged-batch": (_set(B=15), BOTH, b"batch 15 must be num_seqs=2"),
    "planar-ring": (_set(rw=0), BOTH, b"the interleaved ring only"),
    "negative-row": (_set(rw=-12), BOTH, b"the interleaved ring only"),
    "unaligned-ring": (_unaligned_ring, BOTH, b"the interleaved ring only"),
    "workspace-too-small": (_set(ws_short=1), BOTH, b"workspace too small"),
    "negative-actor_step0": (_set(actor_step0=-1), ("mod",), b"actor_step0=-1"),
    "nan-critic_value": (_set(critic_value=float("nan")), ("mod",), b"critic_value="),
    "three-hidden-layers": (_set(net=[64, 48, 32]), BOTH, b"outside the fused step's shapes"),
    "draw_in_step-two": (_set(draw_in_step=2), ("mod",), b"draw_in_step=2"),
    "draw_in_step-negative": (_set(draw_in_step=-1), ("mod",), b"draw_in_step=-1"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_bad_arguments_are_refused_before_any_launch(case):
    from elegantrl_amd import _hip
    L = _hip.lib()
    spoil, entries, word = CASES[case]
    for entry in entries:
        a = _Args()
        spoil(a)
        rc = getattr(a, entry)(L)
        msg = L.erl_last_error_string()
        assert rc == -1 and msg.startswith(NAMES[entry] + b":") and word in msg, (entry, rc, msg)


def test_the_switches_default_to_off_without_a_device(monkeypatch):
    """both routes are opt-in: an agent built from a Config that names neither switch has them off, the environment turns them on"""
    from elegantrl_amd.agents import AgentModSAC, AgentSAC
    from elegantrl_amd.train import Config

    def build(cls):
        args = Config(cls, None, {"env_name": "x", "num_envs": 4, "max_step": 10, "state_dim": 5, "action_dim": 2, "if_discrete": False})
        args.net_dims, args.quiet, args.if_use_per = [64, 32], True, True
        assert not hasattr(args, "per_draw_in_step") and not hasattr(args, "mod_per_loop_in_c")
        return cls(args.net_dims, 5, 2, gpu_id=-1, args=args)
    for name in ("ERL_SAC_PER_DRAW_IN_STEP", "ERL_SAC_MOD_PER_LOOP_IN_C"):
        monkeypatch.delenv(name, raising=False)
    sac, mod = build(AgentSAC), build(AgentModSAC)
    assert not sac.per_draw_in_step and not mod.per_draw_in_step and not mod.mod_per_loop_in_c
    assert "AgentModSAC" in mod._variant_per_loop_reason() and sac._variant_per_loop_reason() is None
    monkeypatch.setenv("ERL_SAC_PER_DRAW_IN_STEP", "1")
    monkeypatch.setenv("ERL_SAC_MOD_PER_LOOP_IN_C", "1")
    sac, mod = build(AgentSAC), build(AgentModSAC)
    assert sac.per_draw_in_step and mod.per_draw_in_step and mod.mod_per_loop_in_c
