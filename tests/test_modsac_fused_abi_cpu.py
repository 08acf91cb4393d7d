"""CPU-side checks of the fused AgentModSAC step's entry points (csrc/sac.hip erl_sac_update_mod_*, csrc/sac_fused.hip): the four symbols in
the header, the binding and the library with the ABI still 22, the shape query at its limits, argument validation before any launch, and the
step route in AgentModSAC's `kernel_path` (no GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("erl_sac_mod_fused_supported", "erl_sac_update_mod_f32", "erl_sac_update_mod_ring_f32", "erl_sac_update_mod_ring_loop_f32")


def test_the_four_symbols_and_abi_22():
    from elegantrl_amd import _hip
    txt = open(os.path.join(ROOT, "include", "erl_hip.h")).read()
    assert int(re.search(r"#define ERL_ABI_VERSION (\d+)", txt).group(1)) == _hip.ABI_VERSION == _hip.lib().erl_abi_version() == 23
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NAMES:
        assert name in _hip.EXPORTED_SYMBOLS and re.search(r"ERL_API int " + name + r"\(", txt), name
        assert hasattr(raw, name) and getattr(_hip.lib(), name) is not None


def _hid(*h):
    return (ctypes.c_int * len(h))(*h), len(h)


def test_supported_answers_at_the_limits():
    from elegantrl_amd import _hip, ops
    sup = _hip.lib().erl_sac_mod_fused_supported
    assert sup(56, 8, *_hid(256, 256), 8, 4096) == 1
    assert sup(1, 1, *_hid(16, 16), 1, 1) == 1
    for S, A, hid, E, B in ((55, 9, (256, 256), 8, 4096),            # A 9
                            (57, 8, (256, 256), 8, 4096),            # S + A 65
                            (56, 8, (24, 256), 8, 4096), (56, 8, (256, 24), 8, 4096),      # width 24
                            (56, 8, (272, 256), 8, 4096),            # wider than 256
                            (56, 8, (256,), 8, 4096), (56, 8, (256, 256, 256), 8, 4096),   # one / three hidden layers
                            (56, 8, (256, 256), 9, 4096),            # E 9
                            (56, 8, (256, 256), 8, 4097)):           # B 4097
        assert sup(S, A, *_hid(*hid), E, B) == 0, (S, A, hid, E, B)
    assert ops.sac_mod_fused_supported(ops.SacSpec(56, 8, [256, 256], 8, actor_variant=_hip.SAC_ACTOR_FIX), 4096)
    assert not ops.sac_mod_fused_supported(ops.SacSpec(11, 3, [64], 8, actor_variant=_hip.SAC_ACTOR_FIX), 64)


S, A, E, B = 11, 3, 8, 64
FLOATS = [0.99, -1.1, 0.005, 1e-3, 0.9, 0.999, 1e-8, 3.0]


def _ring(p, row_floats, ids, max_size=64, num_seqs=8, sample_len=31):
    from elegantrl_amd.ops import _RingSample
    return _RingSample(p, p if not row_floats else None, p if not row_floats else None, p if not row_floats else None,
                       p if not row_floats else None, max_size, num_seqs, ids, sample_len, None, None, row_floats)


def _calls(p, ws_bytes, hid=(64, 32), step=1, n_steps=3, actor_step0=0, ring=None, B_=B):
    """argument lists of the three entries with `p` for every tensor"""
    h, nh = _hid(*hid)
    head = [p] * 10 + [S, A, h, nh, E]
    r = ctypes.addressof(ring) if ring is not None else None
    return {
        "erl_sac_update_mod_f32": head + [p] * 8 + [B_, None, None, 1, 1] + FLOATS + [step, 1, 1, p, p, p, ws_bytes, None],
        "erl_sac_update_mod_ring_f32": head + [r] + [p] * 6 + [B_, None, None, 1, 1] + FLOATS + [step, 1, 1, p, p, p, ws_bytes, None],
        "erl_sac_update_mod_ring_loop_f32": head + [r, p, n_steps] + [p] * 6 + [B_, 1, 1] + FLOATS + [step, actor_step0, 1.0, p, p, None, p,
                                                                                                     ws_bytes, None],
    }


def test_entry_points_validate_before_any_launch():
    """every refusal comes back as ERL_EINVAL with the entry's name in the error string; nothing is launched (no device here), and the dummy
    non-NULL host address is never dereferenced"""
    from elegantrl_amd import _hip
    L = _hip.lib()
    err = L.erl_last_error_string
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                        # (the interleaved ring's base must be 16-byte aligned)
    h, nh = _hid(64, 32)
    need = L.erl_sac_workspace_bytes(S, A, h, nh, E, B)
    assert need > 0
    rf = L.erl_replay_row_floats(S, A)
    good = _ring(p, rf, p)

    def refused(name, args, *words):
        rc = getattr(L, name)(*args)
        msg = err()
        assert rc == -1 and name.encode() in msg and all(w in msg for w in words), (name, rc, msg)

    for name in NAMES[1:]:
        refused(name, _calls(None, need, ring=good)[name], b"NULL")                                     # NULL tensors
        refused(name, _calls(p, need - 1, ring=good)[name], b"workspace")                               # a short workspace
        refused(name, _calls(p, need, step=0, ring=good)[name], b"step")                                # step / step0 < 1
        for hid in ((64,), (64, 48, 32), (64, 24), (272, 64)):                                          # outside the fused step's shapes
            refused(name, _calls(p, 1 << 40, hid=hid, ring=good)[name], b"outside the fused step's shapes")
        refused(name, _calls(p, 1 << 40, ring=good, B_=4097)[name], b"outside the fused step's shapes")
    planar = _ring(p, 0, p)
    planar.buf_unmasks = None                                                                           # a planar ring short of an array
    wrong_rf, no_base, no_rows, no_ids = _ring(p, rf + 4, p), _ring(None, rf, p), _ring(p, rf, p, sample_len=0), _ring(p, rf, None)
    for name in NAMES[2:]:                                             # (the ring structs stay alive: the calls take their addresses)
        refused(name, _calls(p, need, ring=None)[name], b"NULL ring")                                   # no ring at all
        refused(name, _calls(p, need, ring=wrong_rf)[name], b"row_floats")                              # row_floats is not the ring's
        refused(name, _calls(p, need, ring=no_base)[name], b"NULL ring")
        refused(name, _calls(p, need, ring=planar)[name], b"NULL ring")
        refused(name, _calls(p, need, ring=no_rows)[name], b"bad ring shape")
    refused(NAMES[2], _calls(p, need, ring=no_ids)[NAMES[2]], b"NULL ring")                             # the single step reads ring->ids
    loop = NAMES[3]
    refused(loop, _calls(p, need, ring=good, n_steps=-1)[loop], b"n_steps=-1")
    refused(loop, _calls(p, need, ring=good, actor_step0=-1)[loop], b"actor_step0=-1")
    a = _calls(p, need, ring=good)[loop]
    a[16] = None                                                                                        # ids_all
    refused(loop, a, b"NULL")
    # update_actor with an actor step below 1
    a = _calls(p, need)[NAMES[1]]
    a[-6] = 0
    refused(NAMES[1], a, b"actor_step=0")
    # zero steps: nothing to launch, the count of actor updates is written
    n = ctypes.c_int32(-7)
    a = _calls(p, need, ring=good, n_steps=0)[loop]
    a[-4] = ctypes.byref(n)
    assert getattr(L, loop)(*a) == 0 and n.value == 0


def test_kernel_path_names_the_step_route(monkeypatch):
    """the text is built without a device: flag on / off / unset (the class's `_fused_step_default`, which follows the route's A/B record),
    the environment switch, and shapes / options the fused step does not cover"""
    monkeypatch.delenv("ERL_FUSED_MODSAC_STEP", raising=False)
    monkeypatch.delenv("ERL_SAC_FUSED", raising=False)
    from elegantrl_amd.agents import AgentModSAC
    from elegantrl_amd.train import Config

    def agent(net, fused=None, **extra):
        args = Config(AgentModSAC, None, {"env_name": "x", "num_envs": 4, "max_step": 10, "state_dim": 11, "action_dim": 3, "if_discrete": False})
        args.net_dims, args.quiet, args.batch_size = list(net), True, 64
        if fused is not None:
            args.fused_step = fused
        for k, v in extra.items():
            setattr(args, k, v)
        return AgentModSAC(args.net_dims, 11, 3, gpu_id=-1, args=args)

    on, off, default = agent((256, 256), True), agent((256, 256), False), agent((256, 256))
    assert on.fused_step and on.kernel_path.startswith("fused ModSAC step") and "erl_sac_update_mod_f32" in on.kernel_path
    assert not off.fused_step and off.kernel_path.startswith("layered ModSAC step") and "args.fused_step is off" in off.kernel_path
    assert "erl_sac_update_opt_f32" in off.kernel_path
    assert default.fused_step == (AgentModSAC._fused_step_default != "0")
    assert default.kernel_path.startswith("fused ModSAC step" if default.fused_step else "layered ModSAC step")
    assert on.update_path is None and on.per_path is None                       # set by update_net
    for net in ((64,), (64, 48, 32), (64, 24)):
        a = agent(net, True)
        assert a.fused_step and a.kernel_path.startswith("layered ModSAC step") and "outside the fused step's shapes" in a.kernel_path, net
    assert "lambda_fit_cum_r" in agent((256, 256), True, lambda_fit_cum_r=0.3).kernel_path
    assert "outside the fused step's shapes" in agent((256, 256), True, num_ensembles=9).kernel_path
    # the route is a per-call choice
    on.fused_step = False
    assert on._fused_step_reason(64) is not None
    on.fused_step = True
    assert on._fused_step_reason(64) is None and on._fused_step_reason(4097) is not None
    monkeypatch.setenv("ERL_FUSED_MODSAC_STEP", "1")
    assert agent((64, 32)).kernel_path.startswith("fused ModSAC step")
    monkeypatch.setenv("ERL_FUSED_MODSAC_STEP", "0")
    assert agent((64, 32)).kernel_path.startswith("layered ModSAC step")
    assert agent((64, 32), True).kernel_path.startswith("fused ModSAC step")    # args wins over the environment
    monkeypatch.setenv("ERL_SAC_FUSED", "0")
    assert "ERL_SAC_FUSED=0" in agent((64, 32), True).kernel_path
