"""CPU-side checks of the TD3 / DDPG entry points (csrc/td3.hip): the six symbols in the header, the binding and the library; every
refusal returns nonzero with the entry's own name in the message before anything is launched (there is no device here, and the dummy
non-NULL host address is never dereferenced); the workspace query is monotone in B and E."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("erl_td3_param_counts", "erl_td3_workspace_bytes", "erl_td3_explore_action_f32", "erl_td3_update_f32", "erl_td3_update_ring_f32",
         "erl_td3_update_ring_loop_f32")
UPDATES = NAMES[3:]
S, A, E, B = 11, 3, 8, 64
FLOATS = [0.1, 0.99, 0.005, 1e-3, 0.9, 0.999, 1e-8, 3.0]       # policy_noise_std, gamma, tau, lr, beta1, beta2, eps_adam, max_norm


def _hid(*h):
    return (ctypes.c_int * len(h))(*h), len(h)


def test_the_six_symbols_are_declared_bound_and_exported():
    from elegantrl_amd import _hip, ops
    from tests.test_abi_signatures_cpu import ctypes_kind, header_prototypes
    txt = open(os.path.join(ROOT, "include", "erl_hip.h")).read()
    protos = header_prototypes()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NAMES:
        assert name in _hip.EXPORTED_SYMBOLS and re.search(r"ERL_API \w+ " + name + r"\(", txt), name
        assert hasattr(raw, name) and getattr(_hip.lib(), name) is not None
        res, argtypes = _hip._SIGNATURES[name]
        assert [ctypes_kind(t) for t in argtypes] == protos[name], name                   # the declared signature, argument by argument
        assert res is (ctypes.c_int64 if name == "erl_td3_workspace_bytes" else ctypes.c_int)
    for fn in ("td3_update", "td3_update_from_ring", "td3_update_ring_loop", "td3_explore_action", "Td3Spec"):
        assert hasattr(ops, fn)
    src = open(os.path.join(ROOT, "elegantrl_amd", "ops.py")).read()
    for name in NAMES:
        assert name in src, f"ops.py never calls {name}"


def test_param_counts_and_workspace_query():
    from elegantrl_amd import _hip, ops
    L = _hip.lib()
    h, nh = _hid(64, 32)
    pa, pc = ctypes.c_int64(0), ctypes.c_int64(0)
    assert L.erl_td3_param_counts(S, A, h, nh, E, ctypes.byref(pa), ctypes.byref(pc)) == 0
    assert pa.value == 11 * 64 + 64 + 64 * 32 + 32 + 32 * 3 + 3 and pc.value == 14 * 64 + 64 + 64 * 32 + 32 + 32 * 8 + 8
    spec = ops.Td3Spec(S, A, [64, 32], E)
    assert (spec.actor_count, spec.critic_count) == (pa.value, pc.value)
    assert spec.critic_slices()[-1] == ("net.4.bias", pc.value - 8, (8,)) and spec.actor_slices()[0] == ("net.0.weight", 0, (64, 11))
    for bad_E in (0, 9, -1):
        assert L.erl_td3_param_counts(S, A, h, nh, bad_E, None, None) == -1 and b"erl_td3_param_counts" in L.erl_last_error_string()
        assert L.erl_td3_workspace_bytes(S, A, h, nh, bad_E, B) == -1
    assert L.erl_td3_workspace_bytes(S, A, h, nh, E, 0) == -1 and L.erl_td3_workspace_bytes(S, A, None, nh, E, B) == -1
    h7, n7 = _hid(*[16] * 7)
    assert L.erl_td3_workspace_bytes(S, A, h7, n7, E, B) == -1                              # more than ERL_MAX_LAYERS hidden layers
    # monotone in B and in E (strictly in B)
    last = 0
    for b in (1, 2, 63, 64, 65, 255, 256, 257, 300, 1024, 4096, 65536):
        w = L.erl_td3_workspace_bytes(S, A, h, nh, E, b)
        assert w > last, (b, w, last)
        last = w
    for b in (1, 64, 300):
        sizes = [L.erl_td3_workspace_bytes(S, A, h, nh, e, b) for e in range(1, 9)]
        assert all(x > 0 for x in sizes) and sizes == sorted(sizes), (b, sizes)
    h3, n3 = _hid(64, 48, 32)
    assert L.erl_td3_workspace_bytes(S, A, h3, n3, E, B) > L.erl_td3_workspace_bytes(S, A, h, nh, E, B)


def _ring(p, row_floats, ids, max_size=64, num_seqs=8, sample_len=31):
    from elegantrl_amd.ops import _RingSample
    q = p if not row_floats else None
    return _RingSample(p, q, q, q, q, max_size, num_seqs, ids, sample_len, None, None, row_floats)


def _calls(p, ws_bytes, hid=(64, 32), E_=E, step=1, update_actor=1, actor_step=1, n_steps=3, freq=2, ring=None, B_=B, ids_all="p", std=0.1):
    """argument lists of the three update entries with `p` for every tensor"""
    h, nh = _hid(*hid)
    head = [p] * 8 + [S, A, h, nh, E_]
    r = ctypes.addressof(ring) if ring is not None else None
    fl = [std] + FLOATS[1:]
    return {
        "erl_td3_update_f32": head + [p] * 6 + [None, None, B_, None, 1, 1] + fl + [step, update_actor, actor_step, p, p, ws_bytes, None],
        "erl_td3_update_ring_f32": head + [r] + [p] * 6 + [B_, None, 1, 1] + fl + [step, update_actor, actor_step, p, p, ws_bytes, None],
        "erl_td3_update_ring_loop_f32": head + [r, p if ids_all == "p" else ids_all, n_steps] + [p] * 6 + [B_, 1, 1] + fl +
                                        [step, actor_step, freq, 1, p, None, p, ws_bytes, None],
    }


def test_update_entries_refuse_before_any_launch():
    from elegantrl_amd import _hip
    L = _hip.lib()
    err = L.erl_last_error_string
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16                        # (the interleaved ring's base must be 16-byte aligned)
    h, nh = _hid(64, 32)
    need = L.erl_td3_workspace_bytes(S, A, h, nh, E, B)
    assert need > 0
    rf = L.erl_replay_row_floats(S, A)
    good = _ring(p, rf, p)

    def refused(name, args, *words):
        rc = getattr(L, name)(*args)
        msg = err()
        assert rc == -1 and name.encode() in msg and all(w in msg for w in words), (name, rc, msg)

    for name in UPDATES:
        refused(name, _calls(None, need, ring=good)[name], b"NULL")                                     # NULL tensors
        refused(name, _calls(p, need - 1, ring=good)[name], b"workspace too small")                     # an undersized workspace
        refused(name, _calls(p, 0, ring=good)[name], b"workspace too small")
        for bad_E in (0, 9):
            refused(name, _calls(p, 1 << 40, E_=bad_E, ring=good)[name], b"E=%d" % bad_E)              # E < 1, E > 8
        refused(name, _calls(p, 1 << 40, hid=[16] * 7, ring=good)[name], b"unsupported dims")
        refused(name, _calls(p, need, step=0, ring=good)[name], b"step")                                # Adam steps are 1-based
        refused(name, _calls(p, 1 << 40, ring=good, B_=0)[name], b"B=0")
        refused(name, _calls(p, need, ring=good, std=-0.1)[name], b"policy_noise_std")
    for name in UPDATES[:2]:
        refused(name, _calls(p, need, ring=good, update_actor=1, actor_step=0)[name], b"actor_step=0")  # an actor update needs its Adam step
    planar = _ring(p, 0, p)
    planar.buf_unmasks = None                                                                           # a planar ring short of an array
    wrong_rf, no_base, no_rows, no_ids = _ring(p, rf + 4, p), _ring(None, rf, p), _ring(p, rf, p, sample_len=0), _ring(p, rf, None)
    unaligned = _ring(p + 4, rf, p)
    for name in UPDATES[1:]:                                           # (the ring structs stay alive: the calls take their addresses)
        refused(name, _calls(p, need, ring=None)[name], b"NULL ring")                                   # no ring at all
        refused(name, _calls(p, need, ring=wrong_rf)[name], b"row_floats")                              # row_floats is not the ring's
        refused(name, _calls(p, need, ring=unaligned)[name], b"row_floats")
        refused(name, _calls(p, need, ring=no_base)[name], b"NULL ring")
        refused(name, _calls(p, need, ring=planar)[name], b"NULL ring")
        refused(name, _calls(p, need, ring=no_rows)[name], b"bad ring shape")
    refused(UPDATES[1], _calls(p, need, ring=no_ids)[UPDATES[1]], b"NULL ring")                         # the single step reads ring->ids
    loop = UPDATES[2]
    for freq in (0, -2):
        refused(loop, _calls(p, need, ring=good, freq=freq)[loop], b"update_freq=%d" % freq)            # update_freq < 1
    refused(loop, _calls(p, need, ring=good, n_steps=-1)[loop], b"n_steps=-1")
    refused(loop, _calls(p, need, ring=good, actor_step=-1)[loop], b"actor_step0=-1")
    refused(loop, _calls(p, need, ring=good, ids_all=None)[loop], b"NULL")
    # zero steps: nothing to launch, the count of actor updates is written
    n = ctypes.c_int32(-7)
    a = _calls(p, need, ring=good, n_steps=0, actor_step=0)[loop]
    a[-4] = ctypes.byref(n)
    assert getattr(L, loop)(*a) == 0 and n.value == 0


def test_explore_action_refuses_before_any_launch():
    from elegantrl_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    h, nh = _hid(64, 32)
    name = "erl_td3_explore_action_f32"
    need = L.erl_td3_workspace_bytes(S, A, h, nh, 1, 5)

    def refused(args, word):
        rc = L.erl_td3_explore_action_f32(*args)
        msg = L.erl_last_error_string()
        assert rc == -1 and name.encode() in msg and word in msg, (rc, msg)

    ok = [p, S, A, h, nh, p, 5, None, 1, 1, 0.05, p, None, p, need, None]
    for i in (0, 5, 11, 13):
        a = list(ok)
        a[i] = None
        refused(a, b"NULL")
    refused(ok[:6] + [0] + ok[7:], b"bad N")
    refused(ok[:10] + [-1.0] + ok[11:], b"action_std")
    refused(ok[:14] + [16] + ok[15:], b"workspace too small")
    h7, n7 = _hid(*[16] * 7)
    refused(ok[:3] + [h7, n7] + ok[5:], b"unsupported dims")
