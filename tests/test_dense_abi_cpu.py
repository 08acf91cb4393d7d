"""CPU-side checks of the direct dense-layer entries (csrc/mlpn.hip, erl_dense_*): the four symbols in the header, the binding and the
library; every refusal returns nonzero with the entry's own name in the message before anything is launched (there is no device here, and
the dummy non-NULL host address is never dereferenced; out_form keeps the value it had); the workspace query is monotone in rows."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("erl_dense_forward_f32", "erl_dense_backward_input_f32", "erl_dense_weight_grad_workspace_bytes", "erl_dense_weight_grad_f32")
QUERY = NAMES[2]
ENTRIES = (NAMES[0], NAMES[1], NAMES[3])


def test_the_four_symbols_are_declared_bound_and_exported():
    from elegantrl_amd import _hip, ops
    from tests.test_abi_signatures_cpu import ctypes_kind, header_prototypes
    txt = open(os.path.join(ROOT, "include", "erl_hip.h")).read()
    protos = header_prototypes()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NAMES:
        assert name in _hip.EXPORTED_SYMBOLS and re.search(r"ERL_API \w+ " + name + r"\(", txt), name
        assert hasattr(raw, name) and getattr(_hip.lib(), name) is not None
        res, argtypes = _hip._SIGNATURES[name]
        assert [ctypes_kind(t) for t in argtypes] == protos[name], name
        assert res is (ctypes.c_int64 if name == QUERY else ctypes.c_int)
    for fn in ("dense_forward", "dense_backward_input", "dense_weight_grad", "dense_weight_grad_workspace_bytes"):
        assert hasattr(ops, fn)
    src = open(os.path.join(ROOT, "elegantrl_amd", "ops.py")).read()
    for name in NAMES:
        assert name in src, f"ops.py never calls {name}"
    assert _hip.lib().erl_abi_version() == _hip.ABI_VERSION == 23        # additive: the ABI number stays


def _calls(p, rows=64, Nw=8, K=8, ws=None, ws_bytes=0, form=None, nulls=()):
    """argument lists of the three entries with `p` for every tensor; nulls: positions to pass as NULL"""
    a = {
        "erl_dense_forward_f32": [p, p, p, p, None, rows, Nw, K, 1, form, None],
        "erl_dense_backward_input_f32": [p, p, p, None, 0, rows, Nw, K, form, None],
        "erl_dense_weight_grad_f32": [p, p, p, p, rows, Nw, K, ws, ws_bytes, form, None],
    }
    for name, args in a.items():
        for i in nulls:
            if i < 4 and args[i] is not None:
                args[i] = None
    return a


REQUIRED = {"erl_dense_forward_f32": (0, 1, 2, 3), "erl_dense_backward_input_f32": (0, 1, 2), "erl_dense_weight_grad_f32": (0, 1, 2, 3)}


def test_entries_refuse_before_any_launch():
    from elegantrl_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    form = ctypes.c_int(-7)
    fp = ctypes.byref(form)

    def refused(name, args, *words):
        rc = getattr(L, name)(*args)
        msg = L.erl_last_error_string()
        assert rc == -1 and name.encode() in msg and all(w in msg for w in words), (name, rc, msg)
        assert form.value == -7, name                                   # nothing was chosen, nothing launched

    for name in ENTRIES:
        for i in REQUIRED[name]:
            refused(name, _calls(p, form=fp, nulls=(i,))[name], b"NULL")
        for bad in ({"rows": 0}, {"rows": -1}, {"Nw": 0}, {"K": 0}, {"Nw": -3}, {"K": -1}):
            refused(name, _calls(p, form=fp, **bad)[name], b"bad shape")
        refused(name, _calls(p, form=fp, Nw=_hip.MAXN_WIDTH + 1)[name], b"bad shape", b"4096")
        refused(name, _calls(p, form=fp, K=_hip.MAXN_WIDTH + 1)[name], b"bad shape", b"4096")
        refused(name, _calls(p, form=fp, K=4100, Nw=4)[name], b"bad shape", b"4096")
        refused(name, _calls(p, form=fp, rows=1 << 31)[name], b"bad shape", b"2^31")
        refused(name, _calls(p, form=fp, rows=(1 << 40) + 5)[name], b"bad shape", b"2^31")
    # a gate and accumulate at once
    a = _calls(p, form=fp)["erl_dense_backward_input_f32"]
    a[3], a[4] = p, 1
    refused("erl_dense_backward_input_f32", a, b"gate")
    # a workspace that is too small (a NULL workspace is the unsplit path and needs no bytes)
    name = "erl_dense_weight_grad_f32"
    for rows, Nw, K in ((1024, 3, 5), (4097, 64, 256), (1 << 20, 130, 130)):
        need = L.erl_dense_weight_grad_workspace_bytes(rows, Nw, K)
        assert need > 0
        for have in (0, 16, need - 1, -1):
            refused(name, _calls(p, rows=rows, Nw=Nw, K=K, ws=p, ws_bytes=have, form=fp)[name], b"workspace too small")


def test_workspace_query():
    from elegantrl_amd import _hip
    L = _hip.lib()
    q = L.erl_dense_weight_grad_workspace_bytes
    for bad in ((0, 8, 8), (-1, 8, 8), (64, 0, 8), (64, 8, 0), (64, _hip.MAXN_WIDTH + 1, 8), (64, 8, _hip.MAXN_WIDTH + 1), (1 << 31, 8, 8)):
        assert q(*bad) == -1 and QUERY.encode() in L.erl_last_error_string(), bad
    for Nw, K in ((1, 1), (3, 5), (64, 256), (257, 63), (4, 4036), (4096, 4096)):
        last = 0
        for rows in (1, 2, 255, 256, 1023, 1024, 1025, 1279, 1280, 1281, 4096, 65536, (1 << 31) - 1):
            w = q(rows, Nw, K)
            assert w >= last and (w > 0) == (rows >= 1024), (rows, Nw, K, w, last)       # monotone; below 1024 rows nothing is split
            if rows >= 1024:
                splits = -(-rows // 256)
                assert w >= 4 * splits * (Nw * K + 2 * Nw), (rows, Nw, K, w)             # the dW partials, a db partial in either layout
                assert w % 256 == 0
            last = w
        assert q(1024, Nw, K) < q(1025, Nw, K)                                           # a fifth chunk
