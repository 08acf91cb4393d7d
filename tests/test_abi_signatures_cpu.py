"""The ctypes table against the header, argument by argument (no GPU, nothing in the library is called): every `ERL_API` prototype of
include/erl_hip.h is parsed, each parameter mapped to a kind (pointer, 32-bit int, int64, uint64, uint32, float, double), and the
sequence compared with the kinds of `_hip._SIGNATURES[name][1]`.  A miscounted `[_P] * n` in the table is a silent stack mismatch on
the next call; here it is a failed comparison that names the symbol and the position."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "erl_hip.h")

SCALARS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint64_t": "u64", "uint32_t": "u32", "float": "f32", "double": "f64"}
CTYPES = {ctypes.c_int: "i32", ctypes.c_int32: "i32", ctypes.c_int64: "i64", ctypes.c_uint64: "u64", ctypes.c_uint32: "u32",
          ctypes.c_float: "f32", ctypes.c_double: "f64", ctypes.c_void_p: "ptr", ctypes.c_char_p: "ptr"}


def header_prototypes():
    """{name: [kind of each parameter]} of every ERL_API declaration"""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    out = {}
    for m in re.finditer(r"\bERL_API\s+[\w\s\*]+?\b(erl_\w+)\s*\(([^()]*)\)\s*;", txt):
        name, params = m.group(1), " ".join(m.group(2).split())
        assert name not in out, f"{name} is declared twice"
        kinds = []
        for p in ([] if params in ("", "void") else params.split(",")):
            p = p.strip()
            if "*" in p or "[" in p:
                kinds.append("ptr")
                continue
            words = [w for w in p.split() if w not in ("const", "unsigned", "signed")]
            assert len(words) == 2 and words[0] in SCALARS and "unsigned" not in p, f"{name}: cannot classify parameter `{p}`"
            kinds.append(SCALARS[words[0]])
        out[name] = kinds
    return out


def ctypes_kind(t):
    if t in CTYPES:
        return CTYPES[t]
    assert isinstance(t, type) and issubclass(t, ctypes._Pointer), f"no kind for argtype {t!r}"
    return "ptr"


def test_every_prototype_parses_and_the_names_are_the_table():
    from elegantrl_amd import _hip
    protos = header_prototypes()
    n_decl = len(re.findall(r"^ERL_API\b", open(HEADER).read(), flags=re.M))
    assert len(protos) == n_decl >= 100, (len(protos), n_decl)          # nothing the pattern above skipped
    assert set(protos) == set(_hip.EXPORTED_SYMBOLS), set(protos) ^ set(_hip.EXPORTED_SYMBOLS)
    assert len(_hip.EXPORTED_SYMBOLS) == len(set(_hip.EXPORTED_SYMBOLS))


def test_argument_kinds_match_the_header():
    from elegantrl_amd import _hip
    protos = header_prototypes()
    wrong = {}
    for name, (_, argtypes) in _hip._SIGNATURES.items():
        have, want = [ctypes_kind(t) for t in argtypes], protos[name]
        if have != want:
            at = next((i for i, (a, b) in enumerate(zip(have, want)) if a != b), min(len(have), len(want)))
            wrong[name] = f"{len(have)} argtypes against {len(want)} parameters, first difference at position {at}"
    assert not wrong, wrong
