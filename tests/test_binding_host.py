"""The Python binding takes every signature from the headers (transit_amd._abi.bind): the binder covers every prototype
of both headers, the signatures most likely to break a parser are spelled out here by hand, every structure of
include/transit_hip.h agrees with its ctypes mirror field by field, and Engine and Batch know the shapes of their installed
sets from the constructor on.  No GPU: the libraries are only loaded."""
import ctypes as C
import os
import re

import pytest

from transit_amd import _abi, build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, I32, I64 = C.c_double, C.c_int32, C.c_int64
DP, I32P, I64P, VP = C.POINTER(D), C.POINTER(I32), C.POINTER(I64), C.c_void_p
ATM, OPTS, DBG = C.POINTER(_abi.TrxAtm), C.POINTER(_abi.TrxOpts), C.POINTER(_abi.TrxDebug)


def stripped(path):
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def hip_lib():
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    return C.CDLL(path)


@pytest.mark.parametrize("header,prefix,load,atleast", [(_abi.HIP_HEADER, "trx_", hip_lib, 72),
                                                      (_abi.HOST_HEADER, "trh_", lambda: C.CDLL(build.build_host()), 31)])
def test_every_prototype_of_a_header_is_bound(header, prefix, load, atleast):
    txt = stripped(header)
    # every `name(` of the prefix outside comments, the callback's typedef `(*trx_log_fn)(` not being one; with the text
    # between the parentheses, counted by its commas
    found = {m.group(1): m.group(2) for m in re.finditer(r"\b(%s[a-z_0-9]+)\s*\(([^()]*)\)\s*;" % prefix, txt)}
    assert len(found) >= atleast
    lib = _abi.bind(load(), header, prefix)
    for name, args in found.items():
        fn = getattr(lib, name)
        nargs = 0 if args.strip() in ("", "void") else args.count(",") + 1
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        ret = re.search(r"([\w \t*]+?)\s*\b%s\s*\(" % name, txt).group(1).replace("const", "").split()
        if ret == ["int"]:
            assert fn.restype is C.c_int, name
        elif ret == ["void"]:
            assert fn.restype is None, name
        elif ret == ["char", "*"]:
            assert fn.restype is C.c_char_p, name
        elif ret == ["int64_t"]:
            assert fn.restype is I64, name
        else:                                               # transit_host.h hands out the plain structures
            assert ret[1:] == ["*"] and fn.restype is C.POINTER(getattr(_abi, "".join(w.capitalize() for w in ret[0].split("_")))), name
    if prefix == "trx_":
        assert {fn.restype for fn in (getattr(lib, n) for n in found)} == {C.c_int, C.c_char_p, None}
    assert _abi.prototypes(header, prefix) is _abi.prototypes(header, prefix)          # parsed once


def test_a_type_the_binder_does_not_know_is_an_error(tmp_path):
    ok = "typedef struct trx_handle trx_handle;\nint trx_fine(trx_handle *h, const double *x /* [n] */, int32_t n);\n"
    assert _abi.parse(ok, "trx_") == {"trx_fine": (C.c_int, [VP, DP, I32])}
    for bad in ("int trx_odd(trx_handle *h, const long double *x);", "int trx_odd(trx_handle *h, trx_nosuch *s);",
                "int trx_odd(trx_handle *h, trx_atm a);", "uint64_t trx_odd(trx_handle *h);"):
        with pytest.raises(ValueError, match="trx_odd"):
            _abi.parse(ok + bad, "trx_")
    path = tmp_path / "odd.h"
    path.write_text(ok + "int trx_odd(trx_handle *h, size_t n);\n")

    class Lib:
        pass
    with pytest.raises(ValueError, match="trx_odd, argument 2.*size_t"):
        _abi.bind(Lib(), str(path), "trx_")


def test_the_signatures_a_parser_breaks_first():
    lib = _abi.bind(hip_lib(), _abi.HIP_HEADER, "trx_")
    want = {
        "trx_normalise_observed": [VP, ATM, OPTS, DP, I32, DP, I32, D, D, DP, DP, DP, I64P, I64P, DBG],
        "trx_pca_observed": [VP, ATM, OPTS, DP, I32, DP, C.POINTER(_abi.TrxPca), DP, DP, DP, DP, DP, I64P, I64P, DBG],
        "trx_run_batch_velocity_map": [VP, I32, ATM, OPTS, C.POINTER(_abi.TrxVmap), C.POINTER(DP), C.POINTER(DP)],
        "trx_create": [C.POINTER(_abi.TrxStatic), C.POINTER(VP)],
        "trx_set_log": [_abi.LOG_FN, VP, C.c_int],
        "trx_sweep_permol": [VP, I32, DP, DP, DP, D, I32, I32P, DP],
        "trx_table_copy": [VP, C.POINTER(C.c_float)],
        "trx_restore_extinction": [VP, I32, DP, C.POINTER(C.c_uint8)],
    }
    for name, args in want.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args, name
        assert fn.restype is (None if name == "trx_set_log" else C.c_int), name
    assert _abi.LOG_FN is engine.LOG_FN
    assert _abi.LOG_FN._restype_ is None and list(_abi.LOG_FN._argtypes_) == [C.c_int, C.c_char_p, VP]
    assert lib.trx_last_error.restype is C.c_char_p and list(lib.trx_last_error.argtypes) == [VP]
    assert lib.trx_abi_version() == 5 and list(lib.trx_abi_version.argtypes) == []


SCALARS = {"int32_t": I32, "int64_t": I64, "double": D, "float": C.c_float, "int16_t": C.c_int16, "uint8_t": C.c_uint8}


def header_structs():
    """[(trx_name, [(field, ctypes type), ...])] of every `typedef struct { ... } trx_name;` of include/transit_hip.h"""
    out = []
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(trx_\w+)\s*;", stripped(_abi.HIP_HEADER), flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.replace("const", " ").split())
            if not decl:
                continue
            base, rest = decl.split(" ", 1)
            for d in rest.split(","):                      # `int32_t nwave, ntemp`, `const double *wn`, `int32_t mol[2]`
                m = re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[(\d+)\])?\s*", d)
                assert m, (name, decl)
                stars, field, length = len(m.group(1)), m.group(2), m.group(3)
                assert stars <= 1, (name, decl)
                if base == "void":
                    assert stars == 1 and not length
                    t = VP
                else:
                    t = SCALARS[base] if base in SCALARS else getattr(_abi, "".join(w.capitalize() for w in base.split("_")))
                    t = C.POINTER(t) if stars else t
                    t = t * int(length) if length else t
                fields.append((field, t))
        out.append((name, fields))
    return out


def test_every_structure_of_the_header_agrees_with_its_ctypes_mirror():
    structs = header_structs()
    names = [n for n, _ in structs]
    declared = re.findall(r"\}\s*(trx_\w+)\s*;", re.sub(r"typedef\s+enum\s*\{.*?\}\s*\w+\s*;", " ", stripped(_abi.HIP_HEADER), flags=re.S))
    assert names == declared and len(names) == len(set(names)) == 21
    mirrors = {n for n, v in vars(_abi).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    assert {"".join(w.capitalize() for w in n.split("_")) for n in names} == mirrors
    compared = 0
    for name, fields in structs:
        cls = getattr(_abi, "".join(w.capitalize() for w in name.split("_")))
        assert [f for f, _ in cls._fields_] == [f for f, _ in fields], name
        for (field, got), (_, want) in zip(cls._fields_, fields):
            assert got is want, (name, field, got, want)
        compared += 1
    assert compared == 21
    # the parser of this test on the declarations that can fool it: an array, several declarators, one-line structures
    byname = dict(structs)
    assert byname["trx_cia"][:4] == [("nspec", I32), ("mol", I32 * 2), ("nwave", I32), ("ntemp", I32)]
    assert byname["trx_scatter"] == [("kind", I32), ("min_live", I32), ("clip", D)]
    assert ("cia", C.POINTER(_abi.TrxCia)) in byname["trx_static"] and ("comm", VP) in byname["trx_static"]
    assert byname["trx_stats"][-2:] == [("ms_k_walk_form", D * 3), ("ms_walk_span", D)]


class StubLibrary:
    """every trx_ function succeeds and does nothing"""

    def __getattr__(self, name):
        if not name.startswith("trx_"):
            raise AttributeError(name)
        return lambda *args: 0


@pytest.mark.parametrize("make", [engine.Engine, lambda st: engine.Batch(st, ways=2)], ids=["Engine", "Batch"])
def test_the_shapes_of_the_installed_sets_are_there_from_the_constructor_on(monkeypatch, make):
    monkeypatch.setattr(engine, "_hip", StubLibrary())
    obj = make(_abi.TrxStatic())
    assert {"nbands", "npix", "mom_shape"} <= set(vars(obj))
    assert (obj.nbands, obj.npix, obj.mom_shape) == (0, 0, (0, 0))
    for cls in (engine.Engine, engine.Batch):
        assert not any(hasattr(cls, a) for a in ("nbands", "npix", "mom_shape"))        # instance state, set in __init__


def test_the_family_under_another_prefix():
    """bind_engine_api(lib, prefix): the header's trx_ signatures on a library that exports the family as <prefix>name"""
    class Other:
        pass
    other = Other()
    family = ("create", "run", "destroy", "get_stats", "table_info", "table_copy", "width_grids", "sweep_permol")
    for name in family:
        setattr(other, "abc_" + name, Other())
    assert _abi.bind_engine_api(other, "abc_") is other
    want = _abi.prototypes(_abi.HIP_HEADER, "trx_")
    for name in family:
        fn = getattr(other, "abc_" + name)
        assert (fn.restype, fn.argtypes) == want["trx_" + name], name
    assert _abi.parse("int\ntrx_split(\n  int32_t n);", "trx_") == {"trx_split": (C.c_int, [I32])}      # a return type on its own line
    assert not hasattr(_abi, "bind_trail_api")
