"""Every prototype of include/ssamd.h against the ctypes ``restype`` / ``argtypes`` that ``_native.lib()`` declares, class by
class: a transposed int / double, or an ``int`` where the header says ``long long``, corrupts arguments silently."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double, "float": ctypes.c_float}


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "ssamd.h")) as f:
        return f.read()


def _prototypes(header):
    """{name: (return type, [parameter types])} with 'ptr' for any pointer; every statement of the header must parse"""
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
    text = text.replace('extern "C" {', " ").replace("}", " ")
    protos = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"(int|const char \*) ?(ssamd_[a-z0-9_]+) ?\((.*)\)", stmt)
        assert m, "not a prototype: %r" % stmt
        ret, name, params = m.groups()
        assert name not in protos, name
        kinds = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            p = p.strip()
            if "*" in p:
                kinds.append("ptr")
                continue
            words = [w for w in p.split() if w != "const"]
            assert len(words) >= 2, (name, p)                  # a type and the parameter's name
            kind = " ".join(words[:-1])
            assert kind in SCALARS, (name, p)
            kinds.append(kind)
        protos[name] = (ret, kinds)
    return protos


def _is_pointer_class(t):
    return t is ctypes.c_void_p or t is ctypes.c_char_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def test_parser_sees_every_entry_point(header):
    protos = _prototypes(header)
    declared = set(re.findall(r"\b(ssamd_[a-z0-9_]+)\s*\(", header))      # the regex of test_c_abi_exports_every_declared_symbol
    assert set(protos) == declared
    assert len(protos) == 54
    assert sorted(n for n, (_, kinds) in protos.items() if not kinds) == [
        "ssamd_abi_version", "ssamd_device_count", "ssamd_last_error", "ssamd_profile_reset"]
    assert protos["ssamd_np_unwrap"] == ("int", ["ptr", "long long", "long long", "long long", "double", "double", "ptr", "int"])
    assert protos["ssamd_gsw"][1][7:11] == ["int", "float", "int", "int"]


def test_every_prototype_matches_its_ctypes_declaration(header):
    from simplestereo_amd import _native
    lib = _native.lib()
    protos = _prototypes(header)
    for name, (ret, kinds) in sorted(protos.items()):
        fn = getattr(lib, name)
        assert fn.restype is (ctypes.c_char_p if ret == "const char *" else ctypes.c_int), name
        assert fn.argtypes is not None, "%s has no argtypes" % name
        assert len(fn.argtypes) == len(kinds), name
        for i, (t, kind) in enumerate(zip(fn.argtypes, kinds)):
            if kind == "ptr":
                assert _is_pointer_class(t), (name, i, t)
            else:
                assert t is SCALARS[kind], (name, i, t, kind)


def test_constants_match_the_header(header):
    from simplestereo_amd import _native
    codes = dict(re.findall(r"#define SSAMD_(OK|E[A-Z]+) \(?(-?\d+)\)?", header))
    assert sorted(codes) == ["EHIP", "EINVAL", "ELIMIT", "ENODEVICE", "ENOMEM", "OK"]
    for k, v in codes.items():
        assert getattr(_native, k) == int(v), k
    slots = {k: int(v) for k, v in re.findall(r"#define SSAMD_(K_[A-Z_0-9]+) (\d+)", header)}
    assert slots["K_COUNT"] == _native.K_COUNT == len(slots) - 1
    assert {k for k in dir(_native) if k.startswith("K_")} == set(slots)
    for k, v in slots.items():
        assert getattr(_native, k) == v, k
