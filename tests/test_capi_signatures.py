"""The signature table of chan_vese_amd/_abi.py against include/chanvese_hip.h, declaration by declaration: the names, the number of
arguments, the return type and the kind of every argument.  Needs the built library for lib() only; runs nothing on a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


@pytest.fixture(scope="module")
def declarations():
    """{name: (return type, [parameter declarations])} of the header, its /* */ comments stripped"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chanvese_hip.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^([\w \*]+?)\b(cvh_\w+)\(([^;{}]*?)\);", hdr, flags=re.M):
        params = [" ".join(p.split()) for p in m.group(3).split(",")]
        out[m.group(2)] = (" ".join(m.group(1).split()), [] if params == ["void"] else params)
    return out


def is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def test_exports_are_the_headers_declarations(capi, declarations):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert set(capi.EXPORTS) == set(re.findall(r"^[\w \*]+?\b(cvh_\w+)\(", hdr, flags=re.M))   # (the pattern of test_multiphase_api.py)
    assert set(capi.EXPORTS) == set(declarations) and len(capi.EXPORTS) == len(set(capi.EXPORTS)) == len(declarations)
    assert capi.EXPORTS == list(capi.SIGNATURES)


def test_every_signature_agrees_with_its_declaration(capi, declarations):
    L = capi.lib()
    wrong = []
    for name in capi.EXPORTS:
        returns, params = declarations[name]
        fn = getattr(L, name)
        want = None if returns.endswith("void") else ctypes.c_char_p if returns.endswith("const char *") else ctypes.c_int
        if fn.restype is not want:
            wrong.append(f"{name}: returns {returns!r}, bound as {fn.restype}")
        if len(fn.argtypes) != len(params):
            wrong.append(f"{name}: {len(params)} parameters, {len(fn.argtypes)} argtypes")
            continue
        for k, (decl, bound) in enumerate(zip(params, fn.argtypes)):
            if "*" in decl:
                ok = is_pointer(bound)
            else:
                base = [w for w in decl.split()[:-1] if w != "const"]
                ok = len(base) == 1 and SCALARS.get(base[0]) is bound
            if not ok:
                wrong.append(f"{name}: argument {k} {decl!r} bound as {bound}")
    assert not wrong, "\n".join(wrong)
