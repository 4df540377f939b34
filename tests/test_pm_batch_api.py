"""CPU-side checks of the Perona-Malik batch (cvh_perona_malik_batch): declared, exported, bound, and the argument errors that are
decided before any device is touched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cvh_perona_malik_batch"
ERR_ARG = 1   # CVH_ERR_ARG


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi as m
    return m


def test_header_declares_pm_batch():
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert re.search(r"int\s+cvh_perona_malik_batch\s*\(\s*cvh_context\s*\*\s*const\s*\*\s*ctxs\s*,\s*int\s+n\s*,\s*const\s+double\s*\*\s*K\s*,"
                     r"\s*const\s+double\s*\*\s*L\s*,\s*const\s+double\s*\*\s*T\s*\)\s*;", hdr)


def test_library_exports_pm_batch(capi):
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), NAME)


def test_capi_binds_pm_batch(capi):
    assert NAME in capi.EXPORTS
    fn = getattr(capi.lib(), NAME)
    assert fn.restype is ctypes.c_int and fn.argtypes is not None and len(fn.argtypes) == 5
    assert callable(capi.perona_malik_batch)


def test_empty_negative_or_null_member_is_refused_without_a_device(capi):
    L = capi.lib()
    v = (ctypes.c_double * 2)(30.0, 30.0)
    lam = (ctypes.c_double * 2)(0.25, 0.25)
    t = (ctypes.c_double * 2)(1.0, 1.0)
    assert L.cvh_perona_malik_batch(None, 0, v, lam, t) == ERR_ARG
    assert b"member" in L.cvh_last_error(None)
    arr = (ctypes.c_void_p * 2)(None, None)
    assert L.cvh_perona_malik_batch(arr, 0, v, lam, t) == ERR_ARG
    assert b"member" in L.cvh_last_error(None)
    assert L.cvh_perona_malik_batch(arr, -3, v, lam, t) == ERR_ARG
    assert b"member" in L.cvh_last_error(None)
    assert L.cvh_perona_malik_batch(arr, 2, v, lam, t) == ERR_ARG     # a NULL member
    assert b"member 0" in L.cvh_last_error(None)
    with pytest.raises(capi.CvhError) as e:
        capi.perona_malik_batch([], 30, 0.25, 1.0)
    assert e.value.code == ERR_ARG and "member" in str(e.value)
