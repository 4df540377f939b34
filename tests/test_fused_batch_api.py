"""CPU-side checks of the fused batch entry points (cvh_enqueue_steps_batch, cvh_run_batch): declared, exported, bound, and the
argument errors that are decided before any device is touched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cvh_enqueue_steps_batch", "cvh_run_batch")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi as m
    return m


def test_header_declares_batch_entry_points():
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert re.search(r"int\s+cvh_enqueue_steps_batch\s*\(\s*cvh_context\s*\*\s*const\s*\*\s*ctxs\s*,\s*int\s+n\s*,\s*int\s+nsteps\s*\)\s*;", hdr)
    assert re.search(r"int\s+cvh_run_batch\s*\(\s*cvh_context\s*\*\s*const\s*\*\s*ctxs\s*,\s*int\s+n\s*,\s*int\s+max_steps\s*,"
                     r"\s*int\s*\*\s*steps_done\s*,\s*double\s*\*\s*last_norm\s*\)\s*;", hdr)


def test_library_exports_batch_entry_points(capi):
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name


def test_capi_binds_batch_entry_points(capi):
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, name
    assert callable(capi.run_batch) and callable(capi.enqueue_steps_batch)


def test_empty_or_negative_member_list_is_refused_without_a_device(capi):
    L = capi.lib()
    err_arg = 1   # CVH_ERR_ARG
    assert L.cvh_run_batch(None, 0, 5, None, None) == err_arg
    assert b"member list" in L.cvh_last_error(None)
    assert L.cvh_run_batch(None, -1, 5, None, None) == err_arg
    arr = (ctypes.c_void_p * 1)(None)
    assert L.cvh_run_batch(arr, -1, 5, None, None) == err_arg
    assert L.cvh_enqueue_steps_batch(None, 0, 5) == err_arg
    assert L.cvh_enqueue_steps_batch(arr, -1, 5) == err_arg
    assert L.cvh_enqueue_steps_batch(arr, 1, 5) == err_arg          # a NULL member
    assert b"member 0" in L.cvh_last_error(None)
    with pytest.raises(capi.CvhError) as e:
        capi.run_batch([], 5)
    assert e.value.code == err_arg
    with pytest.raises(capi.CvhError) as e:
        capi.enqueue_steps_batch([], 5)
    assert e.value.code == err_arg
