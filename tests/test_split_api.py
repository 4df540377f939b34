"""CPU side of the object split (include/chanvese_hip.h, "Object split"): the boundary -- header, exports, the geometry call, what is
refused before a device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cvh_split", "cvh_split_batch", "cvh_split_levelset", "cvh_split_levelset_batch")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def test_header_declares_and_library_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert "---- Object split ----" in hdr
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", hdr), name
    assert re.search(r"int cvh_split\(cvh_context \*ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest, uint32_t r2, "
                     r"int32_t \*d_labels,\s+cvh_component \*table, int cap, int \*count, void \*stream\);", hdr)
    assert re.search(r"int cvh_split_batch\(cvh_context \*const \*ctxs, int n, int conn, int invert, long min_area, long fill_holes, int keep_largest,\s+"
                     r"const uint32_t \*r2, int32_t \*const \*d_labels, int \*counts, void \*stream\);", hdr)
    for text in ("M = E  u  { p in F0", "(d << 32) | L", "ANY order of relaxation", "some 8-neighbour q of p has L(q) > L(p)", "ceil(sweeps / 4)",
                 "8 bytes per pixel of the plane rounded up to whole tiles"):
        assert text in hdr, text
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW + ("cvh_split_geometry",):
        assert hasattr(raw, name) and name in capi.EXPORTS, name
    for name in ("cvh_debug_split_launch_sets", "cvh_debug_split_sweeps"):
        fn = getattr(raw, name)
        fn.restype = ctypes.c_ulong
        assert fn() >= 0


def test_the_geometry_call(capi):
    tr, tc, group = capi.split_geometry()
    assert tr >= 8 and tc >= 16 and tc % 2 == 0 and group >= 1          # (two 64-bit keys make a 16-byte piece)
    capi.lib().cvh_split_geometry(None, None, None)                       # any output may be NULL


def test_null_arguments_are_refused_without_a_device(capi):
    L = capi.lib()
    ptrs = (ctypes.c_void_p * 1)(None)
    r2 = (ctypes.c_uint32 * 1)(1)
    assert L.cvh_split(None, 4, 0, 0, 0, 0, 1, None, None, 0, None, None) != capi.CVH_OK
    assert L.cvh_split_levelset(None, 4, 0, 0, 0, 0, 1, 1.0, -1.0) != capi.CVH_OK
    for ctxs, n in ((None, 1), ((ctypes.c_void_p * 1)(None), 1), ((ctypes.c_void_p * 1)(None), 0)):
        assert L.cvh_split_batch(ctxs, n, 4, 0, 0, 0, 0, r2, ptrs, None, None) != capi.CVH_OK
        assert b"cvh_split_batch" in L.cvh_last_error(None)
        assert L.cvh_split_levelset_batch(ctxs, n, 4, 0, 0, 0, 0, r2, 1.0, -1.0) != capi.CVH_OK
        assert b"cvh_split_levelset_batch" in L.cvh_last_error(None)
    for call in (lambda: capi.split_batch([], r2=1), lambda: capi.split_levelset_batch([], r2=1)):
        with pytest.raises(capi.CvhError):
            call()
    for bad in (dict(r2=-1), dict(r2=2 ** 32), dict(r2=1, radius=1.0), dict(radius=-1.0)):
        with pytest.raises(ValueError):
            capi.split_batch([object()], **bad)


def test_split_without_gpu_fails_as_other_calls_do(capi):
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CvhError) as e:
        capi.Context(16, 16).split(r2=1)
    assert "no HIP device" in str(e.value)
