"""CPU side of the localised-regions calls (include/chanvese_hip.h, "Localised regions"): the boundary -- header, exports, bindings --,
what the library refuses before it touches a device, and the partition the norm is summed over (pure host arithmetic)."""
import ctypes
import os
import re

import pytest

import localized_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cvh_localized_run", "cvh_localized_means", "cvh_localized_geometry")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def test_header_declares_and_library_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert "---- Localised regions ----" in hdr
    assert set(re.findall(r"^(?:int|void) (cvh_localized_\w+)\(", hdr, flags=re.M)) == set(NAMES)
    assert re.search(r"int cvh_localized_run\(cvh_context \*ctx, int radius, int max_steps, int \*steps_done, double \*norm, double \*trace, "
                     r"int trace_rows, int \*rows\);", hdr)
    assert re.search(r"int cvh_localized_means\(cvh_context \*ctx, int radius, double \*c1, double \*c2, uint64_t \*wq, uint64_t \*a, uint64_t \*s\);", hdr)
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in capi.EXPORTS
    for name in ("localized_run", "localized_geometry"):
        assert callable(getattr(capi, name))
    assert callable(capi.Context.localized_means)


def test_ctypes_signatures(capi):
    L = capi.lib()
    vp, ip, dp, ci = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double), ctypes.c_int
    assert L.cvh_localized_run.argtypes == [vp, ci, ci, ip, dp, dp, ci, ip] and L.cvh_localized_run.restype is ci
    assert L.cvh_localized_means.argtypes == [vp, ci, dp, dp, vp, vp, vp] and L.cvh_localized_means.restype is ci
    assert L.cvh_localized_geometry.argtypes == [ci, ci, ci, ip, ip, ip, ip] and L.cvh_localized_geometry.restype is None


def test_refusals_that_need_no_device(capi):
    L = capi.lib()
    out = (ctypes.c_double * 4)()
    assert L.cvh_localized_run(None, 3, 1, None, None, None, 0, None) == 1    # CVH_ERR_ARG
    assert L.cvh_localized_means(None, 3, out, None, None, None, None) == 1
    with pytest.raises(ValueError):
        capi.localized_run(None, 3, max_steps=-1, trace=True)   # all rows of an unbounded run: refused before the library is reached


def test_partition(capi):
    """61 output columns per wave; items of a multiple of four rows, at least 8, for about 4096 waves: a function of h and w alone; a
    strip is the smallest whole number of items with at least 2 (2 R + 1) rows, capped at the plane"""
    g = capi.localized_geometry
    assert g(U.SEAM_H, 130, U.SEAM_R) == (61, 8, 2 * 3, 8) and g(U.ITEM_H, 70, U.ITEM_R) == (61, 8, 4 * 2, 24)
    assert g(4096, 4096, 2) == (61, 72, 57 * 68, 72) and g(4096, 4096, 32) == (61, 72, 57 * 68, 144) and g(4096, 4096, 127)[3] == 576
    assert g(1024, 1024, 10) == (61, 8, 128 * 17, 48)
    assert g(9, 300, 127) == (61, 8, 2 * 5, 16)                               # capped: one strip holds the plane
    for bad in ((1 << 14, 1 << 14, 3), (0, 5, 3), (16, 16, 0), (16, 16, 128)):
        assert g(*bad)[1:] == (0, 0, 0)                                       # not what the calls take
    shapes = [(h, w, r) for h, w, _, r, _ in U.CASES] + [(4096, 4096, 10), (2048, 2048, 127), (100000, 7, 50), (33, 2000, 1)]
    for h, w, r in shapes:
        got = g(h, w, r)
        assert got == U.geometry(h, w, r)
        assert got[:3] == g(h, w, 1)[:3] == g(h, w, 127)[:3]                  # the items do not depend on the radius
        assert got[3] % got[1] == 0 and (got[3] >= 2 * (2 * r + 1) or got[3] >= h)
