"""CPU side of the subpixel contours (include/chanvese_hip.h, "Subpixel contours"): the header section and prototypes, the four exports,
what is refused before a device is touched, and the host-only helper cvh_contour_subpixel_measure against its restatement in Python
floats with ==.  The refusals that need a context are in tests/test_gpu_subpixel.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import subpixel_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
NAMES = ("cvh_contours_subpixel", "cvh_contours_subpixel_device", "cvh_contours_subpixel_device_batch", "cvh_contour_subpixel_measure")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def test_header_declares_and_library_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert hdr.index("---- Contours ----") < hdr.index("---- Subpixel contours ----") < hdr.index("---- Mask morphology ----")
    clean = r"int conn, int invert, long min_area, long fill_holes, int keep_largest,\s+"
    assert re.search(r"int cvh_contours_subpixel\(cvh_context \*ctx, " + clean + r"cvh_contour_loop \*loops, long loop_cap, double \*points, "
                     r"long point_cap, long \*nloops, long \*npoints\);", hdr)
    assert re.search(r"int cvh_contours_subpixel_device\(cvh_context \*ctx, " + clean + r"cvh_contour_loop \*loops, long loop_cap, double \*d_points, "
                     r"long point_cap, long \*nloops, long \*npoints,\s+void \*stream\);", hdr)
    assert re.search(r"int cvh_contours_subpixel_device_batch\(cvh_context \*const \*ctxs, int n, " + clean + r"cvh_contour_loop \*const \*loops, "
                     r"const long \*loop_caps, double \*const \*d_points,\s+const long \*point_caps, long \*nloops, long \*npoints, void \*stream\);", hdr)
    assert "int cvh_contour_subpixel_measure(const double *points, long n, double *area, double *length);" in hdr
    section = hdr[hdr.index("---- Subpixel contours ----"):hdr.index("---- Mask morphology ----")]
    for text in ("t = a / (a - b), one IEEE division", "a > 0 AND b <= 0 AND a - b is finite", "otherwise t = 0.5", "8-byte aligned",
                 "16 bytes per point", "After cvh_reinit every point is its edge's MIDPOINT", "lives in the evolved u", "simplify = 0",
                 "x = (c + 0.5) + dx t", "accumulated left to right"):
        assert text in section, text
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in capi.EXPORTS
    assert callable(capi.Context.contours_subpixel) and callable(capi.contours_subpixel_batch) and callable(capi.contour_subpixel_measures)


def test_refused_before_a_device_is_touched(capi):
    """a NULL context, an empty or NULL member list -- with negative caps or without -- are CVH_ERR_ARG and write nothing"""
    L = capi.lib()
    nl, npts = ctypes.c_long(7), ctypes.c_long(7)
    for lcap, pcap in ((0, 0), (-1, 0), (0, -4)):
        assert L.cvh_contours_subpixel(None, 8, 0, 0, 0, 0, None, lcap, None, pcap, ctypes.byref(nl), ctypes.byref(npts)) == ERR_ARG
        assert L.cvh_contours_subpixel_device(None, 8, 0, 0, 0, 0, None, lcap, None, pcap, ctypes.byref(nl), ctypes.byref(npts), None) == ERR_ARG
    assert (nl.value, npts.value) == (7, 7)
    for n in (0, -3):
        assert L.cvh_contours_subpixel_device_batch(None, n, 8, 0, 0, 0, 0, None, None, None, None, None, None, None) == ERR_ARG
        assert b"cvh_contours_subpixel_device_batch: empty member list" in L.cvh_last_error(None)
    arr = (ctypes.c_void_p * 1)(None)
    caps = (ctypes.c_long * 1)(-1)
    assert L.cvh_contours_subpixel_device_batch(arr, 1, 8, 0, 0, 0, 0, None, caps, None, caps, None, None, None) == ERR_ARG
    assert b"cvh_contours_subpixel_device_batch: member 0 is NULL" in L.cvh_last_error(None)


def c_measure(capi, pts, n=None):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
    buf = np.concatenate([pts.reshape(-1), [777.0]])   # (never empty: an address for n = 0)
    a, ln = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
    assert capi.lib().cvh_contour_subpixel_measure(buf.ctypes.data, pts.shape[0] if n is None else n, ctypes.byref(a), ctypes.byref(ln)) == 0
    return a.value, ln.value


def test_measure_helper_equals_its_restatement(capi):
    assert c_measure(capi, np.zeros((0, 2))) == (0.0, 0.0) == su.measure(np.zeros((0, 2)))
    assert c_measure(capi, [[3.25, -1.5]]) == (0.0, 0.0) == su.measure([[3.25, -1.5]])
    square = [[1.0, 1.0], [3.0, 1.0], [3.0, 3.0], [1.0, 3.0]]            # the order of an outer loop: the foreground on the right, y downwards
    assert c_measure(capi, square) == (4.0, 8.0) == su.measure(square)
    assert c_measure(capi, square[::-1]) == (-4.0, 8.0) == su.measure(square[::-1])   # a hole
    assert c_measure(capi, square, 2) == su.measure(square[:2]) == (0.0, 4.0)
    rng = np.random.default_rng(9)
    for n in (2, 3, 17, 1000):
        pts = rng.uniform(-50, 900, (n, 2))
        assert c_measure(capi, pts) == su.measure(pts), n
    loops, pts = su.trace_subpixel(su.disk(64), 8)
    assert c_measure(capi, pts) == su.measure(pts)
    # loop by loop through the binding: an outer boundary and its hole, with the signs of area2
    m = np.zeros((12, 12), bool)
    m[2:10, 2:10] = True
    m[5:7, 5:7] = False
    loops, pts = su.trace_subpixel(su.from_mask(m, 4), 8)
    area, length = capi.contour_subpixel_measures(loops, pts)
    assert loops.size == 2 and area.dtype == length.dtype == np.float64
    for k, l in enumerate(loops):
        o, n = int(l["offset"]), int(l["points"])
        assert (area[k], length[k]) == su.measure(pts[o:o + n])
        assert np.sign(area[k]) == np.sign(int(l["area2"]))
    assert area[0] > 0 > area[1]
    empty = capi.contour_subpixel_measures(loops[:0], pts[:0])
    assert empty[0].size == 0 and empty[1].size == 0


def test_measure_helper_refusals(capi):
    L = capi.lib()
    pts = np.zeros(8)
    a, ln = ctypes.c_double(5.0), ctypes.c_double(5.0)
    assert L.cvh_contour_subpixel_measure(pts.ctypes.data, -1, ctypes.byref(a), ctypes.byref(ln)) == ERR_ARG
    assert L.cvh_contour_subpixel_measure(None, 4, ctypes.byref(a), ctypes.byref(ln)) == ERR_ARG
    assert L.cvh_contour_subpixel_measure(None, 0, ctypes.byref(a), ctypes.byref(ln)) == ERR_ARG
    assert L.cvh_contour_subpixel_measure(pts.ctypes.data, 4, None, ctypes.byref(ln)) == ERR_ARG
    assert L.cvh_contour_subpixel_measure(pts.ctypes.data, 4, ctypes.byref(a), None) == ERR_ARG
    assert (a.value, ln.value) == (5.0, 5.0)
