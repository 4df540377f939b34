"""CPU side of the contours (include/chanvese_hip.h, "Contours"): the header section, the three exports, the numpy dtype against the C
struct (32 bytes), and what is refused before a device is touched.  The refusals that need a context are in tests/test_gpu_contour.py."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
NAMES = ("cvh_contours", "cvh_contours_device", "cvh_contours_device_batch")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def test_header_declares_and_library_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert "---- Contours ----" in hdr
    clean = r"int conn, int invert, long min_area, long fill_holes, int keep_largest,\s+int simplify,\s+"
    assert re.search(r"int cvh_contours\(cvh_context \*ctx, " + clean + r"cvh_contour_loop \*loops, long loop_cap, int32_t \*points, long point_cap, "
                     r"long \*nloops, long \*npoints\);", hdr)
    assert re.search(r"int cvh_contours_device\(cvh_context \*ctx, " + clean + r"cvh_contour_loop \*loops, long loop_cap, int32_t \*d_points, "
                     r"long point_cap, long \*nloops, long \*npoints,\s+void \*stream\);", hdr)
    assert re.search(r"int cvh_contours_device_batch\(cvh_context \*const \*ctxs, int n, " + clean + r"cvh_contour_loop \*const \*loops, "
                     r"const long \*loop_caps, int32_t \*const \*d_points,\s+const long \*point_caps, long \*nloops, long \*npoints, void \*stream\);", hdr)
    for text in ("4 (r w + c) + k", "left turn for conn = 8 and the right turn for conn = 4", "Host waits: TWO", "6 bytes per pixel",
                 "45 bytes per edge", "h w >= 2^30"):
        assert text in hdr, text
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in capi.EXPORTS


def test_struct_layout_matches_the_header(capi, tmp_path):
    dt = capi.CONTOUR_LOOP_DTYPE
    src = tmp_path / "layout.c"
    body = '  printf("%zu", sizeof(cvh_contour_loop));\n' + "".join(f'  printf(" %zu", offsetof(cvh_contour_loop, {f}));\n' for f in dt.names)
    src.write_text('#include "chanvese_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' + body + "  return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    line = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout
    assert [int(x) for x in line.split()] == [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    assert dt.itemsize == 32 and dt.names == ("first", "edges", "points", "pad", "offset", "area2")


def test_refused_before_a_device_is_touched(capi):
    L = capi.lib()
    nl, npts = ctypes.c_long(7), ctypes.c_long(7)
    assert L.cvh_contours(None, 8, 0, 0, 0, 0, 1, None, 0, None, 0, ctypes.byref(nl), ctypes.byref(npts)) == ERR_ARG
    assert L.cvh_contours_device(None, 8, 0, 0, 0, 0, 1, None, 0, None, 0, ctypes.byref(nl), ctypes.byref(npts), None) == ERR_ARG
    assert (nl.value, npts.value) == (7, 7)
    assert L.cvh_contours_device_batch(None, 0, 8, 0, 0, 0, 0, 1, None, None, None, None, None, None, None) == ERR_ARG
    assert b"cvh_contours_device_batch: empty member list" in L.cvh_last_error(None)
    arr = (ctypes.c_void_p * 1)(None)
    assert L.cvh_contours_device_batch(arr, 1, 8, 0, 0, 0, 0, 1, None, None, None, None, None, None, None) == ERR_ARG
    assert b"cvh_contours_device_batch: member 0 is NULL" in L.cvh_last_error(None)


def test_trip_arithmetic(capi):
    """the sections contour_run.hip gives a member (host arithmetic): a lane of the edge launches takes about four edges and at most sixteen pixels (192 x 320 pixels: 15 workgroups)"""
    raw = ctypes.CDLL(capi.LIB_PATH)
    pb, st, eb, el = ctypes.c_uint(), ctypes.c_uint(), ctypes.c_uint(), ctypes.c_ulonglong()
    for edges, blocks in ((0, 0), (1, 15), (15 * 1024 + 1, 16), (61000, 60), (1 << 26, 2048)):
        assert raw.cvh_debug_contour_trips(192, 320, ctypes.c_ulonglong(edges), ctypes.byref(pb), ctypes.byref(st), ctypes.byref(eb), ctypes.byref(el)) == 0
        assert (pb.value, st.value, eb.value, el.value) == (240, 64, blocks, 256 * blocks)
