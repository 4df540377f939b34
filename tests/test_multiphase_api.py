"""CPU side of the four-phase calls (include/chanvese_hip.h, "Four phases"): the boundary -- header, exports, bindings --, what the
library refuses before it touches a device, and the partition the sums are taken over (pure host arithmetic)."""
import ctypes
import os
import re

import pytest

import multiphase_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cvh_multiphase_run", "cvh_multiphase_means", "cvh_multiphase_labels", "cvh_multiphase_labels_device", "cvh_multiphase_geometry")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def test_header_declares_and_library_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert "---- Four phases ----" in hdr
    declared = set(re.findall(r"^(?:int|void) (cvh_multiphase_\w+)\(", hdr, flags=re.M))
    assert declared == set(NAMES)
    assert re.search(r"int cvh_multiphase_run\(cvh_context \*a, cvh_context \*b, int max_steps, int \*steps_done, double \*norms /\* 2 \*/, "
                     r"double \*trace, int trace_rows,\s+int \*rows\);", hdr)
    assert re.search(r"int cvh_multiphase_means\(cvh_context \*a, cvh_context \*b, double \*c /\* 4 C \*/\);", hdr)
    assert re.search(r"int cvh_multiphase_labels\(cvh_context \*a, cvh_context \*b, uint8_t \*labels\);", hdr)
    assert re.search(r"int cvh_multiphase_labels_device\(cvh_context \*a, cvh_context \*b, uint8_t \*d_labels, void \*stream\);", hdr)
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in capi.EXPORTS
    # every symbol the header declares is bound, and nothing else
    assert set(capi.EXPORTS) == set(re.findall(r"^[\w \*]+?\b(cvh_\w+)\(", hdr, flags=re.M))


def test_ctypes_signatures(capi):
    L = capi.lib()
    vp, ip, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    assert L.cvh_multiphase_run.argtypes == [vp, vp, ctypes.c_int, ip, dp, dp, ctypes.c_int, ip] and L.cvh_multiphase_run.restype is ctypes.c_int
    assert L.cvh_multiphase_means.argtypes == [vp, vp, dp]
    assert L.cvh_multiphase_labels.argtypes == [vp, vp, ctypes.POINTER(ctypes.c_uint8)]
    assert L.cvh_multiphase_labels_device.argtypes == [vp, vp, vp, vp]
    assert L.cvh_multiphase_geometry.argtypes == [ctypes.c_int, ctypes.c_int, ip, ip, ip] and L.cvh_multiphase_geometry.restype is None


def test_null_pairs_are_refused_without_a_device(capi):
    L = capi.lib()
    out = (ctypes.c_double * 12)()
    lab = (ctypes.c_uint8 * 4)()
    for name, call in (("cvh_multiphase_run", lambda: L.cvh_multiphase_run(None, None, 1, None, None, None, 0, None)),
                       ("cvh_multiphase_means", lambda: L.cvh_multiphase_means(None, None, out)),
                       ("cvh_multiphase_labels", lambda: L.cvh_multiphase_labels(None, None, lab)),
                       ("cvh_multiphase_labels_device", lambda: L.cvh_multiphase_labels_device(None, None, None, None))):
        assert call() == 1   # CVH_ERR_ARG
        assert L.cvh_last_error(None).decode().startswith(name + ": context a is NULL")


def test_driver_checks_its_arguments_first(capi):
    if capi.device_count() == 0:   # (no context without a device: as every other call)
        with pytest.raises(capi.CvhError) as e:
            capi.Context(16, 16)
        assert "no HIP device" in str(e.value)
    with pytest.raises(ValueError):
        capi.multiphase_run(None, None, max_steps=-1, trace=True)   # all rows of an unbounded run: refused before the library is reached


def test_partition_is_a_function_of_the_shape(capi):
    """61 output columns per wave; about 4096 waves; strips of a multiple of four rows, at least 8 -- and what multiphase_util restates"""
    g = capi.multiphase_geometry
    assert g(M.SEAM_H, 130) == (61, M.SEAM_H - 1, 2 * 3) and g(8, 130) == (61, 8, 3)
    assert g(24, 64) == (61, 8, 3 * 2) and g(24, 61) == (61, 8, 3)
    assert g(4096, 4096) == (61, 72, 57 * 68)
    assert g(1024, 1024) == (61, 8, 128 * 17)
    assert g(1 << 14, 1 << 14)[1:] == (0, 0) and g(0, 5)[1:] == (0, 0)       # not planes the calls take
    for h, w, _, _ in M.CASES:
        cols, rows, items = g(h, w)
        assert rows == M.strip_rows(h, w) and rows % 4 == 0 and rows >= 8 and items == -(-h // rows) * -(-w // cols)
    for h, w in ((4096, 4096), (1024, 1024), (100000, 7), (33, 2000)):
        assert g(h, w)[1] == M.strip_rows(h, w)
